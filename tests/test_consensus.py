"""The contact consensus of docking poses (drgnn_consensus.h; deeprank_gnn_amd.interface.contact_frequency,
consensus_scores, consensus_contacts, PoseContacts.select, PoseClusters.consensus) on the host-emulation build: the numpy
statement of the rule in tests/consensus_ref.py against the literals of the four 1ATN poses and of the family batch, then
the kernels against it and against the row sums of common_contacts, all by exact equality: hand-packed words across the
word edges with clean and dirty tails, counters past 255 and 1023, groupings of every kind, another set scored against a
frequency, thresholds, select, independence of place / run / chunk, the capacities, refusals, the empty batch.  CPU only;
tests/test_gpu_consensus.py runs the same checks on the device."""
import pytest

import consensus_cases as C


@pytest.fixture(scope="module")
def api():
    from emu_api import emu
    return emu()


def test_consensus_ref_reproduces_the_1ATN_literals():
    C.check_ref_literals()


def test_the_family_batch_has_the_clusters_and_consensus_it_is_there_for():
    """on the reference alone: clusters of 45, 23, 22, 12 and 8 poses, 20 in none, two poses without contacts; 26 / 68 / 3
    consensus contacts of the set at 0.5 / 0.25 / 0.75; 58, 21, 99, 8, 90 of the clusters; a largest count of 117"""
    assert C.family()["counts"].max() == C.FAMILY_LARGEST


def test_numerators_are_the_row_sums_of_common_contacts(api):
    C.check_identity(api, "cpu")


def test_a_frequency_scores_another_set(api):
    C.check_other_set(api, "cpu")


@pytest.mark.parametrize("M", C.HAND_M)
@pytest.mark.parametrize("n_b", C.HAND_NB)
def test_hand_packed_words_and_dirty_tails(n_b, M, api):
    C.check_hand_packed(api, "cpu", n_b, M)


@pytest.mark.parametrize("M", C.ONES_M)
def test_all_ones_where_a_narrow_counter_wraps(M, api):
    C.check_all_ones(api, "cpu", M)


def test_groups_of_every_kind(api):
    C.check_groups(api, "cpu")


def test_leave_one_out_and_a_group_of_one(api):
    C.check_leave_one_out(api, "cpu")


def test_thresholds(api):
    C.check_thresholds(api, "cpu")


def test_select_carries_a_subset_into_clustering(api):
    C.check_select(api, "cpu")


def test_results_do_not_depend_on_place_run_or_chunk(api):
    C.check_independence(api, "cpu")


def test_capacity_is_refused_not_wrong(api):
    C.check_capacity(api, "cpu")


def test_consensus_scores_splits_at_the_capacity(api, monkeypatch):
    C.check_scores_are_split(api, "cpu", monkeypatch)


def test_empty_batch(api):
    C.check_empty_batch(api, "cpu")


def test_value_errors():
    C.check_value_errors()


@pytest.mark.parametrize("name", C.refusal_names())
def test_bad_requests_are_refused_before_a_launch(name, api):
    C.check_refusal(api, "cpu", name)
