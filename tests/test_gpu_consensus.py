"""The contact consensus of docking poses on the device (drgnn_consensus.h through libdrgnn.so): the checks of
tests/test_consensus.py on the MI355X, two runs bit for bit, and the device against the host emulation, exactly."""
import pytest

import consensus_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


@pytest.fixture(scope="module")
def batch(api):
    return C.check_independence(api, "cuda")


def test_numerators_are_the_row_sums_of_common_contacts(api):
    C.check_identity(api, "cuda")


def test_a_frequency_scores_another_set(api):
    C.check_other_set(api, "cuda")


@pytest.mark.parametrize("M", C.HAND_M)
@pytest.mark.parametrize("n_b", C.HAND_NB)
def test_hand_packed_words_and_dirty_tails(n_b, M, api):
    C.check_hand_packed(api, "cuda", n_b, M)


@pytest.mark.parametrize("M", C.ONES_M)
def test_all_ones_where_a_narrow_counter_wraps(M, api):
    C.check_all_ones(api, "cuda", M)


def test_groups_of_every_kind(api):
    C.check_groups(api, "cuda")


def test_leave_one_out_and_a_group_of_one(api):
    C.check_leave_one_out(api, "cuda")


def test_thresholds(api):
    C.check_thresholds(api, "cuda")


def test_select_carries_a_subset_into_clustering(api):
    C.check_select(api, "cuda")


def test_results_do_not_depend_on_place_run_or_chunk(batch):
    assert len(batch) == 6


def test_device_equals_emulation(api, batch):
    from emu_api import emu
    C.assert_same_results(batch, C.all_outputs(C.family_contacts(emu(), "cpu"), C.family()["labels"], 5))
    for n_b in C.HAND_NB:
        for M in C.HAND_M:
            C.assert_same_results(C.check_hand_packed(api, "cuda", n_b, M), C.check_hand_packed(emu(), "cpu", n_b, M))


def test_capacity_is_refused_not_wrong(api):
    C.check_capacity(api, "cuda")


def test_consensus_scores_splits_at_the_capacity(api, monkeypatch):
    C.check_scores_are_split(api, "cuda", monkeypatch)


def test_empty_batch(api):
    C.check_empty_batch(api, "cuda")


def test_value_errors():
    C.check_value_errors()


@pytest.mark.parametrize("name", C.refusal_names())
def test_bad_requests_are_refused_before_a_launch(name, api):
    C.check_refusal(api, "cuda", name)
