"""FCC clustering of docking poses on the device (drgnn_fcc.h through libdrgnn.so): the checks of tests/test_fcc.py on the
MI355X, two runs bit for bit, and the device against the host emulation, exactly."""
import pytest

import fcc_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


@pytest.fixture(scope="module")
def batch(api):
    return C.check_independence(api, "cuda")


def test_1ATN_poses_equal_fcc_ref_and_the_literals(api):
    C.check_atn(api, "cuda")


@pytest.mark.parametrize("name", sorted(C.hand_cases()))
def test_hand_made_atoms(name, api):
    C.check_hand_case(name, api, "cuda")


@pytest.mark.parametrize("n_b", [64, 65, 128, 129])
def test_word_boundaries_and_tail_bits(n_b, api):
    C.check_word_edges(api, "cuda", n_b)


def test_a_pose_without_contacts(api):
    C.check_no_contact_pose(api, "cuda")


@pytest.mark.parametrize("M", C.BATCH_SIZES)
def test_pose_batches_equal_fcc_ref(M, api):
    C.check_batch(api, "cuda", M)


def test_hand_written_relations(api):
    C.check_hand_relations(api, "cuda")


@pytest.mark.parametrize("M", [65, 130])
def test_both_rules_run_one_relation_and_one_greedy(M, api):
    C.check_one_relation_one_greedy(api, "cuda", M)


def test_results_do_not_depend_on_batch_chunk_place_or_run(batch):
    assert len(batch) == 17


def test_device_equals_emulation(api, batch):
    from emu_api import emu
    from deeprank_gnn_amd.interface import AtomTable, pose_contacts
    table, xyz = C.family_batch()
    C.assert_same_results(batch, pose_contacts(AtomTable.poses(table, xyz[:17]), api=emu(), device="cpu"))
    dev = pose_contacts(AtomTable.poses(table, xyz), api=api, device="cuda")
    C.assert_same_results(dev, pose_contacts(AtomTable.poses(table, xyz), api=emu(), device="cpu"))


def test_common_contacts_splits_at_the_capacity(api, monkeypatch):
    C.check_common_is_split(api, "cuda", monkeypatch)


def test_rigid_motions(api):
    C.check_rigid_motion(api, "cuda")


def test_capacity_is_refused_not_wrong(api):
    C.check_capacity(api, "cuda")


def test_empty_batch(api):
    C.check_empty_batch(api, "cuda")


def test_value_errors():
    C.check_value_errors()


@pytest.mark.parametrize("name", C.refusal_names())
def test_bad_requests_are_refused_before_a_launch(name, api):
    C.check_refusal(api, "cuda", name)
