"""lDDT and interface lDDT on the device (drgnn_lddt.h through libdrgnn.so): the checks of tests/test_lddt.py on the
MI355X, and the device's integers against the host emulation's, bit for bit."""
import pytest

import lddt_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


def test_1ATN_poses_equal_the_rule(api):
    C.check_atn(api, "cuda")


def test_hand_made_edges_equal_the_rule(api):
    C.check_edges(api, "cuda")


def test_residue_without_a_pair_is_zero_in_node_data(api):
    C.check_edges_node_data(api, "cuda")


@pytest.mark.parametrize("name", sorted(C.STARS))
def test_lane_and_stride_edges(name, api):
    C.check_star(name, api, "cuda")


def test_rigid_motion_and_count_invariants(api):
    C.check_rigid_motion(api, "cuda")


def test_pose_results_do_not_depend_on_batch_chunk_or_pass(api):
    C.check_independence(api, "cuda")


def test_device_equals_emulation(api):
    from emu_api import emu
    for case in C.device_cases():
        C.assert_bits_equal(case.run(api, "cuda"), case.run(emu(), "cpu"))


def test_bad_requests_are_refused_before_a_launch(api):
    C.check_refusals(api, "cuda")


def test_second_table_of_entry_points_and_the_record(api):
    C.check_binding(api)
    assert hasattr(api.lib, "drgnn_pose_lddt")


def test_atoms_to_lddt_targets_end_to_end(api):
    C.check_end_to_end(api, "cuda")
