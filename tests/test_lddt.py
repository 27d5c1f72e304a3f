"""lDDT and interface lDDT of docking poses (csrc/drgnn_lddt.h) on the host emulation: LddtReference, lddt_scores and
drgnn_pose_lddt against the numpy rule of tests/lddt_ref.py, integer for integer.  CPU only; tests/test_gpu_lddt.py runs
the same checks on the device."""
import pytest

import lddt_cases as C


@pytest.fixture(scope="module")
def api():
    from emu_api import emu
    return emu()


def test_1ATN_poses_equal_the_rule(api):
    C.check_atn(api, "cpu")


def test_hand_made_edges_equal_the_rule(api):
    C.check_edges(api, "cpu")


def test_residue_without_a_pair_is_zero_in_node_data(api):
    C.check_edges_node_data(api, "cpu")


@pytest.mark.parametrize("name", sorted(C.STARS))
def test_lane_and_stride_edges(name, api):
    C.check_star(name, api, "cpu")


def test_rigid_motion_and_count_invariants(api):
    C.check_rigid_motion(api, "cpu")


def test_pose_results_do_not_depend_on_batch_chunk_or_pass(api):
    C.check_independence(api, "cpu")


def test_bad_requests_are_refused_before_a_launch(api):
    C.check_refusals(api, "cpu")


def test_value_errors():
    C.check_value_errors()


def test_second_table_of_entry_points_and_the_record(api):
    C.check_binding(api)
    assert hasattr(api.lib, "drgnn_pose_lddt")


def test_atoms_to_lddt_targets_end_to_end(api):
    C.check_end_to_end(api, "cpu")
