"""Docking scores on the device (drgnn_score.h through libdrgnn.so): the checks of tests/test_scores.py on the MI355X,
two runs bit for bit, the device against the host emulation, and the way from atoms to a net trained on the scores."""
import pytest

import score_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


@pytest.fixture(scope="module")
def sweep(api):
    return C.check_classes(api, "cuda")


def test_1ATN_poses_equal_score_ref(api):
    C.check_atn(api, "cuda")


@pytest.mark.parametrize("k", range(3), ids=["main", "zone3", "planar"])
def test_hand_made_complex_equals_score_ref(k, api):
    C.check_hand_case(C.hand_cases()[k], api, "cuda")


def test_rigid_motion_invariants(api):
    C.check_rigid_motion(api, "cuda")


def test_classes_across_the_thresholds(sweep):
    assert sweep["irmsd"].shape == (64,)


def test_pose_results_do_not_depend_on_batch_or_chunk(api, sweep):
    C.check_independence(api, "cuda", sweep)


def test_repeat_runs_are_bit_identical(api, sweep):
    C.assert_bits_equal(sweep, C.sweep_case().run(api, "cuda"))
    case, _ = C.atn()
    C.assert_bits_equal(case.run(api, "cuda"), case.run(api, "cuda"))


def test_device_equals_emulation(api, sweep):
    from emu_api import emu
    C.assert_device_equals_emulation(sweep, C.sweep_case().run(emu(), "cpu"))
    case, _ = C.atn()
    C.assert_device_equals_emulation(case.run(api, "cuda"), case.run(emu(), "cpu"))
    for hand in C.hand_cases():
        C.assert_device_equals_emulation(hand.run(api, "cuda"), hand.run(emu(), "cpu"))


def test_bad_requests_are_refused_before_a_launch(api):
    C.check_refusals(api, "cuda")


def test_atoms_to_targets_end_to_end(api, tmp_path):
    C.check_end_to_end(api, "cuda", tmp_path)
