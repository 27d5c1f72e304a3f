"""Residue depth on the device (drgnn_depth.h through libdrgnn.so): the checks of tests/test_depth.py on the MI355X at the
default 192 dots per atom on all four poses, the device against the host emulation, and the way through the layers."""
import pytest

import depth_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


@pytest.fixture(scope="module")
def batch(api):
    return C.check_independence(api, "cuda")


@pytest.mark.parametrize("pose", [0, 1, 2, 3])
def test_1ATN_nodes_equal_depth_ref(api, pose):
    C.check_atn(api, "cuda", pose)


@pytest.mark.parametrize("name", C.HAND_CASES)
def test_hand_made_atoms_equal_depth_ref(name, api):
    C.check_hand_case(name, api, "cuda")


@pytest.mark.parametrize("n_dots", C.DOT_COUNTS)
def test_dot_counts(n_dots, api):
    C.check_dot_count(api, "cuda", n_dots)


def test_results_do_not_depend_on_batch_chunk_targets_or_run(batch):
    assert batch.shape[0] == 3


def test_device_equals_emulation(api, batch):
    C.device_equals_emulation(api, batch)


def test_capacity_is_refused_not_wrong(api):
    C.check_capacity(api, "cuda")


def test_empty_target_list(api):
    C.check_empty_targets(api, "cuda")


@pytest.mark.parametrize("name", C.refusal_names())
def test_bad_requests_are_refused_before_a_launch(name, api):
    C.check_refusal(api, "cuda", name)


def test_interface_graphs_with_depth(api, tmp_path):
    C.check_graphs(api, "cuda", tmp_path, poses=(0, 1, 2, 3))


def test_resident_set_with_depth_equals_the_store_path(api):
    C.check_resident_set(api, "cuda")
