"""Buried surface area on the device (drgnn_bsa.h through libdrgnn.so): the checks of tests/test_bsa.py on the MI355X
over all nodes of the four 1ATN poses, two runs bit for bit, the device against the host emulation, and
interface_graphs(bsa=True) up to the shipped checkpoints."""
import numpy as np
import pytest

import bsa_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


@pytest.fixture(scope="module")
def subset():
    return C.emu_subset()


@pytest.fixture(scope="module")
def batch(api, subset):
    return C.check_independence(api, "cuda", subset)


def test_1ATN_nodes_equal_bsa_ref(api):
    C.check_atn(api, "cuda", [0, 1, 2, 3])


@pytest.mark.parametrize("name", sorted(C.hand_cases()))
def test_hand_made_atoms_equal_bsa_ref(name, api):
    C.check_hand_case(name, api, "cuda")


def test_neighbour_capacity_is_refused_not_wrong(api):
    C.check_capacity(api, "cuda")


def test_empty_target_list(api):
    C.check_empty_targets(api, "cuda")


def test_other_slice_counts(api):
    C.check_other_slices(api, "cuda")


def test_rigid_motions(api):
    C.check_rigid_motion(api, "cuda")


def test_results_do_not_depend_on_batch_chunk_place_or_targets(batch):
    assert batch[0].shape[0] == 3


def test_repeat_runs_are_bit_identical(api, batch, subset):
    from deeprank_gnn_amd.interface import AtomTable, residue_bsa
    a = C.atn()
    poses = AtomTable.poses(a["table"], a["xyz"][[0, 1, 2]])
    again = residue_bsa(poses, residues=subset, api=api, device="cuda", parts=True)
    assert all(C.same_bits(x[:, subset], y[:, subset]) for x, y in zip(batch, again))
    nodes = np.sort(a["nodes"][3])
    one = AtomTable.poses(a["table"], a["xyz"][[3]])
    runs = [residue_bsa(one, residues=nodes, api=api, device="cuda") for _ in range(3)]
    assert C.same_bits(runs[0], runs[1]) and C.same_bits(runs[0], runs[2])
    atoms = C.hand_cases()["ring_200"][0]
    assert C.same_bits(atoms.run(api, "cuda", [0])[0], atoms.run(api, "cuda", [0])[0])


def test_device_equals_emulation(api, batch, subset):
    from emu_api import emu
    from deeprank_gnn_amd.interface import AtomTable, residue_bsa
    a = C.atn()
    host = residue_bsa(AtomTable.poses(a["table"], a["xyz"][[0, 1, 2]]), residues=subset, api=emu(), device="cpu", parts=True)
    C.assert_device_equals_emulation(batch, host, subset)
    for name in ("crowd", "ring_200", "same_place"):
        atoms, targets, _ = C.hand_cases()[name]
        assert np.abs(atoms.run(api, "cuda", targets)[0] - atoms.run(emu(), "cpu", targets)[0]).max() <= C.TOL


def test_value_errors():
    C.check_value_errors()


def test_bad_requests_are_refused_before_a_launch(api):
    C.check_refusals(api, "cuda")


def test_interface_graphs_with_bsa(api, tmp_path):
    C.check_graphs(api, "cuda", tmp_path)
