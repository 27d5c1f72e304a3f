"""Half-sphere exposure on the device (drgnn_hse.h through libdrgnn.so): the checks of tests/test_hse.py on the MI355X, two
runs bit for bit, the device against the host emulation, and interface_graphs(hse=True) on the four poses."""
import numpy as np
import pytest

import hse_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


@pytest.fixture(scope="module")
def batch(api):
    return C.check_independence(api, "cuda")


@pytest.mark.parametrize("opt", [{}, {"connect": "CN"}, {"direction": "CB"}], ids=["CA", "CN", "CB"])
def test_1ATN_residues_equal_hse_ref(api, opt):
    C.check_atn(api, "cuda", **opt)


@pytest.mark.parametrize("name", sorted(C.hand_cases()))
def test_hand_made_atoms_equal_hse_ref(name, api):
    C.check_hand_case(name, api, "cuda")


def test_rigid_motions(api):
    C.check_rigid_motion(api, "cuda")


def test_results_do_not_depend_on_batch_chunk_tile_place_or_targets(batch):
    assert batch.shape == (3, 627, 3)


def test_repeat_runs_are_bit_identical(api, batch):
    from deeprank_gnn_amd.interface import AtomTable, residue_hse
    a = C.atn()
    poses = AtomTable.poses(a["table"], a["xyz"][[0, 1, 2]])
    for _ in range(2):
        assert C.same_bits(batch, residue_hse(poses, api=api, device="cuda"))
    atoms, opt, _ = C.hand_cases()["offset_3_radius_8"]
    assert C.same_bits(atoms.run(api, "cuda", **opt), atoms.run(api, "cuda", **opt))


def test_device_equals_emulation(api, batch):
    from emu_api import emu
    from deeprank_gnn_amd.interface import AtomTable, residue_hse
    a = C.atn()
    host = residue_hse(AtomTable.poses(a["table"], a["xyz"][[0, 1, 2]]), api=emu(), device="cpu")
    C.assert_device_equals_emulation(batch, host)
    for name in ("offset_3_radius_8", "gly_with_n_and_c", "cb_direction_gly", "collinear"):
        atoms, opt, _ = C.hand_cases()[name]
        C.equal_rows(atoms.run(api, "cuda", **opt), atoms.run(emu(), "cpu", **opt), name)


def test_empty_target_list(api):
    C.check_empty_targets(api, "cuda")


def test_capacity_is_refused_not_wrong(api):
    C.check_capacity(api, "cuda")


def test_value_errors():
    C.check_value_errors()


@pytest.mark.parametrize("name", C.refusal_names())
def test_bad_requests_are_refused_before_a_launch(name, api):
    C.check_refusal(api, "cuda", name)


def test_interface_graphs_with_hse(api):
    C.check_graphs(api, "cuda")
