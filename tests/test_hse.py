"""Half-sphere exposure (drgnn_hse.h, deeprank_gnn_amd.interface.residue_hse) on the host-emulation build: the float64
statement of the rule in tests/hse_ref.py against the values the reference recorded for the four 1ATN poses, then the
kernel against hse_ref on every residue of the four poses, on hand-made atoms, under rigid motions, batch / chunk / tile /
target-list independence, the capacity, refusals, and interface_graphs(hse=True).  CPU only; tests/test_gpu_hse.py runs
the same checks on the device."""
import numpy as np
import pytest

import hse_cases as C


@pytest.fixture(scope="module")
def api():
    from emu_api import emu
    return emu()


@pytest.mark.parametrize("connect", ["CA", "CN"])
def test_hse_ref_reproduces_the_recorded_hse(connect):
    """all 496 nodes of the four poses: counts equal, angles within 1e-9 rad (measured: 1.2e-15) of node_data/hse on the
    float32-rounded coordinates; exactly the chain-terminal nodes have zero rows.  No kernel: this pins the rule."""
    C.check_ref_against_recorded(connect)


def test_the_package_table_is_the_written_table():
    """hse_table against hse_ref.table_of on 1ATN and on hand-made residues with atoms missing"""
    from deeprank_gnn_amd.interface import hse_table
    bb = hse_table(C.atn()["table"])
    assert bb.dtype == np.int32 and np.array_equal(bb, C.atn_bb())
    assert ((bb[:, 4] & 4) != 0).sum() == 2 and (bb[:, 4] & 1).all() and ((bb[:, 4] & 2) != 0).sum() == (C.atn()["table"].res_name == "GLY").sum()
    for name in ("gly_without_n", "no_cb", "nonstandard_breaks"):
        t = C.hand_cases()[name][0].table()
        import hse_ref as R
        assert np.array_equal(hse_table(t), R.table_of(t.res_name, t.res_chain, t.atom_ptr, t.atom_name)), name


@pytest.mark.parametrize("opt", [{}, {"connect": "CN"}, {"direction": "CB"}], ids=["CA", "CN", "CB"])
def test_1ATN_residues_equal_hse_ref(api, opt):
    C.check_atn(api, "cpu", **opt)


@pytest.mark.parametrize("name", sorted(C.hand_cases()))
def test_hand_made_atoms_equal_hse_ref(name, api):
    C.check_hand_case(name, api, "cpu")


def test_rigid_motions(api):
    C.check_rigid_motion(api, "cpu")


def test_results_do_not_depend_on_batch_chunk_tile_place_or_targets(api):
    C.check_independence(api, "cpu")


def test_empty_target_list(api):
    C.check_empty_targets(api, "cpu")


def test_capacity_is_refused_not_wrong(api):
    C.check_capacity(api, "cpu")


def test_value_errors():
    C.check_value_errors()


@pytest.mark.parametrize("name", C.refusal_names())
def test_bad_requests_are_refused_before_a_launch(name, api):
    C.check_refusal(api, "cpu", name)


def test_interface_graphs_with_hse(api):
    C.check_graphs(api, "cpu", poses=(0,))
