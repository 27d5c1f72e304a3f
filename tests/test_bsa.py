"""Buried surface area (drgnn_bsa.h, deeprank_gnn_amd.interface.residue_bsa) on the host-emulation build: the float64
statement of the rule in tests/bsa_ref.py against the values the reference recorded for the four 1ATN poses, then the
kernel against bsa_ref on twelve node residues of one pose, on hand-made atoms, under rigid motions, batch / chunk /
target-list independence, refusals, and interface_graphs(bsa=True) up to the shipped checkpoints.  CPU only;
tests/test_gpu_bsa.py runs the same checks on the device, over all nodes of the four poses."""
import numpy as np
import pytest

import bsa_cases as C


@pytest.fixture(scope="module")
def api():
    from emu_api import emu
    return emu()


def test_bsa_ref_reproduces_the_recorded_bsa():
    """all 496 nodes of the four poses within 1e-9 A^2 of node_data/bsa (measured: 3.1e-12 at most); nodes are matched
    to residues by node_data/pos.  No kernel: this pins the rule and the two radius tables."""
    a = C.atn()
    assert sum(len(n) for n in a["nodes"]) == 496
    for m, mol in enumerate(a["mols"]):
        got = C.atn_ref(m, a["nodes"][m], rounded=False)[2]
        err = np.abs(got - a["recorded"][m]).max()
        print("%s: %d nodes, max |bsa_ref - recorded| = %.3g A^2, recorded %.3f .. %.3f"
              % (mol, len(got), err, a["recorded"][m].min(), a["recorded"][m].max()))
        assert err <= 1e-9
    assert min(r.min() for r in a["recorded"]) < -5.0 and max(r.max() for r in a["recorded"]) > 100.0


def test_the_package_tables_are_the_reference_tables():
    """bsa_radii against the tables written out in bsa_ref, atom for atom of 1ATN, and in the protor mode"""
    import bsa_ref as R
    from deeprank_gnn_amd.interface import bsa_radii
    t = C.atn()["table"]
    res = np.repeat(t.res_name, np.diff(t.atom_ptr))
    for mode in ("reference", "protor"):
        got, want = bsa_radii(t, mode), R.radii_of(res, t.atom_name, mode)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (bsa_radii(t)[0] == 0).sum() == sum(str(n).startswith("H") for n in t.atom_name) > 0
    explicit = bsa_radii(t, (np.arange(t.n_input_atoms), np.ones(t.n_input_atoms)))
    assert np.array_equal(explicit[0], t.order.astype(np.float64))          # input atom order -> grouped order


def test_1ATN_residues_equal_bsa_ref(api):
    C.check_atn(api, "cpu", [0], C.emu_subset())


@pytest.mark.parametrize("name", sorted(C.hand_cases()))
def test_hand_made_atoms_equal_bsa_ref(name, api):
    C.check_hand_case(name, api, "cpu")


def test_neighbour_capacity_is_refused_not_wrong(api):
    C.check_capacity(api, "cpu")


def test_empty_target_list(api):
    C.check_empty_targets(api, "cpu")


def test_other_slice_counts(api):
    C.check_other_slices(api, "cpu")


def test_rigid_motions(api):
    C.check_rigid_motion(api, "cpu")


def test_results_do_not_depend_on_batch_chunk_place_or_targets(api):
    C.check_independence(api, "cpu", C.emu_subset(), poses=(0, 1))


def test_value_errors():
    C.check_value_errors()


def test_bad_requests_are_refused_before_a_launch(api):
    C.check_refusals(api, "cpu")


def test_interface_graphs_with_bsa(api, tmp_path):
    C.check_graphs(api, "cpu", tmp_path, {"_api": api, "device": "cpu"}, poses=(0,))
