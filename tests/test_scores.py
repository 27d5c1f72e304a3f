"""Docking scores (drgnn_score.h, deeprank_gnn_amd.interface.docking_scores) on the host-emulation build: the float64
reference of tests/score_ref.py against the values the reference recorded for the four 1ATN poses, then the kernel
against score_ref on 1ATN, on hand-made complexes, under rigid motions, across the class thresholds, batch / chunk
independence, refusals and the way from atoms to a trained net.  CPU only; tests/test_gpu_scores.py runs the same checks
on the device."""
import numpy as np
import pytest

import score_cases as C


@pytest.fixture(scope="module")
def api():
    from emu_api import emu
    return emu()


def test_score_ref_reproduces_the_recorded_scores():
    """fnat within 1e-6, irmsd and lrmsd within 1.5e-3 A, dockQ within 2e-6 of what the reference stored (three
    decimals for the RMSDs, six for the others); 68 pairs and zones of 448 / 1476 / 1032 atoms"""
    case, record = C.atn()
    want = case.want()
    assert len(case.ref.pairs) == 68
    for m, w in enumerate(want):
        assert w["n_ref_pairs"] == 68 and w["zone_sizes"] == (448, 1476, 1032)
        print(record["mols"][m], {k: w[k] for k in ("fnat", "irmsd", "lrmsd", "dockQ")})
        assert abs(w["fnat"] - record["fnat"][m]) <= 1e-6
        assert abs(w["irmsd"] - record["irmsd"][m]) <= 1.5e-3 and abs(w["lrmsd"] - record["lrmsd"][m]) <= 1.5e-3
        assert abs(w["dockQ"] - record["dockQ"][m]) <= 2e-6
        assert bool(w["binclass"]) == bool(record["binclass"][m])


def test_1ATN_poses_equal_score_ref(api):
    C.check_atn(api, "cpu")


@pytest.mark.parametrize("k", range(3), ids=["main", "zone3", "planar"])
def test_hand_made_complex_equals_score_ref(k, api):
    C.check_hand_case(C.hand_cases()[k], api, "cpu")


def test_rigid_motion_invariants(api):
    C.check_rigid_motion(api, "cpu")


def test_classes_across_the_thresholds(api):
    C.check_classes(api, "cpu")


def test_pose_results_do_not_depend_on_batch_or_chunk(api):
    C.check_independence(api, "cpu")


def test_bad_requests_are_refused_before_a_launch(api):
    C.check_refusals(api, "cpu")


def test_value_errors():
    C.check_value_errors()


def test_atom_names_are_optional_and_grouped():
    from deeprank_gnn_amd.interface import AtomTable
    chain, seq = np.array(list("BABAXBA")), np.array([7, 3, 7, 1, 1, 2, 3])
    name = np.array(["SER", "GLY", "SER", "ALA", "HOH", "UNK", "GLY"])
    xyz = np.arange(21, dtype=np.float64).reshape(7, 3)
    t = AtomTable(chain, seq, name, xyz, atom_name=np.array(["N", "CA", "CA", "C", "O", "CB", "N"]))
    assert t.atom_name.tolist() == ["CA", "N", "C", "N", "CA", "CB"]
    plain = AtomTable(chain, seq, name, xyz)
    assert plain.atom_name is None and plain.order.tolist() == t.order.tolist()
    with pytest.raises(ValueError):
        AtomTable(chain, seq, name, xyz, atom_name=np.array(["N"]))


def test_read_pdb_atom_names_follows_read_pdb_atoms(tmp_path):
    from deeprank_gnn_amd.interface import read_pdb_atom_names, read_pdb_atoms
    lines = ["HEADER    TEST",
             "ATOM      1  N   ALA A  11      -2.500   0.125   1.000  1.00  0.00",
             "ATOM      2  CA  ALA A  11      -1.500   0.125   1.000  1.00  0.00",
             "HETATM    3  O   HOH A  99       0.000   0.000   0.000  1.00  0.00",
             "ATOM      4 HD11 LEU B  21       2.500   1.000   1.000  1.00  0.00",
             "END"]
    path = tmp_path / "x.pdb"
    path.write_text("\n".join(lines) + "\n")
    names = read_pdb_atom_names(str(path))
    chain, seq, res, xyz = read_pdb_atoms(str(path))
    assert names.tolist() == ["N", "CA", "HD11"] and chain.tolist() == ["A", "A", "B"] and seq.tolist() == [11, 11, 21]
    assert res.tolist() == ["ALA", "ALA", "LEU"] and xyz.shape == (3, 3)


def test_atoms_to_targets_end_to_end(api, tmp_path):
    C.check_end_to_end(api, "cpu", tmp_path, {"_api": api, "device": "cpu"})
