"""Export what the docking-score tests need beyond tests/golden/atoms_1ATN.npz to a small .npz (data, not code).

Run once where the reference checkout is, with its tests/data directory as the argument:
    python tests/golden/gen/export_score_inputs.py <reference>/tests/data
Sources: pdb/1ATN/1ATN_1w.pdb (the atom names of the pose topology), ref/1ATN/1ATN.pdb.save (the reference structure
the scores are taken against) and tests/golden/fixture_1ATN.npz (the scores the reference recorded for the four
poses).  Output: tests/golden/scores_1ATN.npz with arrays only:
    atom_names       the distinct atom names of both structures, sorted
    pose_name_index  int16 [T]   into atom_names: the ATOM records of the poses, in the order atoms_1ATN.npz uses
    ref_chain        uint8 [N]   0: chain A, 1: chain B            (the reference structure's ATOM records, file order)
    ref_res_seq      int32 [N]
    ref_name_index   int16 [N]   into atom_names
    ref_xyz_milli    int32 [N,3] coordinates in milli-angstrom (exact: the file carries three decimals)
    mols             the four names
    fnat, irmsd, lrmsd, dockQ  float64 [4], binclass bool [4]: score/<key> of the four molecules in fixture_1ATN.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", ".."))
from deeprank_gnn_amd.interface import read_pdb_atom_names, read_pdb_atoms  # noqa: E402

MOLS = ["1ATN_1w", "1ATN_2w", "1ATN_3w", "1ATN_4w"]
DST = os.path.join(HERE, "..", "scores_1ATN.npz")


def main(src):
    pose = os.path.join(src, "pdb", "1ATN", MOLS[0] + ".pdb")
    ref = os.path.join(src, "ref", "1ATN", "1ATN.pdb.save")
    pose_names = read_pdb_atom_names(pose)
    with np.load(os.path.join(HERE, "..", "atoms_1ATN.npz")) as z:
        assert pose_names.shape[0] == z["xyz_milli"].shape[1], "not the topology of atoms_1ATN.npz"
    chain, seq, _, xyz = read_pdb_atoms(ref)
    ref_names = read_pdb_atom_names(ref)
    assert set(chain.tolist()) == {"A", "B"}
    milli = np.rint(xyz * 1000.0).astype(np.int32)
    assert np.array_equal(milli / 1000.0, xyz), "coordinates with more than three decimals"
    names = np.array(sorted(set(pose_names.tolist()) | set(ref_names.tolist())))
    out = {"atom_names": names, "pose_name_index": np.searchsorted(names, pose_names).astype(np.int16),
           "ref_chain": (chain == "B").astype(np.uint8), "ref_res_seq": seq.astype(np.int32),
           "ref_name_index": np.searchsorted(names, ref_names).astype(np.int16), "ref_xyz_milli": milli,
           "mols": np.array(MOLS)}
    with np.load(os.path.join(HERE, "..", "fixture_1ATN.npz")) as z:
        for k in ("fnat", "irmsd", "lrmsd", "dockQ", "binclass"):
            out[k] = np.array([z["%s/score/%s" % (m, k)][()] for m in MOLS])
    np.savez_compressed(DST, **out)
    print("wrote", os.path.normpath(DST), len(pose_names), "pose atoms", len(chain), "reference atoms")


if __name__ == "__main__":
    main(sys.argv[1])
