"""Export the atoms of the reference's four 1ATN poses to a small .npz (data, not code).

Run once where the reference checkout is, with its PDB directory as the argument:
    python tests/golden/gen/export_atoms.py <reference>/tests/data/pdb/1ATN
Source: 1ATN_{1,2,3,4}w.pdb there, the poses the graphs 1ATN_{1..4}w of tests/golden/fixture_1ATN.npz were
generated from.  Output: tests/golden/atoms_1ATN.npz with arrays only:
    mols            the four names
    res_names       the distinct residue names, sorted
    res_chain       uint8 [R]   0: chain A, 1: chain B            (residues in file order: each is one run of ATOM records)
    res_seq         int32 [R]
    res_name_index  int8  [R]   into res_names
    atom_ptr        int32 [R+1] atom range of each residue
    xyz_milli       int32 [4, T, 3] coordinates in milli-angstrom (exact: the files carry three decimals)
The four files must have the same topology; the script stops if they do not.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
from deeprank_gnn_amd.interface import read_pdb_atoms  # noqa: E402

MOLS = ["1ATN_1w", "1ATN_2w", "1ATN_3w", "1ATN_4w"]
DST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "atoms_1ATN.npz")


def main(src):
    topo, coords = None, []
    for mol in MOLS:
        chain, seq, name, xyz = read_pdb_atoms(os.path.join(src, mol + ".pdb"))
        milli = np.rint(xyz * 1000.0).astype(np.int32)
        assert np.array_equal(milli / 1000.0, xyz), "coordinates with more than three decimals"
        if topo is None:
            topo = (chain, seq, name)
        assert all(np.array_equal(a, b) for a, b in zip(topo, (chain, seq, name))), mol + ": another topology"
        coords.append(milli)
    chain, seq, name = topo
    assert set(chain.tolist()) == {"A", "B"}
    start = np.flatnonzero(np.r_[True, (chain[1:] != chain[:-1]) | (seq[1:] != seq[:-1])])
    keys = list(zip(chain[start].tolist(), seq[start].tolist()))
    assert len(set(keys)) == len(keys), "a residue split over several runs of records"
    res_names = np.array(sorted(set(name.tolist())))
    np.savez_compressed(DST, mols=np.array(MOLS), res_names=res_names,
                        res_chain=(chain[start] == "B").astype(np.uint8), res_seq=seq[start].astype(np.int32),
                        res_name_index=np.searchsorted(res_names, name[start]).astype(np.int8),
                        atom_ptr=np.r_[start, len(chain)].astype(np.int32), xyz_milli=np.stack(coords))
    print("wrote", os.path.normpath(DST), len(start), "residues", len(chain), "atoms")


if __name__ == "__main__":
    main(sys.argv[1])
