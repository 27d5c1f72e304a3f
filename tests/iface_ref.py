"""The interface-graph rule in numpy float64, with the project's canonical order: the plain statement that
drgnn_iface.h is held to (tests/test_iface.py, tests/test_gpu_iface.py).

One complex: xyz [T,3], atom_ptr [R+1] (atoms sorted by residue, chain A's residues first), split = number of chain-A
residues, res_type [R] (-1: non-standard).
    interface pair   a in A, b in B with an atom pair at d^2 < contact_distance^2 (strict); dist = min atom distance
    node             standard residue in a pair whose partner is standard too
    internal edge    nodes i < j of one chain with an atom pair at d^2 < internal_contact_distance^2 (strict)
Nodes by (chain, residue), interface edges (A node, B node) and internal edges (i < j) sorted by their pair; node ids
local to the complex.
"""
import numpy as np


def _min_d2(xa, pa, xb, pb):
    """[len(pa)-1, len(pb)-1] smallest squared distance between the atom groups of xa and xb (non-empty groups)"""
    d2 = np.zeros((xa.shape[0], xb.shape[0]))
    for k in range(3):
        d = xa[:, None, k] - xb[None, :, k]
        d2 += d * d
    return np.minimum.reduceat(np.minimum.reduceat(d2, pa[:-1], axis=0), pb[:-1], axis=1)


def interface_graph(xyz, atom_ptr, split, res_type, contact_distance=8.5, internal_contact_distance=3.0):
    xyz = np.asarray(xyz, dtype=np.float64)
    atom_ptr = np.asarray(atom_ptr, dtype=np.int64)
    res_type = np.asarray(res_type)
    R = len(atom_ptr) - 1
    assert np.all(np.diff(atom_ptr) > 0), "the reference statement takes non-empty residues"
    empty = {"node_residue": np.zeros(0, np.int64), "pos": np.zeros((0, 3)), "chain": np.zeros(0, np.int64),
             "type": np.zeros(0, np.int64), "edge_index": np.zeros((0, 2), np.int64), "dist": np.zeros(0),
             "internal_edge_index": np.zeros((0, 2), np.int64), "internal_dist": np.zeros(0)}
    if split == 0 or split == R:
        return empty
    cut = atom_ptr[split]
    pa, pb = atom_ptr[:split + 1], atom_ptr[split:] - cut
    m = _min_d2(xyz[:cut], pa, xyz[cut:], pb)
    ok = (m < contact_distance ** 2) & (res_type[:split, None] >= 0) & (res_type[None, split:] >= 0)
    is_node = np.concatenate((ok.any(axis=1), ok.any(axis=0)))
    nodes = np.flatnonzero(is_node)
    if nodes.size == 0:
        return empty
    local = np.cumsum(is_node) - 1
    ia, ib = np.nonzero(ok)                                            # row-major: sorted by (a, b)
    out = {"node_residue": nodes,
           "pos": np.array([xyz[atom_ptr[r]:atom_ptr[r + 1]].mean(axis=0) for r in nodes]),
           "chain": (nodes >= split).astype(np.int64), "type": res_type[nodes].astype(np.int64),
           "edge_index": np.stack((local[ia], local[split + ib]), axis=1), "dist": np.sqrt(m[ia, ib])}
    pairs, dist = [], []
    for lo, hi in ((0, split), (split, R)):
        sel = nodes[(nodes >= lo) & (nodes < hi)]
        if sel.size < 2:
            continue
        idx = np.concatenate([np.arange(atom_ptr[r], atom_ptr[r + 1]) for r in sel])
        ptr = np.concatenate(([0], np.cumsum(atom_ptr[sel + 1] - atom_ptr[sel])))
        mi = _min_d2(xyz[idx], ptr, xyz[idx], ptr)
        i, j = np.nonzero(np.triu(mi < internal_contact_distance ** 2, k=1))
        pairs.append(np.stack((local[sel[i]], local[sel[j]]), axis=1))
        dist.append(np.sqrt(mi[i, j]))
    out["internal_edge_index"] = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int64)
    out["internal_dist"] = np.concatenate(dist) if dist else np.zeros(0)
    return out


def as_fp32(g):
    """the reference result in the kernels' output types (coordinates on a 1/8 A grid make this exact)"""
    f32 = ("pos", "dist", "internal_dist")
    return {k: (v.astype(np.float32) if k in f32 else v.astype(np.int64)) for k, v in g.items()}
