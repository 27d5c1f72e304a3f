"""The rule of FCC clustering (fraction of common contacts: Rodrigues et al. 2012, HADDOCK's cluster_fcc) as plain numpy:
what deeprank_gnn_amd.interface.pose_contacts / common_contacts / fcc_matrix / cluster_poses (csrc/drgnn_fcc.h) are held
to, by exact equality.  Float-free except where the rule itself has a float:

  contacts   residue pair (a of chain 0, b of chain 1) is a contact iff a counted atom of a and a counted atom of b have
             d2 <= cut2, with d2 = (dx*dx + dy*dy) + dz*dz in float32 on the float32 coordinates (numpy rounds every
             operation, nothing is fused) and cut2 = float32(float64(cutoff) * float64(cutoff)): the product in float64,
             then ONE rounding to float32.  Counted: every atom, or every atom that is not a hydrogen (the first character
             of its name that is neither a digit nor a blank is H).
  common     common[i, j] = |C_i & C_j|, int32; n_i = common[i, i]
  fcc        fcc[i, j] = common[i, j] / n_i, one float64 division; 0.0 where n_i == 0
  neighbour  j of i iff i != j and fcc[i, j] >= cutoff_fcc and fcc[j, i] >= cutoff_fcc * strictness (directed; the
             product once in float64)
  greedy     deg[i] = alive neighbours of i over the alive poses; the centre is the alive pose of largest deg, smallest
             index on a tie (HADDOCK leaves the tie to its sort; this is its rule with the tie made deterministic); stop
             when deg[centre] < min_size - 1; else the centre and its alive neighbours get the next label and die."""
import numpy as np


def is_hydrogen(name):
    return str(name).lstrip("0123456789 ")[:1] == "H"


def counted(atom_name, n_atoms, heavy_only):
    if not heavy_only:
        return np.ones(n_atoms, dtype=bool)
    return np.array([not is_hydrogen(n) for n in atom_name], dtype=bool).reshape(-1)


def cut2_of(cutoff):
    return np.float32(np.float64(cutoff) * np.float64(cutoff))


def contact_map(xyz, atom_ptr, split, count, cutoff=5.0):
    """bool [nA, nB] of one pose: xyz float32 [T, 3] grouped by atom_ptr [R+1], residues [0, split) chain 0"""
    x = np.asarray(xyz)
    assert x.dtype == np.float32
    R = len(atom_ptr) - 1
    res_of = np.repeat(np.arange(R), np.diff(atom_ptr))
    ia, ib = np.flatnonzero(count & (res_of < split)), np.flatnonzero(count & (res_of >= split))
    A, B = x[ia], x[ib]
    dx, dy, dz = (A[:, None, k] - B[None, :, k] for k in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    a, b = np.nonzero(d2 <= cut2_of(cutoff))
    out = np.zeros((split, R - split), dtype=bool)
    out[res_of[ia[a]], res_of[ib[b]] - split] = True
    return out


def pairs_of(cmap):
    """sorted int32 [n, 2] (residue of chain 0, residue of chain 1), indices into all residues"""
    a, b = np.nonzero(cmap)
    return np.stack((a, b + cmap.shape[0]), axis=1).astype(np.int32)


def common_of(maps_a, maps_b=None):
    """int32 [M, M2] from bool [M, nA, nB] contact maps"""
    fa = np.asarray(maps_a).reshape(len(maps_a), -1).astype(np.int32)
    fb = fa if maps_b is None else np.asarray(maps_b).reshape(len(maps_b), -1).astype(np.int32)
    return (fa @ fb.T).astype(np.int32)


def fcc_of(common, n):
    common, n = np.asarray(common), np.asarray(n)
    out = np.zeros(common.shape, dtype=np.float64)
    has = n > 0
    out[has] = common[has].astype(np.float64) / n[has].astype(np.float64)[:, None]
    return out


def neighbours_of(common, n, cutoff_fcc=0.6, strictness=0.75):
    """bool [M, M]: [i, j] j is a neighbour of i.  common [M, M] need not be symmetric"""
    f = fcc_of(common, n)
    rev = np.float64(cutoff_fcc) * np.float64(strictness)
    nb = (f >= np.float64(cutoff_fcc)) & (f.T >= rev)
    np.fill_diagonal(nb, False)
    return nb


def cluster(nb, min_size=4):
    """(labels int32 [M], centres, sizes int32 [K], ties): ties = the centre choices at which several alive poses had the
    largest deg"""
    M = nb.shape[0]
    alive = np.ones(M, dtype=bool)
    labels = np.full(M, -1, dtype=np.int32)
    centres, sizes, ties = [], [], 0
    while alive.any():
        deg = np.where(alive, (nb & alive[None, :]).sum(axis=1), -1)
        c = int(np.argmax(deg))                                        # the first of the largest: the smallest index
        if deg[c] < min_size - 1:
            break
        ties += int((deg == deg[c]).sum() > 1)
        members = nb[c] & alive
        members[c] = True
        labels[members] = len(centres)
        centres.append(c)
        sizes.append(int(members.sum()))
        alive &= ~members
    return labels, np.array(centres, dtype=np.int32), np.array(sizes, dtype=np.int32), ties


def rank(labels, n_clusters, scores, top=4, ascending=False):
    """(order, means): clusters by the mean of their `top` best scores, best first, ties by ordinal"""
    best = [sorted(scores[labels == k], reverse=not ascending)[:top] for k in range(n_clusters)]
    means = np.array([np.mean(b) for b in best], dtype=np.float64).reshape(-1)
    order = sorted(range(n_clusters), key=lambda k: (means[k] if ascending else -means[k], k))
    return np.array(order, dtype=np.int64), means
