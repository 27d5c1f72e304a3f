"""The rule of the pose-by-pose RMSD matrix and of RMSD clustering (HADDOCK's cluster_struc, ClusPro) as plain numpy
float64: what deeprank_gnn_amd.interface.pose_rmsd / cluster_poses_rmsd (csrc/drgnn_rmsd.h) are held to.

  distance   poses xyz float32 [M, T, 3] taken to float64, an index list rms (nR >= 1) and an index list fit (nF >= 3)
             or None.  Without fit: D[i, j] = sqrt(sum_a |p_i[a] - p_j[a]|^2 / nR) over rms, from coordinate
             differences.  With fit: the optimal PROPER rotation and translation of pose i's fit atoms onto pose j's,
             applied to pose i, then the same sum over rms.  D[i, i] = 0; the inverse transform is the optimum of the
             reversed pair, so i < j is computed and mirrored.  A collinear or coincident fit set leaves the rotation
             undetermined: the result is then undefined.
             The rule is stated twice.  (a) `kabsch`: SVD of the 3 x 3 covariance with the determinant correction, the
             residual from the transformed coordinates: the reference.  (b) `moments`: both poses centred about their
             fit centroid, the largest eigenvalue's eigenvector of Horn's 4 x 4 matrix (LAPACK), then
             A_i + A_j - 2 sum R o C over the rms moments: the form the kernels use.  The gap between the two is what
             the tolerance of tests/rmsd_cases.py is derived from.
  neighbour  j of i iff i != j and D[i, j] <= cutoff, in float64 on the stored value
  greedy     exactly fcc_ref.cluster: the centre is the alive pose with the most alive neighbours, the smallest index on
             a tie; stop below min_size - 1 neighbours; the centre and its alive neighbours die."""
import numpy as np

from fcc_ref import cluster  # noqa: F401  (the greedy rule, shared)


def _sets(xyz, rms, fit):
    x = np.asarray(xyz)
    assert x.dtype == np.float32 and x.ndim == 3
    x = x.astype(np.float64)
    return x, np.asarray(rms, dtype=np.int64), None if fit is None else np.asarray(fit, dtype=np.int64)


def plain_sq(p, q):
    """sum |p - q|^2 of two [n, 3] sets, from coordinate differences"""
    d = p - q
    return float((d * d).sum())


def kabsch_sq(pf, qf, pr, qr):
    """(a): sum over the rms atoms of |R (pr - cp) + cq - qr|^2 with the optimal proper rotation of pf onto qf"""
    cp, cq = pf.mean(axis=0), qf.mean(axis=0)
    H = (pf - cp).T @ (qf - cq)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    moved = (pr - cp) @ R.T + cq
    return plain_sq(moved, qr)


def horn_matrix(S):
    return np.array([
        [S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
        [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
        [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
        [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])


def moments_sq(pf, qf, pr, qr):
    """(b): (sum over rms of |.|^2 by the moment form, A_i + A_j): both about the fit centroids"""
    cp, cq = pf.mean(axis=0), qf.mean(axis=0)
    S = (pf - cp).T @ (qf - cq)
    w, v = np.linalg.eigh(horn_matrix(S))
    q0, qx, qy, qz = v[:, np.argmax(w)]
    R = np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                  [2 * (qx * qy + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                  [2 * (qx * qz - q0 * qy), 2 * (qy * qz + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]])
    a, b = pr - cp, qr - cq
    C = a.T @ b
    A = float((a * a).sum() + (b * b).sum())
    return A - 2.0 * float((R.T * C).sum()), A


def matrix_sq(xyz, rms, fit=None, other=None, form="kabsch"):
    """(sum of squares float64 [M, M'], scale float64 [M, M']): D^2 nR by form (a) "kabsch" or (b) "moments", and A_i + A_j
    (the rms atoms' sum |x|^2 about the fit centroids; without fit: the sum of squares itself).  Square: i < j computed
    and mirrored, the diagonal 0."""
    x, rms, fit = _sets(xyz, rms, fit)
    y = x if other is None else _sets(other, rms, fit)[0]
    out, scale = np.zeros((len(x), len(y))), np.zeros((len(x), len(y)))
    for i in range(len(x)):
        for j in range(len(y)):
            if other is None and j <= i:
                continue
            if fit is None:
                out[i, j] = scale[i, j] = plain_sq(x[i][rms], y[j][rms])
            else:
                m, A = moments_sq(x[i][fit], y[j][fit], x[i][rms], y[j][rms])
                out[i, j] = m if form == "moments" else kabsch_sq(x[i][fit], y[j][fit], x[i][rms], y[j][rms])
                scale[i, j] = A
    if other is None:
        out, scale = out + out.T, scale + scale.T
    return out, scale


def matrix(xyz, rms, fit=None, other=None, form="kabsch"):
    """D float64 [M, M']"""
    sq = matrix_sq(xyz, rms, fit, other, form)[0]
    return np.sqrt(np.maximum(sq, 0.0) / len(np.asarray(rms)))


def neighbours_of(d, cutoff):
    """bool [M, M]: [i, j] j is a neighbour of i.  d need not be symmetric"""
    d = np.asarray(d, dtype=np.float64)
    nb = d <= np.float64(cutoff)
    np.fill_diagonal(nb, False)
    return nb


def cluster_dist(d, cutoff=7.5, min_size=4):
    """(labels, centres, sizes, ties) of fcc_ref.cluster on the relation of d"""
    return cluster(neighbours_of(d, cutoff), min_size)


# ---- selections ------------------------------------------------------------------------------------------------------
BACKBONE = ("CA", "C", "N", "O")


def select(atom_name, res_chain, atom_ptr, names=BACKBONE, chain=None, residues=None):
    """indices (grouped atom order) of the atoms named in `names` (None: all), of `chain` (None: both), of `residues`"""
    res_of = np.repeat(np.arange(len(atom_ptr) - 1), np.diff(atom_ptr))
    keep = np.ones(len(res_of), dtype=bool)
    if names is not None:
        keep &= np.array([str(n) in names for n in atom_name], dtype=bool)
    if chain is not None:
        keep &= np.asarray(res_chain)[res_of] == chain
    if residues is not None:
        keep &= np.isin(res_of, np.asarray(residues))
    return np.flatnonzero(keep)


def kind_lists(kind, atom_name, res_chain, atom_ptr, residues=None):
    """(rms, fit or None) of the shorthand kinds"""
    n0 = int((np.asarray(res_chain) == 0).sum())
    long_chain = 0 if n0 >= len(res_chain) - n0 else 1
    sel = lambda **k: select(atom_name, res_chain, atom_ptr, **k)
    if kind == "ligand":
        return sel(chain=1 - long_chain), sel(chain=long_chain)
    if kind == "fixed":
        return sel(chain=1 - long_chain), None
    if kind == "interface":
        return sel(residues=residues), sel(residues=residues)
    assert kind == "all"
    return sel(), sel()
