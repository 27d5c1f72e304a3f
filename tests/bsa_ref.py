"""The buried-surface-area rule in numpy float64: the plain statement that drgnn_bsa.h is held to (tests/test_bsa.py,
tests/test_gpu_bsa.py), and the radius tables of the reference's `bsa` node feature written out.

    bsa(residue) = SASA_unbound(residue) - SASA_complex(residue)
Each SASA is the sum over the residue's atoms of a Lee-Richards area, probe 1.4 A, 20 slices.

Lee-Richards area of atom i among atoms with expanded radii R = r + probe: delta = 2 R_i / n_slices; slice k lies at
z = z_i - R_i + delta (k + 1/2); the atom's circle there has radius r_i' = sqrt(R_i^2 - (z - z_i)^2).  Every other atom
j with |z - z_j| < R_j has the circle r_j' = sqrt(R_j^2 - (z - z_j)^2) at the in-plane distance d:
    d >= r_i' + r_j'     no effect
    d + r_i' <= r_j'     the slice is buried: it contributes 0
    d + r_j' <= r_i'     no effect
    otherwise            j buries the arc [beta - alpha, beta + alpha], beta = atan2(dy, dx),
                         alpha = acos((r_i'^2 + d^2 - r_j'^2) / (2 r_i' d))
The slice contributes R_i delta (2 pi - the measure of the union of the arcs on the circle).

Radii.  Complex: heavy atoms only (the name does not start with H), ProtOr radii by (residue name, atom name).
Unbound: each chain alone, every atom, the radius from the first character of the atom name (the reference hands
freesasa '{:>2}'.format(atomName[0]) for the chains): this is why some recorded values are negative.
"""
import numpy as np

TWO_PI = 2.0 * np.pi
BACKBONE = {"N": 1.64, "CA": 1.88, "C": 1.61, "O": 1.42, "OXT": 1.46}
FIRST_LETTER = {"C": 1.61, "N": 1.64, "O": 1.42, "S": 1.80, "H": 1.10}
# the standard heavy side-chain atoms of the 20 residues
SIDE_CHAINS = {
    "ALA": "CB", "ARG": "CB CG CD NE CZ NH1 NH2", "ASN": "CB CG OD1 ND2", "ASP": "CB CG OD1 OD2", "CYS": "CB SG",
    "GLN": "CB CG CD OE1 NE2", "GLU": "CB CG CD OE1 OE2", "GLY": "", "HIS": "CB CG ND1 CD2 CE1 NE2",
    "ILE": "CB CG1 CG2 CD1", "LEU": "CB CG CD1 CD2", "LYS": "CB CG CD CE NZ", "MET": "CB CG SD CE",
    "PHE": "CB CG CD1 CD2 CE1 CE2 CZ", "PRO": "CB CG CD", "SER": "CB OG", "THR": "CB OG1 CG2",
    "TRP": "CB CG CD1 CD2 NE1 CE2 CE3 CZ2 CZ3 CH2", "TYR": "CB CG CD1 CD2 CE1 CE2 CZ OH", "VAL": "CB CG1 CG2"}
C_161 = {"ARG": "CZ", "ASN": "CG", "ASP": "CG", "GLN": "CD", "GLU": "CD", "HIS": "CG", "PHE": "CG", "TRP": "CG CD2 CE2",
         "TYR": "CG CZ"}
C_176 = {"HIS": "CD2 CE1", "PHE": "CD1 CD2 CE1 CE2 CZ", "TRP": "CD1 CE3 CZ2 CZ3 CH2", "TYR": "CD1 CD2 CE1 CE2"}
O_142 = {"ASN": "OD1", "GLN": "OE1", "ASP": "OD1", "GLU": "OE1"}


def protor_radius(res_name, atom_name):
    """ProtOr radius of a heavy atom; ValueError for anything outside the table"""
    if atom_name in BACKBONE:
        if res_name not in SIDE_CHAINS:
            raise ValueError("no ProtOr radius for %s %s" % (res_name, atom_name))
        return BACKBONE[atom_name]
    if atom_name not in SIDE_CHAINS.get(res_name, "").split():
        raise ValueError("no ProtOr radius for %s %s" % (res_name, atom_name))
    e = atom_name[0]
    if e == "N":
        return 1.64
    if e == "S":
        return 1.77
    if e == "O":
        return 1.42 if atom_name in O_142.get(res_name, "").split() else 1.46
    if atom_name in C_161.get(res_name, "").split():
        return 1.61
    if atom_name in C_176.get(res_name, "").split():
        return 1.76
    return 1.88


def radii_of(res_name, atom_name, mode="reference"):
    """(complex_r [T], unbound_r [T]) float64 for per-atom residue and atom names; 0: the atom is absent from the state"""
    heavy = np.array([not str(a).startswith("H") for a in atom_name])
    cr = np.array([protor_radius(str(r), str(a)) if h else 0.0 for r, a, h in zip(res_name, atom_name, heavy)])
    if mode == "protor":
        return cr, cr.copy()
    ur = []
    for a in atom_name:
        if str(a)[:1] not in FIRST_LETTER:
            raise ValueError("no radius for the first letter of atom %r" % str(a))
        ur.append(FIRST_LETTER[str(a)[0]])
    return cr, np.array(ur)


def atom_area(i, xyz, R, n_slices=20):
    """Lee-Richards area of atom i among the atoms xyz [n,3] with expanded radii R [n] (every atom takes part)"""
    Ri = R[i]
    d = xyz - xyz[i]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    near = np.flatnonzero(d2 < (Ri + R + 0.01) ** 2)
    near = near[near != i]
    delta = 2.0 * Ri / n_slices
    zo = -Ri + delta * (np.arange(n_slices) + 0.5)                      # slice planes relative to z_i
    ri2 = Ri * Ri - zo * zo
    ri = np.sqrt(ri2)
    if near.size == 0:
        return float(Ri * delta * TWO_PI * n_slices)
    dx, dy, dz, Rj = d[near, 0], d[near, 1], d[near, 2], R[near]
    h = zo[:, None] - dz[None, :]                                       # [S, n]
    rj2 = Rj[None, :] * Rj[None, :] - h * h
    cut = np.abs(h) < Rj[None, :]
    rj = np.sqrt(np.where(cut, rj2, 0.0))
    dp2 = (dx * dx + dy * dy)[None, :]
    dp = np.sqrt(dp2)
    rI, rI2 = ri[:, None], ri2[:, None]
    apart = dp >= rI + rj
    buried = cut & ~apart & (dp + rI <= rj)
    inside = dp + rj <= rI
    arc = cut & ~apart & ~buried & ~inside
    with np.errstate(invalid="ignore", divide="ignore"):
        cosa = (rI2 + dp2 - rj2) / (2.0 * rI * dp)
    alpha = np.arccos(np.clip(np.where(arc, cosa, 1.0), -1.0, 1.0))
    beta = np.broadcast_to(np.arctan2(dy, dx)[None, :], alpha.shape)
    lo = np.mod(beta - alpha, TWO_PI)
    hi = lo + 2.0 * alpha
    # intervals on [0, 2 pi): a wrapped arc is split in two; the absent ones sit at 2 pi with length 0
    s1 = np.where(arc, lo, TWO_PI)
    e1 = np.where(arc, np.minimum(hi, TWO_PI), TWO_PI)
    wraps = arc & (hi > TWO_PI)
    s2 = np.where(wraps, 0.0, TWO_PI)
    e2 = np.where(wraps, hi - TWO_PI, TWO_PI)
    s, e = np.concatenate((s1, s2), axis=1), np.concatenate((e1, e2), axis=1)
    order = np.argsort(s, axis=1, kind="stable")
    s, e = np.take_along_axis(s, order, axis=1), np.take_along_axis(e, order, axis=1)
    reach = np.maximum.accumulate(e, axis=1)
    before = np.concatenate((np.zeros((n_slices, 1)), reach[:, :-1]), axis=1)
    covered = np.maximum(0.0, e - np.maximum(s, before)).sum(axis=1)
    exposed = np.where(buried.any(axis=1), 0.0, TWO_PI - covered)
    return float(Ri * delta * exposed.sum())


def residue_bsa(xyz, atom_ptr, split, complex_r, unbound_r, residues, probe=1.4, n_slices=20):
    """(sasa_unbound, sasa_complex, bsa) float64 [len(residues)] of one complex: xyz [T,3], atoms sorted by residue,
    atom_ptr [R+1], the first `split` residues are chain A; the two radius arrays [T] (0: absent from the state)"""
    xyz = np.asarray(xyz, dtype=np.float64)
    atom_ptr = np.asarray(atom_ptr, dtype=np.int64)
    cut = int(atom_ptr[split])
    out = np.zeros((3, len(residues)))
    radii = (np.asarray(unbound_r, dtype=np.float64), np.asarray(complex_r, dtype=np.float64))
    for n, r in enumerate(residues):
        for state in (0, 1):
            rr = radii[state]
            part = np.flatnonzero(rr > 0.0)
            if state == 0:                                              # unbound: the residue's own chain
                part = part[part < cut] if r < split else part[part >= cut]
            R = rr[part] + probe
            x = xyz[part]
            total = 0.0
            for t in range(atom_ptr[r], atom_ptr[r + 1]):
                if rr[t] > 0.0:
                    total += atom_area(int(np.searchsorted(part, t)), x, R, n_slices)
            out[state, n] = total
    out[2] = out[0] - out[1]
    return out[0], out[1], out[2]
