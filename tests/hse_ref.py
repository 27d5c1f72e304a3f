"""The half-sphere-exposure rule in numpy float64: the plain statement that drgnn_hse.h is held to (tests/test_hse.py,
tests/test_gpu_hse.py).  It restates what the reference's `hse` node feature records, Biopython's HSExposureCA(model)
with radius 12 A and offset 0 as (up, down, angle), and HSExposureCB for direction="CB".

Atoms are taken by name: X(r) is the first atom of residue r named X.  The per-residue table `bb` int32 [R,5] holds the
offsets of N, CA, C, CB inside the residue (-1: absent) and flags: bit 0 a standard amino acid, bit 1 GLY, bit 2 the
first residue of its chain (never linked to the residue before it).

1. Links.  Residues r, r+1 of one chain are linked iff both are standard amino acids, both have a CA, atom a of r and
   atom b of r+1 exist and |b(r+1) - a(r)| < cutoff: connect "CA" is (CA, CA, 4.3), connect "CN" is (C, N, 1.8).
2. Members: the residues with a link on at least one side.  Only members are counted; the others are invisible.
3. direction "CA": r has a value iff it is linked on both sides.  With c1, c2, c3 = CA(r-1), CA(r), CA(r+1):
   b = unit(unit(c2 - c1) + unit(c2 - c3)); the zero sum stays the zero vector.
   direction "CB": every member with a direction has a value; b = CB - CA, or for a GLY with N and C the rotated N (6).
4. Counts.  For every member o != r (with offset k > 0 also not one of the same peptide at most k positions away):
   d = CA(o) - c2; if |d|^2 < radius^2: up += 1 when d.b > 0, else down += 1 (d.b = 0, d = 0, b = 0: down).
5. Angle (direction "CA"; 0.0 for "CB"): between CB - c2 and b when r has a CB; else for a GLY with N and C between
   Rot(-120 degrees, axis C - c2)(N - c2) and b (the right-handed rotation about the unit axis); otherwise 0.0.
   angle(u, v) = acos(clip(u.v / (|u||v|), -1, 1)): NaN when b is the zero vector.
6. Residues without a value: a NaN row.

Every residue with a value also gets its margin (A): the smallest of ||d| - radius| over the members it looks at, |d.b|
(b of unit length) over those it counts, and |link distance - cutoff| of the candidate links on its two sides.  The
smallest margin over an input says how far that input is from a tie that rounding could decide.

direction "CB" has no recorded values anywhere: it is held to this statement alone."""
import numpy as np

CONNECT = {"CA": (1, 1, 4.3), "CN": (2, 0, 1.8)}
STANDARD = ("CYS", "HIS", "ASN", "GLN", "SER", "THR", "TYR", "TRP", "ALA", "PHE",
            "GLY", "ILE", "VAL", "MET", "PRO", "LEU", "GLU", "ASP", "LYS", "ARG")
COS_M120, SIN_M120 = -0.5, -0.8660254037844386


def table_of(res_name, res_chain, atom_ptr, atom_name):
    """bb int32 [R,5] from the residues' names and chains [R] and the atoms' names [T]"""
    R = len(atom_ptr) - 1
    bb = np.full((R, 5), -1, dtype=np.int32)
    for r in range(R):
        names = [str(n) for n in atom_name[atom_ptr[r]:atom_ptr[r + 1]]]
        for c, want in enumerate(("N", "CA", "C", "CB")):
            if want in names:
                bb[r, c] = names.index(want)
        bb[r, 4] = ((1 if str(res_name[r]) in STANDARD else 0) | (2 if str(res_name[r]) == "GLY" else 0) |
                    (4 if r == 0 or res_chain[r] != res_chain[r - 1] else 0))
    return bb


def unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt((v * v).sum())


def angle(u, v):
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (u * v).sum() / (np.sqrt((u * u).sum()) * np.sqrt((v * v).sum()))
    return float(np.arccos(np.clip(c, -1.0, 1.0)))


def rotated_n(n, ca, c):
    """Rot(-120 degrees, axis c - ca) applied to n - ca"""
    k, v = unit(c - ca), n - ca
    return v * COS_M120 + np.cross(k, v) * SIN_M120 + k * ((k * v).sum() * (1.0 - COS_M120))


def residue_hse(xyz, atom_ptr, bb, radius=12.0, offset=0, connect="CA", direction="CA"):
    """(hse float64 [R,3] up, down, angle with NaN rows for no value; margin float64 [R], inf where nothing is near)"""
    xyz = np.asarray(xyz, dtype=np.float64)
    atom_ptr = np.asarray(atom_ptr, dtype=np.int64)
    bb = np.asarray(bb, dtype=np.int64)
    col_a, col_b, cutoff = CONNECT[connect]
    assert direction in ("CA", "CB")
    R = len(atom_ptr) - 1

    def atom(r, c):
        return xyz[atom_ptr[r] + bb[r, c]] if bb[r, c] >= 0 else None

    ok = [(bb[r, 4] & 1) != 0 and bb[r, 1] >= 0 for r in range(R)]
    link = np.zeros(R, dtype=bool)                  # link[r]: r and r + 1
    link_margin = np.full(R, np.inf)
    for r in range(R - 1):
        if ok[r] and ok[r + 1] and not (bb[r + 1, 4] & 4) and bb[r, col_a] >= 0 and bb[r + 1, col_b] >= 0:
            d = atom(r + 1, col_b) - atom(r, col_a)
            d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            link[r] = d2 < cutoff * cutoff
            link_margin[r] = abs(np.sqrt(d2) - cutoff)
    before = np.concatenate(([False], link[:-1]))   # before[r]: r - 1 and r
    member = link | before
    out = np.full((R, 3), np.nan)
    margin = np.full(R, np.inf)
    mem = np.flatnonzero(member)
    ca = np.array([atom(r, 1) for r in mem]).reshape(-1, 3)
    for r in mem:
        c2 = atom(r, 1)
        if direction == "CA":
            if not (link[r] and before[r]):
                continue
            s = unit(c2 - atom(r - 1, 1)) + unit(c2 - atom(r + 1, 1))
            b = unit(s) if (s != 0.0).any() else s
        else:
            if bb[r, 3] >= 0:
                b = atom(r, 3) - c2
            elif (bb[r, 4] & 2) and bb[r, 0] >= 0 and bb[r, 2] >= 0:
                b = rotated_n(atom(r, 0), c2, atom(r, 2))
            else:
                continue
        lo = hi = r                                 # the stretch of r's peptide within `offset` positions of r
        while r - lo < offset and lo > 0 and link[lo - 1]:
            lo -= 1
        while hi - r < offset and link[hi]:
            hi += 1
        seen = (mem < lo) | (mem > hi)
        d = ca[seen] - c2
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        dot = d[:, 0] * b[0] + d[:, 1] * b[1] + d[:, 2] * b[2]
        inside = d2 < radius * radius
        with np.errstate(invalid="ignore"):
            up = inside & (dot > 0.0)
        out[r, 0], out[r, 1] = up.sum(), inside.sum() - up.sum()
        if direction == "CB":
            out[r, 2] = 0.0
        elif bb[r, 3] >= 0:
            out[r, 2] = angle(atom(r, 3) - c2, b)
        elif (bb[r, 4] & 2) and bb[r, 0] >= 0 and bb[r, 2] >= 0:
            out[r, 2] = angle(rotated_n(atom(r, 0), c2, atom(r, 2)), b)
        else:
            out[r, 2] = 0.0
        m = min(link_margin[r], link_margin[r - 1] if r > 0 else np.inf)
        if d2.size:
            m = min(m, np.abs(np.sqrt(d2) - radius).min())
        if inside.any():
            with np.errstate(invalid="ignore", divide="ignore"):
                m = min(m, np.nan_to_num(np.abs(dot[inside]) / np.sqrt((b * b).sum()), nan=0.0).min())
        margin[r] = m
    return out, margin
