"""The per-residue features on the device: buried surface area (csrc/drgnn_bsa.h), half-sphere exposure
(csrc/drgnn_hse.h) and residue depth (csrc/drgnn_depth.h); one record each and one path for all three."""
import collections

import numpy as np
import torch

from . import _lib
from ._request import Request
from .atoms import AtomTable, Poses, _complexes, _default_device, _ragged


# ---- the part of a request bsa, hse and depth share ------------------------------------------------------------------
def _residue_request(record, device, xyz, atom_ptr, res_ptr, res_split, target_res, target_complex, row):
    """(Request, out, status) of one drgnn_bsa_residues / drgnn_hse_residues / drgnn_depth_residues call with what their
    records have in common filled in: xyz, the offset tables (``res_split`` None: the record has none), the two target
    tables, the counts of atoms, residues, complexes and targets, ``out`` float64 [K] + ``row`` and the status word"""
    r = Request(record, device)
    d_xyz = r.input("xyz", np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3), torch.float32)
    n_residues, n_complexes = len(r.table("atom_ptr", atom_ptr)[0]) - 1, len(r.table("res_ptr", res_ptr)[0]) - 1
    if res_split is not None:
        r.table("res_split", res_split)
    K = len(r.table("target_res", target_res)[0])
    r.table("target_complex", target_complex)
    r.set(n_atoms=int(d_xyz.shape[0]), n_residues=n_residues, n_complexes=n_complexes, n_targets=K)
    return r, r.output("out", (K,) + row, torch.float64), r.output("status", 1, torch.int32, zeros=True)


def _residue_result(out, status, keep_device):
    """(out, or its rows on the host; the status word) as the three raw calls return them"""
    return (out if keep_device else out.cpu().numpy()), int(status.cpu()[0])


# ---- buried surface area (csrc/drgnn_bsa.h) ----------------------------------------------------------------------------
# ProtOr radii of the heavy atoms (the classifier freesasa applies to a PDB file): backbone, then the side chains
BSA_BACKBONE = {"N": 1.64, "CA": 1.88, "C": 1.61, "O": 1.42, "OXT": 1.46}
_C, _N, _O1, _O2, _S, _CT, _CR = 1.88, 1.64, 1.42, 1.46, 1.77, 1.61, 1.76          # _CT trigonal, _CR aromatic CH carbon
BSA_SIDE_CHAIN = {
    "ALA": {"CB": _C},
    "ARG": {"CB": _C, "CG": _C, "CD": _C, "NE": _N, "CZ": _CT, "NH1": _N, "NH2": _N},
    "ASN": {"CB": _C, "CG": _CT, "OD1": _O1, "ND2": _N},
    "ASP": {"CB": _C, "CG": _CT, "OD1": _O1, "OD2": _O2},
    "CYS": {"CB": _C, "SG": _S},
    "GLN": {"CB": _C, "CG": _C, "CD": _CT, "OE1": _O1, "NE2": _N},
    "GLU": {"CB": _C, "CG": _C, "CD": _CT, "OE1": _O1, "OE2": _O2},
    "GLY": {},
    "HIS": {"CB": _C, "CG": _CT, "ND1": _N, "CD2": _CR, "CE1": _CR, "NE2": _N},
    "ILE": {"CB": _C, "CG1": _C, "CG2": _C, "CD1": _C},
    "LEU": {"CB": _C, "CG": _C, "CD1": _C, "CD2": _C},
    "LYS": {"CB": _C, "CG": _C, "CD": _C, "CE": _C, "NZ": _N},
    "MET": {"CB": _C, "CG": _C, "SD": _S, "CE": _C},
    "PHE": {"CB": _C, "CG": _CT, "CD1": _CR, "CD2": _CR, "CE1": _CR, "CE2": _CR, "CZ": _CR},
    "PRO": {"CB": _C, "CG": _C, "CD": _C},
    "SER": {"CB": _C, "OG": _O2},
    "THR": {"CB": _C, "OG1": _O2, "CG2": _C},
    "TRP": {"CB": _C, "CG": _CT, "CD1": _CR, "CD2": _CT, "NE1": _N, "CE2": _CT, "CE3": _CR, "CZ2": _CR, "CZ3": _CR, "CH2": _CR},
    "TYR": {"CB": _C, "CG": _CT, "CD1": _CR, "CD2": _CR, "CE1": _CR, "CE2": _CR, "CZ": _CT, "OH": _O2},
    "VAL": {"CB": _C, "CG1": _C, "CG2": _C},
}
# the unbound chains of the reference: it hands freesasa only the first character of the atom name
BSA_FIRST_LETTER = {"C": 1.61, "N": 1.64, "O": 1.42, "S": 1.80, "H": 1.10}
RESIDUE_XYZ_BUDGET = 256 << 20     # bytes of coordinates one bsa / hse / depth call uploads (sets their default chunk)
BSA_XYZ_BUDGET = RESIDUE_XYZ_BUDGET                                    # (its first name)


def bsa_radii(table, radii="reference"):
    """(complex_r, unbound_r) float64 [T] in the table's grouped atom order; 0: the atom is absent from that state.

    "reference": what the reference's ``bsa`` feature uses.  Complex: heavy atoms only (the name does not start with
    H) with ProtOr radii by (residue, atom name); a heavy atom outside the table or a non-standard residue raises
    ValueError.  Unbound: every atom, hydrogens included, the radius from the first character of its name (C 1.61, N
    1.64, O 1.42, S 1.80, H 1.10; any other raises ValueError).  "protor": the complex radii for both states.
    A pair ``(complex_r, unbound_r)`` of arrays [n_input_atoms] in input atom order is taken as it is."""
    if isinstance(radii, str):
        if radii not in ("reference", "protor"):
            raise ValueError("radii must be 'reference', 'protor' or a pair of arrays, not %r" % radii)
        if table.atom_name is None:
            raise ValueError("the radius tables go by atom name: build the AtomTable with atom_name=")
        bad = np.flatnonzero(table.res_type < 0)
        if bad.size:
            r = int(bad[0])
            raise ValueError("no radii for the non-standard residue %s %s%d" % (table.res_name[r], table.chains[table.res_chain[r]],
                                                                               table.res_seq[r]))
        res_of_atom = np.repeat(np.arange(table.n_residues), np.diff(table.atom_ptr))
        cr = np.zeros(table.n_atoms)
        ur = np.zeros(table.n_atoms)
        for i, nm in enumerate(table.atom_name):
            nm = str(nm)
            if radii == "reference":
                if nm[:1] not in BSA_FIRST_LETTER:
                    raise ValueError("no radius for an atom whose name starts with %r (%s)" % (nm[:1], nm))
                ur[i] = BSA_FIRST_LETTER[nm[0]]
            if not nm.startswith("H"):
                res = str(table.res_name[res_of_atom[i]])
                rad = BSA_BACKBONE.get(nm, BSA_SIDE_CHAIN[res].get(nm))
                if rad is None:
                    raise ValueError("no ProtOr radius for the heavy atom %s of %s" % (nm, res))
                cr[i] = rad
        return (cr, cr.copy()) if radii == "protor" else (cr, ur)
    try:
        cr, ur = radii
    except (TypeError, ValueError):
        raise ValueError("radii must be 'reference', 'protor' or a pair (complex_r, unbound_r)")
    out = []
    for a in (cr, ur):
        a = np.asarray(a, dtype=np.float64)
        if a.shape != (table.n_input_atoms,):
            raise ValueError("radius arrays need %d entries, one per input atom" % table.n_input_atoms)
        if not np.all(a >= 0.0):                                       # (NaN fails too)
            raise ValueError("radii must be >= 0 (0: the atom is absent)")
        out.append(a[table.order])
    return tuple(out)


def bsa_raw(api, xyz, atom_ptr, res_ptr, res_split, rad_complex, rad_unbound, target_res, target_complex, probe=1.4,
            n_slices=20, device="cpu", keep_device=False):
    """One drgnn_bsa_residues call (include/drgnn.h) over numpy arrays.  Returns (out float64 [K,3]: sasa_unbound,
    sasa_complex, bsa; status int): bit 0 of status says a list overflowed (those residues are NaN).  ``keep_device``:
    ``out`` stays a tensor on ``device``; only the status word comes back."""
    rad = [np.ascontiguousarray(a, dtype=np.float32) for a in (rad_complex, rad_unbound)]
    if rad[0].shape != rad[1].shape or rad[0].ndim != 1 or np.shape(target_res) != np.shape(target_complex):
        raise ValueError("the two radius arrays, and the two target arrays, must have one length each")
    r, out, status = _residue_request(_lib.BsaRequest, device, xyz, atom_ptr, res_ptr, res_split, target_res, target_complex, (3,))
    r.input("rad_complex", rad[0], torch.float32)
    r.input("rad_unbound", rad[1], torch.float32)
    r.set(n_radii=int(rad[0].shape[0]), probe=float(probe), n_slices=int(n_slices))
    r.run(api, "bsa_residues")
    return _residue_result(out, status, keep_device)


def _bsa_options(probe=1.4, n_slices=20):
    if int(n_slices) < 1:
        raise ValueError("n_slices must be at least 1")
    if not float(probe) >= 0.0:
        raise ValueError("probe must be >= 0")
    return {"probe": probe, "n_slices": n_slices}


def residue_bsa(tables_or_poses, residues=None, radii="reference", probe=1.4, n_slices=20, device=None, chunk=None, api=None,
                parts=False):
    """Buried surface area (A^2) of residues, on the device: SASA of the residue in its chain alone minus its SASA in
    the complex, each by the Lee-Richards slice method (``probe`` 1.4 A, ``n_slices`` 20: what the reference's ``bsa``
    node feature records, negative values included; see ``bsa_radii`` for ``radii``).

    An ``AtomTable`` gives float64 [R], an ``AtomTable.poses`` batch [M, R], a sequence of either a list of [R_k], with
    NaN for the residues not asked for.  ``residues``: None (all), an index array applied to every complex, or one
    index array per complex.  Only the atoms of the residues asked for are evaluated.  ``chunk``: complexes per
    launch; a residue's bits do not depend on it, on the batch or on ``residues``.  ``parts``: return (bsa,
    sasa_unbound, sasa_complex) instead.  More than 256 neighbours of one atom is refused (DrgnnError, capacity)."""
    rows = _residue_values(BSA, tables_or_poses, residues, radii, {"probe": probe, "n_slices": n_slices}, device, chunk, api)

    def pick(a):                                                       # the columns of a row: sasa_unbound, sasa_complex, bsa
        got = tuple(np.ascontiguousarray(a[..., j]) for j in ((2, 0, 1) if parts else (2,)))
        return got if parts else got[0]
    return [pick(a) for a in rows] if isinstance(rows, list) else pick(rows)


# ---- half-sphere exposure (csrc/drgnn_hse.h) ---------------------------------------------------------------------------
HSE_CONNECT = {"CA": (1, 1, 4.3), "CN": (2, 0, 1.8)}      # (column of bb in r, column in r + 1, cutoff in A)
HSE_DIRECTION = {"CA": 0, "CB": 1}
HSE_BACKBONE = ("N", "CA", "C", "CB")                     # the columns of the bb table
HSE_TILE = (4, 64)                                        # targets per workgroup: the fewest and the most
HSE_WORKGROUPS = 512                                      # a call aims at this many workgroups (two per compute unit)


def hse_table(table):
    """bb int32 [R,5] of an ``AtomTable`` made with ``atom_name``: the offsets of the first atoms named N, CA, C, CB
    inside every residue (-1: absent) and flags: bit 0 one of the 20 standard residue names, bit 1 GLY, bit 2 the first
    residue of its chain."""
    if table.atom_name is None:
        raise ValueError("hse finds the backbone by atom name: build the AtomTable with atom_name=")
    R = table.n_residues
    bb = np.full((R, 5), -1, dtype=np.int32)
    res_of_atom = np.repeat(np.arange(R), np.diff(table.atom_ptr))
    inside = np.arange(table.n_atoms) - table.atom_ptr[:-1][res_of_atom]
    for col, name in enumerate(HSE_BACKBONE):
        hit = np.flatnonzero(table.atom_name == name)[::-1]                # reversed: the first atom of a name wins
        bb[res_of_atom[hit], col] = inside[hit]
    start = np.ones(R, dtype=bool)
    start[1:] = table.res_chain[1:] != table.res_chain[:-1]
    bb[:, 4] = (table.res_type >= 0) * 1 + (table.res_name == "GLY") * 2 + start * 4
    return bb


def hse_tile(n_targets):
    """targets per workgroup for a call of ``n_targets``: small calls spread over many workgroups (1 pose of 1ATN, all
    residues: 8.0 us at 4 against 32.1 us at 64), large ones stage a complex fewer times (1024 poses: 2.46 ms at 64 against
    3.57 ms at 4); profiles/hse_ab.txt.  It changes no bit of the result."""
    return max(HSE_TILE[0], min(HSE_TILE[1], int(n_targets) // HSE_WORKGROUPS))


def _hse_options(radius=12.0, offset=0, connect="CA", direction="CA"):
    if connect not in HSE_CONNECT:
        raise ValueError("connect must be 'CA' or 'CN', not %r" % (connect,))
    if direction not in HSE_DIRECTION:
        raise ValueError("direction must be 'CA' or 'CB', not %r" % (direction,))
    if not float(radius) > 0.0:
        raise ValueError("radius must be > 0")
    if int(offset) != offset or int(offset) < 0:
        raise ValueError("offset must be an integer >= 0")
    return {"radius": float(radius), "offset": int(offset), "connect": connect, "direction": direction}


def hse_raw(api, xyz, atom_ptr, res_ptr, bb, target_res, target_complex, radius=12.0, offset=0, connect="CA",
            direction="CA", device="cpu", tile=None, keep_device=False):
    """One drgnn_hse_residues call (include/drgnn.h) over numpy arrays; the targets in any order (they are grouped by
    complex and cut into tiles of ``tile``, default ``hse_tile``, here, and the rows come back in the order asked for).
    ``connect``: "CA", "CN" or (column, column, cutoff).  Returns (out float64 [K,3]: up, down, angle, NaN rows for no value; status int): bit 0
    of status says a complex was beyond the capacity (its rows are NaN).  ``keep_device``: ``out`` stays a tensor on
    ``device``; only the status word comes back."""
    con = HSE_CONNECT[connect] if isinstance(connect, str) else connect
    tgt_res = np.asarray(target_res, dtype=np.int64).reshape(-1)
    tgt_cx = np.asarray(target_complex, dtype=np.int64).reshape(-1)
    if tgt_res.shape != tgt_cx.shape:
        raise ValueError("the two target arrays must have one length")
    K = int(tgt_res.shape[0])
    tile = max(1, int(tile or hse_tile(K)))
    order = np.argsort(tgt_cx, kind="stable")
    sorted_cx = tgt_cx[order]
    first = np.flatnonzero(np.concatenate(([True], sorted_cx[1:] != sorted_cx[:-1]))) if K else np.zeros(0, np.int64)
    ends = np.append(first[1:], K)
    cuts = [np.arange(lo, hi, tile) for lo, hi in zip(first, ends)]
    tile_ptr = np.concatenate(cuts + [np.array([K])])
    r, out, status = _residue_request(_lib.HseRequest, device, xyz, atom_ptr, res_ptr, None, tgt_res[order], sorted_cx, (3,))
    bb = r.table("bb", bb, shape=(-1, 5))[0]
    r.table("tile_ptr", tile_ptr)
    r.set(n_tiles=len(tile_ptr) - 1, n_rows=int(bb.shape[0]), radius=float(radius), offset=int(offset),
          direction=HSE_DIRECTION.get(direction, direction), connect_a=int(con[0]), connect_b=int(con[1]),
          connect_cutoff=float(con[2]))
    r.run(api, "hse_residues")
    if keep_device:
        if not np.array_equal(order, np.arange(K)):                        # (targets listed complex by complex: as they are)
            rows = torch.empty_like(out)
            rows[torch.from_numpy(order).to(r.device)] = out
            out = rows
        return _residue_result(out, status, True)
    sorted_rows, status = _residue_result(out, status, False)
    rows = np.empty((K, 3))
    rows[order] = sorted_rows
    return rows, status


def residue_hse(tables_or_poses, residues=None, radius=12.0, offset=0, connect="CA", direction="CA", device=None, chunk=None,
                api=None):
    """Half-sphere exposure of residues, on the device: (up, down, angle) as the reference's ``hse`` node feature
    records it from Biopython's ``HSExposureCA(model)`` (``radius`` 12 A, ``offset`` 0).  The CA trace is cut into
    peptides: consecutive standard residues of a chain are linked when their CAs are closer than 4.3 A (``connect``
    "CA", Biopython's CaPPBuilder) or the C of one and the N of the next closer than 1.8 A ("CN", its PPBuilder).  A
    residue linked on both sides has a value: ``up`` / ``down`` count the CAs of the other linked residues within
    ``radius`` on either side of the plane through its CA whose normal is the sum of the unit vectors from its two
    neighbours' CAs; ``angle`` (rad) lies between that normal and CA -> CB (a GLY: the N turned by -120 degrees about CA
    -> C).  ``offset`` k also leaves out the residues of the same peptide at most k positions away.
    ``direction`` "CB" is Biopython's ``HSExposureCB``: the normal is CA -> CB itself, every linked residue with that
    vector has a value and the angle is 0 (the reference records nothing for it: it is held to the written rule of
    tests/hse_ref.py alone).

    An ``AtomTable`` gives float64 [R,3], an ``AtomTable.poses`` batch [M,R,3], a sequence of either a list of [R_k,3];
    NaN rows mark residues without a value and residues not asked for.  ``residues``: None (all), an index array
    applied to every complex, or one index array per complex.  ``chunk``: complexes per launch; a residue's bits do
    not depend on it, on the batch or on ``residues``.  The tables must have been made with ``atom_name``.  A complex of
    more than 4096 residues is refused (DrgnnError, capacity)."""
    return _residue_values(HSE, tables_or_poses, residues, None,
                           {"radius": radius, "offset": offset, "connect": connect, "direction": direction}, device, chunk, api)


# ---- residue depth (csrc/drgnn_depth.h) --------------------------------------------------------------------------------
DEPTH_UNITED = {"C": 1.9, "N": 1.7, "O": 1.5, "S": 1.85, "H": 0.0}     # MSMS' united-atom radii by the first letter of the name
DEPTH_OTHER = 1.8                                                      # any other first letter
DEPTH_COMPONENTS = {"outer": 0, "all": 1}
# bytes of workspace one drgnn_depth_residues call may ask for (sets the complexes per call): k_depth_components gives a
# complex one workgroup, so a call on the device should hold about as many complexes as there are compute units (256;
# 1ATN at 192 dots: 41.7 MB each); the host emulation runs them one after the other
DEPTH_WORKSPACE_BUDGET = {"cpu": 1 << 30, "cuda": 13 << 30}


def depth_radii(table, radii="united"):
    """float64 [T] in the table's grouped atom order; 0: the atom takes no part in the surface.  "united": MSMS'
    united-atom radii by the first letter of the atom name (C 1.9, N 1.7, O 1.5, S 1.85, H 0, any other letter 1.8); a
    name without a letter raises ValueError.  An array [n_input_atoms] in input atom order is taken as
    it is."""
    if isinstance(radii, str):
        if radii != "united":
            raise ValueError("radii must be 'united' or an array, not %r" % radii)
        if table.atom_name is None:
            raise ValueError("the radius table goes by atom name: build the AtomTable with atom_name=")
        out = np.empty(table.n_atoms)
        for i, nm in enumerate(table.atom_name):
            letters = [ch for ch in str(nm) if ch.isalpha()]
            if not letters:
                raise ValueError("no radius for the atom name %r: it holds no letter" % str(nm))
            out[i] = DEPTH_UNITED.get(letters[0], DEPTH_OTHER)
        return out
    a = np.asarray(radii, dtype=np.float64)
    if a.shape != (table.n_input_atoms,):
        raise ValueError("the radius array needs %d entries, one per input atom" % table.n_input_atoms)
    if not np.all(a >= 0.0):                                           # (NaN fails too)
        raise ValueError("radii must be >= 0 (0: the atom takes no part in the surface)")
    return a[table.order]


def depth_dots(n_dots):
    """float64 [n_dots, 3]: the unit dots S_k = (rho cos phi, rho sin phi, z), z = 1 - (2k + 1) / n, rho = sqrt(1 - z^2),
    phi = (k + 1/2) pi (3 - sqrt 5), as tests/depth_ref.py writes them"""
    k = np.arange(int(n_dots), dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / int(n_dots)
    rho = np.sqrt(1.0 - z * z)
    phi = (k + 0.5) * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack((rho * np.cos(phi), rho * np.sin(phi), z), axis=1)


def depth_link(n_dots, probe=1.5):
    """the default link length: one and a half dot spacings on a sphere of radius 1.8 + probe"""
    return float(1.5 * np.sqrt(4.0 * np.pi * (DEPTH_OTHER + probe) ** 2 / int(n_dots)))


def _depth_options(probe=1.5, n_dots=192, link=None, components="outer"):
    if int(n_dots) != n_dots or int(n_dots) < 1:
        raise ValueError("n_dots must be an integer >= 1")
    if not float(probe) > 0.0 or not np.isfinite(float(probe)):
        raise ValueError("probe must be > 0")
    if components not in DEPTH_COMPONENTS:
        raise ValueError("components must be 'outer' or 'all', not %r" % (components,))
    link = depth_link(n_dots, float(probe)) if link is None else float(link)
    if not link >= 0.0 or not np.isfinite(link):
        raise ValueError("link must be >= 0")
    return {"probe": float(probe), "n_dots": int(n_dots), "link": link, "components": components}


def depth_raw(api, xyz, atom_ptr, res_ptr, radii, target_res, target_complex, probe=1.5, n_dots=192, link=None,
              components="outer", device="cpu", keep_device=False, parts=False):
    """One drgnn_depth_residues call (include/drgnn.h) over numpy arrays.  Returns (out float64 [K], status int): bit 0 of
    status says a complex was beyond the capacity (its targets are NaN).  ``keep_device``: ``out`` stays a tensor on
    ``device``.  ``parts``: a third value, the surface the call left in its workspace, per complex a dict of ``mask`` bool
    [atoms, n_dots], ``ids`` (dot ids atom n_dots + k of the accessible dots, atoms counted within the complex),
    ``label`` (the smallest dot id of each dot's component) and ``outer`` (the label kept; -1: all or none)."""
    link = depth_link(n_dots, probe) if link is None else float(link)
    if np.size(target_res) != np.size(target_complex):
        raise ValueError("the two target arrays must have one length")
    r, out, status = _residue_request(_lib.DepthRequest, device, xyz, atom_ptr, res_ptr, None, target_res, target_complex, ())
    T, M, K = r.q.n_atoms, r.q.n_complexes, r.q.n_targets
    rad = r.input("radii", np.ascontiguousarray(radii, dtype=np.float64).reshape(-1), torch.float64)
    r.input("dots", depth_dots(n_dots), torch.float64)
    n_bytes, off = api.depth_workspace(T, M, n_dots)
    work = r.output("workspace", max(1, n_bytes // 8), torch.int64)
    r.set(n_radii=int(rad.shape[0]), probe=float(probe), link=link, n_dots=int(n_dots),
          components=DEPTH_COMPONENTS.get(components, components), workspace_bytes=n_bytes)
    r.run(api, "depth_residues")
    result = _residue_result(out, status, keep_device)
    if not parts:
        return result
    w = work.cpu().numpy().view(np.uint8)
    W, D = (int(n_dots) + 63) // 64, T * int(n_dots)
    mask = w[off[0]:off[0] + 8 * T * W].view(np.uint64).reshape(T, W)
    bits = ((mask[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
    bits = bits.reshape(T, W * 64)[:, :int(n_dots)]
    ids, label = (w[off[j]:off[j] + 4 * D].view(np.int32) for j in (2, 3))
    cx_nd, cx_outer = (w[off[j]:off[j] + 4 * M].view(np.int32) for j in (7, 8))
    first = np.asarray(atom_ptr).reshape(-1)[np.asarray(res_ptr).reshape(-1)]      # the first atom of every complex
    surf = []
    for c in range(M):
        a0, a1, nd = int(first[c]), int(first[c + 1]), int(cx_nd[c])
        base = a0 * int(n_dots)
        if K == 0 or cx_outer[c] == -2:
            surf.append(None)
            continue
        cid = ids[base:base + nd].astype(np.int64)
        surf.append({"mask": bits[a0:a1].copy(), "ids": cid, "label": cid[label[base:base + nd]],
                     "outer": int(cid[cx_outer[c]]) if cx_outer[c] >= 0 else -1})
    return result + (surf,)


def _depth_too_large(api, part, residues, opt, device):
    """a call of these complexes is beyond the workspace budget or the grid"""
    atoms = sum(t.n_atoms for t, _ in part)
    budget = DEPTH_WORKSPACE_BUDGET["cuda" if torch.device(device).type == "cuda" else "cpu"]
    return (44 * atoms * opt["n_dots"] > budget or
            max(sum(len(r) for r in residues), len(part), atoms // 16 + 1) > api.depth_capacity(2))


def residue_depth(tables_or_poses, residues=None, radii="united", probe=1.5, n_dots=192, link=None, components="outer",
                  device=None, chunk=None, api=None):
    """Residue depth (A), on the device: the mean, over the atoms of a residue, of the distance to the molecular surface
    of the complex, as the reference's ``depth`` node feature records it from Biopython's ``residue_depth`` (MSMS).
    MSMS is not reproduced: the surface is a dot surface of the solvent-accessible surface of all atoms of both chains
    (``n_dots`` golden-spiral dots on every sphere of radius r + ``probe``; see ``depth_radii`` for ``radii``), restricted
    to its outer component (dots closer than ``link`` are linked, default one and a half dot spacings; the component with
    the most dots is kept, so that cavities do not count), and depth(atom) = distance to the nearest kept dot - ``probe``.
    ``components`` "all" keeps every accessible dot (for comparison).  tests/depth_ref.py states the rule; on the 496
    recorded 1ATN nodes it lies within 0.15 A rms of the reference's values (r = 0.990), one MSMS vertex spacing.  The
    dot lattice is fixed in the frame of the input: the value is not invariant under rotation, it varies within the dot
    spacing.

    An ``AtomTable`` gives float64 [R], an ``AtomTable.poses`` batch [M, R], a sequence of either a list of [R_k], with
    NaN for the residues not asked for.  ``residues``: None (all), an index array applied to every complex, or one
    index array per complex.  ``chunk``: complexes per call (the workspace also bounds it); a residue's bits do not
    depend on it, on the batch or on ``residues``.  The tables must have been made with ``atom_name``.  More than 4096
    dots per atom, or a complex of more than 4 194 304 atoms x n_dots, is refused (DrgnnError, capacity)."""
    return _residue_values(DEPTH, tables_or_poses, residues, radii,
                           {"probe": probe, "n_dots": n_dots, "link": link, "components": components}, device, chunk, api)


# ---- the per-residue features: one record each, one path for all ("Per-residue features") --------------------
# name: of the option, of node_data/<name> and of the node feature;  row: the shape of one row of the raw call's out
# check(**options): the options of the raw call, validated;  host_table(table, radii): the arrays the raw call takes per
# table, a tuple;  ragged: how many of (xyz, atom_ptr, res_ptr, res_split) the raw call takes;  raw: one call of the
# library;  too_large(api, part, residues, opt, device): the call must be halved;  c_name: the entry point, for errors
# options(value, tables): the graph paths' option (True, a dict, a radii value) as (opt, host tables by id(table))
# needs: what, besides True, the option may be;  node_data(rows): the rows of a complex as the store keeps them
# pack: the (source, column) pairs of drgnn_iface_pack, which takes the rows as the argument ``name``
Feature = collections.namedtuple("Feature", "name row check host_table ragged raw too_large c_name options needs node_data pack")


def _per_table(feature, tables, radii):
    """{id(table): host arrays}: each distinct table's, made once"""
    found = {}
    for t in tables:
        if id(t) not in found:
            found[id(t)] = feature.host_table(t, radii)
    return found


def _bsa_graph_options(value, tables):
    return {"probe": 1.4, "n_slices": 20}, _per_table(BSA, tables, "reference" if value is True else value)


def _hse_graph_options(value, tables):
    opt = _hse_options(**({} if value is True else dict(value)))
    return opt, _per_table(HSE, tables, None)


def _depth_graph_options(value, tables):
    opt = dict({} if value is True else value)
    tabs_of = _per_table(DEPTH, tables, opt.pop("radii", "united"))
    return _depth_options(**opt), tabs_of


def _hse_node_data(rows):
    rows = rows.copy()
    rows[np.isnan(rows[:, 0])] = 0.0
    return rows


BSA = Feature(name="bsa", row=(3,), check=_bsa_options, host_table=bsa_radii, ragged=4, raw=bsa_raw,
              # one workgroup per target: the grid's limit
              too_large=lambda api, part, residues, opt, device: sum(len(r) for r in residues) > api.bsa_capacity(3),
              c_name="drgnn_bsa_residues", options=_bsa_graph_options, needs="a radii option",
              node_data=lambda rows: rows[:, 2:3].copy(), pack=[(_lib.PACK_BSA, 2)])
HSE = Feature(name="hse", row=(3,), check=_hse_options, host_table=lambda table, radii: (hse_table(table),), ragged=3, raw=hse_raw,
              # one workgroup per tile
              too_large=lambda api, part, residues, opt, device: (sum(len(r) // HSE_TILE[0] + 1 for r in residues) >
                                                                  api.hse_capacity(1)),
              c_name="drgnn_hse_residues", options=_hse_graph_options, needs="a dict of options",
              node_data=_hse_node_data, pack=[(_lib.PACK_HSE, j) for j in range(3)])
DEPTH = Feature(name="depth", row=(), check=_depth_options, host_table=lambda table, radii: (depth_radii(table, radii),),
                ragged=3, raw=depth_raw, too_large=_depth_too_large,
                c_name="drgnn_depth_residues", options=_depth_graph_options, needs="a dict of options",
                node_data=lambda rows: rows.copy(), pack=[(_lib.PACK_DEPTH, 0)])
FEATURES = (BSA, HSE, DEPTH)                                           # in the order of the options of the graph paths


def _targets(residues, res_ptr):
    """(target_res, target_complex, sizes) of per-complex lists of local residue indices"""
    sizes = [len(r) for r in residues]
    tgt_res = np.concatenate([np.asarray(r, dtype=np.int64) + int(res_ptr[k]) for k, r in enumerate(residues)]
                             + [np.zeros(0, np.int64)])
    return tgt_res, np.repeat(np.arange(len(residues)), sizes), sizes


def _feature_chunk(feature, api, part, residues, tabs_of, opt, device, ragged=None, keep_device=False):
    """[rows float64 [K_c] + feature.row] for the complexes of ``part`` ([(table, xyz)]) and their residue lists (local
    indices); ``ragged``: ``_ragged(part)`` when the caller has it.  ``keep_device``: one tensor [sum K_c] + feature.row
    on ``device`` instead, the complexes' rows back to back."""
    if len(part) > 1 and feature.too_large(api, part, residues, opt, device):
        half = len(part) // 2
        both = [_feature_chunk(feature, api, part[h], residues[h], tabs_of, opt, device, keep_device=keep_device)
                for h in (slice(0, half), slice(half, None))]
        return torch.cat(both) if keep_device else both[0] + both[1]
    ragged = (ragged if ragged is not None else _ragged(part))[:feature.ragged]
    tables = [t for t, _ in part]
    if all(t is tables[0] for t in tables):                              # poses of one topology share one table
        tabs = tabs_of[id(tables[0])]
    else:
        tabs = [np.concatenate(arrays) for arrays in zip(*[tabs_of[id(t)] for t in tables])]
    tgt_res, tgt_cx, sizes = _targets(residues, ragged[2])
    out, status = feature.raw(api, *ragged, *tabs, tgt_res, tgt_cx, device=device, keep_device=keep_device, **opt)
    if status & 1:
        _lib._check(-2, feature.c_name)
    if keep_device:
        return out
    ends = np.cumsum(sizes)
    return [out[e - n:e] for n, e in zip(sizes, ends)]


def _residue_values(feature, tables_or_poses, residues, radii, options, device, chunk, api):
    """``residue_bsa`` / ``residue_hse`` / ``residue_depth``: the raw rows of the residues asked for, NaN elsewhere; an
    ``AtomTable`` gives float64 [R] + feature.row, an ``AtomTable.poses`` batch [M, R] + feature.row, a sequence a list"""
    api = api or _lib.get()
    device = _default_device(api, device)
    cx = _complexes(tables_or_poses)
    opt = feature.check(**options)
    tabs_of = _per_table(feature, [t for t, _ in cx], radii)
    if residues is None:
        wanted = [np.arange(t.n_residues) for t, _ in cx]
    else:
        per_complex = (isinstance(residues, (list, tuple)) and len(residues) == len(cx) and
                       all(np.ndim(r) == 1 for r in residues))
        wanted = [np.asarray(residues[k] if per_complex else residues, dtype=np.int64).reshape(-1) for k in range(len(cx))]
        for (t, _), w in zip(cx, wanted):
            if w.size and (w.min() < 0 or w.max() >= t.n_residues):
                raise ValueError("a residue index outside [0, %d)" % t.n_residues)
    if chunk is None:
        chunk = RESIDUE_XYZ_BUDGET // (12 * max([t.n_atoms for t, _ in cx] + [1]))
    chunk = max(1, int(chunk))
    full = [np.full((t.n_residues,) + feature.row, np.nan) for t, _ in cx]
    for lo in range(0, len(cx), chunk):
        part = cx[lo:lo + chunk]
        for k, o in enumerate(_feature_chunk(feature, api, part, wanted[lo:lo + chunk], tabs_of, opt, device)):
            full[lo + k][wanted[lo + k]] = o
    if isinstance(tables_or_poses, AtomTable):
        return full[0]
    if isinstance(tables_or_poses, Poses):
        return np.stack(full) if full else np.zeros((0, tables_or_poses.table.n_residues) + feature.row)
    return full
