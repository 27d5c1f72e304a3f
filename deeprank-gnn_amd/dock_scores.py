"""Docking scores of poses against a reference structure on the device (csrc/drgnn_score.h): irmsd, lrmsd, fnat, dockQ
and the two classes (Graph.get_score of the reference); and their lDDT and interface lDDT (csrc/drgnn_lddt.h)."""
import numpy as np
import torch

from . import _lib
from ._request import Request
from .atoms import BACKBONE, _default_device, _pose_batch

# ---- docking scores (csrc/drgnn_score.h) -------------------------------------------------------------------------------
SCORE_KEYS = ("irmsd", "lrmsd", "fnat", "dockQ", "binclass", "capri_class")
SCORE_XYZ_BUDGET = 256 << 20       # bytes of pose coordinates one call uploads (sets the default chunk)


def _residue_pairs(xyz_a, res_a, xyz_b, res_b, n_res_b, cutoff, rows=256):
    """sorted unique res_a * n_res_b + res_b over the atom pairs at d <= cutoff (float64), ``rows`` atoms of A at a
    time"""
    found = []
    for lo in range(0, xyz_a.shape[0], rows):
        d = xyz_a[lo:lo + rows, None, :] - xyz_b[None, :, :]
        i, j = np.nonzero(np.sqrt((d * d).sum(axis=2)) <= cutoff)
        found.append(np.unique(res_a[lo + i] * n_res_b + res_b[j]))
    return np.unique(np.concatenate(found)) if found else np.zeros(0, dtype=np.int64)


class ScoreReference(object):
    """The once-per-complex half of the scores, on the host: the reference structure's residue pairs (an atom pair at
    d <= ``fnat_cutoff``, all atoms) and interface zone (the residues of the pairs at d <= ``izone_cutoff``), the
    matching of the table's atoms to the reference's by (chain, res_seq, atom name), the long chain (more residues in
    the reference, the first chain on a tie) and the four tables ``drgnn_dock_scores`` takes (include/drgnn.h).

    ``ref_chain`` / ``ref_res_seq`` / ``ref_atom_name`` [N] and ``ref_xyz`` [N,3]: the reference's atoms in any order;
    it may hold other atoms, residues and numbering than the decoy: what does not match is ignored on both sides.
    ``n_ref_pairs``: the reference's residue pairs (fnat's denominator); ``n_pairs``: those whose two residues the
    decoy has; ``zone_sizes``: matched backbone atoms of (interface zone, long chain, short chain); ``long_chain``."""

    def __init__(self, table, ref_chain, ref_res_seq, ref_atom_name, ref_xyz, izone_cutoff=10.0, fnat_cutoff=5.0):
        if table.atom_name is None:
            raise ValueError("the scores match atoms by name: build the AtomTable with atom_name=")
        ref_chain = np.asarray(ref_chain).astype("U")
        seq = np.asarray(ref_res_seq).astype(np.int64)
        name = np.asarray(ref_atom_name).astype("U")
        xyz = np.asarray(ref_xyz, dtype=np.float64)
        if not (ref_chain.shape == seq.shape == name.shape == xyz.shape[:1]) or xyz.shape[1:] != (3,):
            raise ValueError("ref_chain, ref_res_seq, ref_atom_name [N] and ref_xyz [N,3] must describe the same atoms")
        self.table = table
        self.izone_cutoff, self.fnat_cutoff = float(izone_cutoff), float(fnat_cutoff)
        side = np.full(ref_chain.shape, -1, dtype=np.int64)
        side[ref_chain == table.chains[0]] = 0
        side[ref_chain == table.chains[1]] = 1
        at = [np.flatnonzero(side == s) for s in (0, 1)]
        useq, inv = zip(*[np.unique(seq[a], return_inverse=True) for a in at])       # residues of each chain by res_seq
        if len(useq[0]) == 0 or len(useq[1]) == 0:
            raise ValueError("the reference has no atoms of chain %r or %r" % tuple(table.chains))
        nb = len(useq[1])
        near = [_residue_pairs(xyz[at[0]], inv[0], xyz[at[1]], inv[1], nb, c) for c in (self.fnat_cutoff, self.izone_cutoff)]
        self.n_ref_pairs = int(near[0].shape[0])
        if self.n_ref_pairs == 0:
            raise ValueError("the reference has no residue pair within %g" % self.fnat_cutoff)
        zone = (set(useq[0][near[1] // nb].tolist()), set(useq[1][near[1] % nb].tolist()))
        self.long_chain = 0 if len(useq[0]) >= len(useq[1]) else 1
        # the table's residues by (side, res_seq); the reference pairs whose two residues the decoy has
        res_of = {(int(c), int(q)): r for r, (c, q) in enumerate(zip(table.res_chain, table.res_seq))}
        pairs = [(res_of.get((0, int(useq[0][k // nb]))), res_of.get((1, int(useq[1][k % nb])))) for k in near[0]]
        pairs = [p for p in pairs if p[0] is not None and p[1] is not None]
        self.pair_res = np.array(pairs, dtype=np.int32).reshape(-1, 2)
        # matching: the first reference atom of every (side, res_seq, name)
        ref_of = {}
        for k in np.flatnonzero(side >= 0)[::-1]:
            ref_of[(int(side[k]), int(seq[k]), str(name[k]))] = int(k)
        res_of_atom = np.repeat(np.arange(table.n_residues), np.diff(table.atom_ptr))
        zones = ([], [], [])
        for i in np.flatnonzero(np.isin(table.atom_name, BACKBONE)):
            r = res_of_atom[i]
            c, q = int(table.res_chain[r]), int(table.res_seq[r])
            k = ref_of.get((c, q, str(table.atom_name[i])))
            if k is None:
                continue
            if q in zone[c]:
                zones[0].append((i, k))
            zones[1 if c == self.long_chain else 2].append((i, k))
        self.zone_sizes = tuple(len(z) for z in zones)
        if min(self.zone_sizes) < 3:
            raise ValueError("a zone of fewer than 3 matched backbone atoms (interface, long chain, short chain: %d, %d, %d)"
                             % self.zone_sizes)
        both = np.array(zones[0] + zones[1] + zones[2], dtype=np.int64)
        self.zone_atom = np.ascontiguousarray(both[:, 0], dtype=np.int32)
        self.zone_ref = np.ascontiguousarray(xyz[both[:, 1]], dtype=np.float64)
        self.zone_ptr = np.concatenate(([0], np.cumsum(self.zone_sizes))).astype(np.int32)
        self.atom_ptr = np.ascontiguousarray(table.atom_ptr, dtype=np.int32)
        self._device = {}

    @property
    def n_pairs(self):
        return int(self.pair_res.shape[0])

    def device_tables(self, device):
        """(zone_atom, zone_ref, pair_res, atom_ptr) on ``device``, uploaded once"""
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(a).to(device) for a in
                                      (self.zone_atom, self.zone_ref, self.pair_res.reshape(-1), self.atom_ptr))
        return self._device[key]


def dock_scores_raw(api, xyz, zone_atom, zone_ptr, zone_ref, pair_res, atom_ptr, n_ref_pairs, fnat_cutoff=5.0, device="cpu",
                    tables=None):
    """One drgnn_dock_scores call (include/drgnn.h) over numpy arrays: xyz float32 [M,T,3].  Returns (scores float64
    [M,4], classes int32 [M,2], n_preserved int32 [M]) as numpy arrays.  ``tables``: the four index tables already on
    the device."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if np.shape(zone_ptr) != (4,) or xyz.ndim != 3 or xyz.shape[2] != 3:
        raise ValueError("zone_ptr [4] and xyz [M,T,3]")
    r = Request(_lib.ScoreRequest, device)
    d_za, d_zr, d_pr, d_ap = tables if tables is not None else (None,) * 4
    r.table("zone_atom", zone_atom, device_copy=d_za)
    r.host_table("zone_ptr", zone_ptr)
    r.input("zone_ref", zone_ref if d_zr is None else d_zr, torch.float64, error="zone_ref on the device must be float64")
    pairs = r.table("pair_res", pair_res, device_copy=d_pr)[0]
    ap = r.table("atom_ptr", atom_ptr, device_copy=d_ap)[0]
    r.input("xyz", xyz, torch.float32)
    M = int(xyz.shape[0])
    r.set(n_poses=M, n_atoms=int(xyz.shape[1]), n_residues=len(ap) - 1, n_pairs=pairs.shape[0] // 2,
          n_ref_pairs=int(n_ref_pairs), fnat_cutoff=float(fnat_cutoff))
    scores = r.output("scores", (M, 4), torch.float64)
    classes = r.output("classes", (M, 2), torch.int32)
    kept = r.output("n_preserved", M, torch.int32)
    r.run(api, "dock_scores")
    return scores.cpu().numpy(), classes.cpu().numpy(), kept.cpu().numpy()


def docking_scores(poses_or_table, reference, device=None, api=None, chunk=None):
    """The scores of M poses of ``reference.table`` (an ``AtomTable.poses`` batch, the table itself, or xyz float32
    [M,T,3] already in the table's grouped atom order) against ``reference``: a dict of numpy arrays [M], ``irmsd``,
    ``lrmsd`` (A), ``fnat``, ``dockQ`` float64, ``binclass``, ``capri_class``, ``n_preserved`` int64.  One launch per
    ``chunk`` poses (default: what keeps the uploaded coordinates within SCORE_XYZ_BUDGET bytes); a pose's result does
    not depend on the chunk, on its place in the batch or on the run."""
    api = api or _lib.get()
    device = _default_device(api, device)
    t, xyz = _pose_batch(poses_or_table, reference.table, "the poses must be of the reference's AtomTable")
    if chunk is None:
        chunk = SCORE_XYZ_BUDGET // (12 * max(t.n_atoms, 1))
    chunk = max(1, int(chunk))
    tables = reference.device_tables(device)
    parts = [dock_scores_raw(api, xyz[lo:lo + chunk], reference.zone_atom, reference.zone_ptr, reference.zone_ref,
                             reference.pair_res, reference.atom_ptr, reference.n_ref_pairs, reference.fnat_cutoff, device, tables)
             for lo in range(0, xyz.shape[0], chunk)]
    sc = np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, 4))
    cl = np.concatenate([p[1] for p in parts]) if parts else np.zeros((0, 2), np.int32)
    kept = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, np.int32)
    return {"irmsd": sc[:, 0].copy(), "lrmsd": sc[:, 1].copy(), "fnat": sc[:, 2].copy(), "dockQ": sc[:, 3].copy(),
            "binclass": cl[:, 0].astype(np.int64), "capri_class": cl[:, 1].astype(np.int64), "n_preserved": kept.astype(np.int64)}


def attach_scores(store, names, scores):
    """``score/<key>`` of molecule ``names[i]`` of ``store`` = ``scores[key][i]`` for the keys of SCORE_KEYS and
    LDDT_KEYS that ``scores`` (what ``docking_scores`` or ``lddt_scores`` returns) holds; ``binclass`` is stored as a
    bool, as the reference does."""
    for i, mol in enumerate(names):
        for k in SCORE_KEYS + LDDT_KEYS:
            if k in scores:
                v = scores[k][i]
                store.set(str(mol), "score/" + k, np.asarray(bool(v)) if k == "binclass" else np.asarray(v))
    return store


# ---- lDDT and interface lDDT (csrc/drgnn_lddt.h) -----------------------------------------------------------------------
LDDT_KEYS = ("lddt", "ilddt")
LDDT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def _heavy(names):
    """bool [N]: not a hydrogen, by the name rule of ``counted_atoms``"""
    return np.array([str(n).lstrip("0123456789 ")[:1] != "H" for n in names], dtype=bool).reshape(-1)


class LddtReference(object):
    """The once-per-complex half of the lDDT (Mariani et al. 2013), on the host: the reference's heavy-atom pairs of
    different residues at ``d_ref < inclusion_radius`` on the table's two chains, the matching of the table's heavy
    atoms to the reference's by (chain, res_seq, atom name) (the first atom of a key on either side), and the tables
    ``drgnn_pose_lddt`` takes (include/drgnn.h): the matched pairs as entries grouped by owning residue, every pair in
    both directions.  The pairs are found ``rows`` reference atoms at a time.

    ``n_pairs`` / ``n_inter_pairs``: the reference's pairs and the inter-chain ones, unmatched atoms included (the
    denominators); ``n_matched_pairs``: those with both atoms in the table; ``n_pairs_of_residue`` /
    ``n_inter_pairs_of_residue`` int64 [R]: the reference's pairs with an end in each residue of the table;
    ``n_ref_atoms`` / ``n_matched_atoms``: the reference's heavy atoms on the two chains and those with a partner."""

    def __init__(self, table, ref_chain, ref_res_seq, ref_atom_name, ref_xyz, inclusion_radius=15.0,
                 thresholds=LDDT_THRESHOLDS, rows=256):
        if table.atom_name is None:
            raise ValueError("lDDT matches atoms by name: build the AtomTable with atom_name=")
        ref_chain = np.asarray(ref_chain).astype("U")
        seq = np.asarray(ref_res_seq).astype(np.int64)
        name = np.asarray(ref_atom_name).astype("U")
        xyz = np.asarray(ref_xyz, dtype=np.float64)
        if not (ref_chain.shape == seq.shape == name.shape == xyz.shape[:1]) or xyz.shape[1:] != (3,):
            raise ValueError("ref_chain, ref_res_seq, ref_atom_name [N] and ref_xyz [N,3] must describe the same atoms")
        thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        if not 1 <= thr.size <= 8 or not np.all(np.isfinite(thr)) or thr[0] < 0.0 or np.any(np.diff(thr) <= 0.0):
            raise ValueError("1 to 8 thresholds, not negative and increasing")
        self.table, self.inclusion_radius, self.thresholds = table, float(inclusion_radius), thr
        side = np.full(ref_chain.shape, -1, dtype=np.int64)
        side[ref_chain == table.chains[0]] = 0
        side[ref_chain == table.chains[1]] = 1
        at = np.flatnonzero((side >= 0) & _heavy(name))                # the reference's heavy atoms on the two chains
        n, R = int(at.size), table.n_residues
        side, seq, name, x = side[at], seq[at], name[at], xyz[at]
        res_id = np.unique(np.stack((side, seq), axis=1), axis=0, return_inverse=True)[1].reshape(-1) if n else np.zeros(0, np.int64)
        res_of = {(int(c), int(q)): r for r, (c, q) in enumerate(zip(table.res_chain, table.res_seq))}
        table_res = np.array([res_of.get((int(c), int(q)), -1) for c, q in zip(side, seq)], dtype=np.int64).reshape(-1)
        # matching: the first heavy atom of every (side, res_seq, name), in the table and in the reference
        res_of_atom = np.repeat(np.arange(R), np.diff(table.atom_ptr))
        table_of = {}
        for i in np.flatnonzero(_heavy(table.atom_name))[::-1]:
            r = res_of_atom[i]
            table_of[(int(table.res_chain[r]), int(table.res_seq[r]), str(table.atom_name[i]))] = int(i)
        partner, seen = np.full(n, -1, dtype=np.int64), set()
        for k in range(n):
            key = (int(side[k]), int(seq[k]), str(name[k]))
            if key not in seen:
                seen.add(key)
                partner[k] = table_of.get(key, -1)
        self.n_ref_atoms, self.n_matched_atoms = n, int((partner >= 0).sum())
        # the pairs i < j, `rows` atoms i at a time
        self.n_pairs = self.n_inter_pairs = 0
        self.n_pairs_of_residue, self.n_inter_pairs_of_residue = np.zeros(R, np.int64), np.zeros(R, np.int64)
        found, col = [], np.arange(n)
        for lo in range(0, n, rows):
            hi = min(lo + rows, n)
            dx, dy, dz = (x[lo:hi, None, a] - x[None, :, a] for a in range(3))
            d = np.sqrt((dx * dx + dy * dy) + dz * dz)
            i, j = np.nonzero((d < self.inclusion_radius) & (res_id[lo:hi, None] != res_id[None, :]) & (col[None, :] > col[lo:hi, None]))
            d, i = d[i, j], i + lo
            inter = side[i] != side[j]
            self.n_pairs += int(i.size)
            self.n_inter_pairs += int(inter.sum())
            for end in (i, j):
                r = table_res[end]
                self.n_pairs_of_residue += np.bincount(r[r >= 0], minlength=R)
                self.n_inter_pairs_of_residue += np.bincount(r[(r >= 0) & inter], minlength=R)
            both = (partner[i] >= 0) & (partner[j] >= 0)
            found.append((partner[i][both], partner[j][both], d[both]))
        if self.n_pairs == 0:
            raise ValueError("the reference has no atom pair within %g" % self.inclusion_radius)
        if self.n_inter_pairs == 0:
            raise ValueError("the reference has no inter-chain atom pair within %g" % self.inclusion_radius)
        ti, tj, d = (np.concatenate([f[a] for f in found]) for a in range(3))
        self.n_matched_pairs = int(ti.size)
        if 2 * self.n_matched_pairs > 2 ** 31 - 1:
            raise ValueError("%d matched pairs are too many for int32 entry offsets" % self.n_matched_pairs)
        # entries: every pair under both of its atoms, grouped by the residue of the first, sorted by (self, other)
        own, other, d = np.concatenate((ti, tj)), np.concatenate((tj, ti)), np.concatenate((d, d))
        order = np.lexsort((other, own))                               # (atoms are grouped by residue: by residue too)
        self.self_atom = np.ascontiguousarray(own[order], dtype=np.int32)
        self.other_atom = np.ascontiguousarray(other[order], dtype=np.int32)
        self.d_ref = np.ascontiguousarray(d[order], dtype=np.float64)
        self.entry_ptr = np.concatenate(([0], np.cumsum(np.bincount(res_of_atom[own], minlength=R)))).astype(np.int32)
        self.n_chain_a_atoms = int(table.atom_ptr[table.split])
        self._device = {}

    def device_tables(self, device):
        """(entry_ptr, self_atom, other_atom, d_ref) on ``device``, uploaded once"""
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(a).to(device) for a in
                                      (self.entry_ptr, self.self_atom, self.other_atom, self.d_ref))
        return self._device[key]


def lddt_raw(api, xyz, entry_ptr, self_atom, other_atom, d_ref, n_chain_a_atoms, thresholds=LDDT_THRESHOLDS,
             residue_counts=False, device="cpu", tables=None, poses_per_pass=0):
    """One drgnn_pose_lddt call (include/drgnn.h) over numpy arrays: xyz float32 [M,T,3].  Returns (counts int32 [M,2,K],
    residue_counts int32 [M,R,2,K] or None) as numpy arrays.  ``tables``: the four entry tables already on the device."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if xyz.ndim != 3 or xyz.shape[2] != 3 or not 1 <= thr.size <= 8:
        raise ValueError("xyz [M,T,3] and 1 to 8 thresholds")
    r = Request(_lib.LddtRequest, device)
    d_ep, d_sa, d_oa, d_dr = tables if tables is not None else (None,) * 4
    ep = r.table("entry_ptr", entry_ptr, device_copy=d_ep)[0]
    sa = r.table("self_atom", self_atom, device_copy=d_sa)[0]
    r.table("other_atom", other_atom, device_copy=d_oa)
    r.input("d_ref", d_ref if d_dr is None else d_dr, torch.float64, error="d_ref on the device must be float64")
    r.input("xyz", xyz, torch.float32)
    M, R, K = int(xyz.shape[0]), len(ep) - 1, int(thr.size)
    r.set(n_poses=M, n_atoms=int(xyz.shape[1]), n_residues=R, n_entries=int(sa.shape[0]), n_chain_a_atoms=int(n_chain_a_atoms),
          thresholds=type(r.q.thresholds)(*thr.tolist()), n_thresholds=K, poses_per_pass=int(poses_per_pass))
    counts = r.output("counts", (M, 2, K), torch.int32)
    per_res = r.output("residue_counts", (M, R, 2, K), torch.int32) if residue_counts else None
    r.run(api, "pose_lddt")
    return counts.cpu().numpy(), per_res.cpu().numpy() if residue_counts else None


def lddt_scores(poses_or_table, reference, per_residue=False, device=None, api=None, chunk=None):
    """The lDDT of M poses of ``reference.table`` (an ``AtomTable.poses`` batch, the table itself, or xyz float32
    [M,T,3] already in the table's grouped atom order) against ``reference``, an ``LddtReference``: a dict of numpy
    arrays, ``lddt`` and ``ilddt`` (the inter-chain pairs alone) float64 [M] and ``preserved`` int64 [M,2,K], the
    preserved pairs (all, inter-chain) at each threshold; with ``per_residue`` also ``residue_lddt`` and
    ``residue_ilddt`` float64 [M,R] (NaN: a residue without a reference pair) and ``residue_preserved`` int64 [M,R,2,K].
    A score is the fp64 quotient of the summed counts and K times the reference's pairs.  One call per ``chunk`` poses
    (default: what keeps the uploaded coordinates, and the per-residue counts, within SCORE_XYZ_BUDGET bytes); a pose's
    result does not depend on the chunk, on its place in the batch or on the run."""
    api = api or _lib.get()
    device = _default_device(api, device)
    t, xyz = _pose_batch(poses_or_table, reference.table, "the poses must be of the reference's AtomTable")
    K, R = int(reference.thresholds.size), t.n_residues
    if chunk is None:
        chunk = SCORE_XYZ_BUDGET // max(12 * t.n_atoms, 8 * K * R if per_residue else 1, 1)
    chunk = max(1, int(chunk))
    tables = reference.device_tables(device)
    parts = [lddt_raw(api, xyz[lo:lo + chunk], reference.entry_ptr, reference.self_atom, reference.other_atom, reference.d_ref,
                      reference.n_chain_a_atoms, reference.thresholds, per_residue, device, tables)
             for lo in range(0, xyz.shape[0], chunk)]
    counts = np.concatenate([p[0] for p in parts]).astype(np.int64) if parts else np.zeros((0, 2, K), np.int64)
    total = counts.sum(axis=2).astype(np.float64)
    out = {"lddt": total[:, 0] / np.float64(K * reference.n_pairs), "ilddt": total[:, 1] / np.float64(K * reference.n_inter_pairs),
           "preserved": counts}
    if per_residue:
        rc = np.concatenate([p[1] for p in parts]).astype(np.int64) if parts else np.zeros((0, R, 2, K), np.int64)
        total = rc.sum(axis=3).astype(np.float64)
        for c, (key, pairs) in enumerate((("residue_lddt", reference.n_pairs_of_residue),
                                          ("residue_ilddt", reference.n_inter_pairs_of_residue))):
            den = (K * pairs).astype(np.float64)
            out[key] = total[:, :, c] / np.where(den > 0, den, np.nan)[None, :]
        out["residue_preserved"] = rc
    return out
