"""Docking poses of one topology as a set, on the device: interface contacts and the fraction of common contacts
(csrc/drgnn_fcc.h), the contact consensus (csrc/drgnn_consensus.h), the pairwise RMSD (csrc/drgnn_rmsd.h) and the
clustering by either relation (csrc/drgnn_posecluster.h)."""
import numpy as np
import torch

from . import _lib
from ._request import Request
from .atoms import AtomTable, Poses, _default_device, _pose_batch, counted_atoms, select_atoms

# ---- clustering of poses by their fraction of common contacts (csrc/drgnn_fcc.h) -----------------------------------
FCC_XYZ_BUDGET = 256 << 20         # bytes of pose coordinates one drgnn_pose_contacts call uploads (sets the default chunk)


class PoseContacts(object):
    """``pose_contacts``: ``bits`` int64 [M, nA, WB] on the device (the 64-bit words of drgnn_pose_contacts: bit b % 64
    of word b / 64 of row a says that residue a of the first chain and residue b of the second are in contact),
    ``n_contacts`` int64 [M] on the host, ``table``, ``n_a`` / ``n_b`` the residues of the two chains."""

    def __init__(self, table, bits, n_contacts, api, device, cutoff, heavy_only):
        self.table, self.bits, self.n_contacts, self.api, self.device = table, bits, n_contacts, api, device
        self.cutoff, self.heavy_only = cutoff, heavy_only
        self.n_a, self.n_b = table.split, table.n_residues - table.split

    def __len__(self):
        return int(self.n_contacts.shape[0])

    def words(self, m=None):
        """the words as numpy uint64 [M, nA, WB], or [nA, WB] of pose m"""
        w = (self.bits if m is None else self.bits[m]).cpu().numpy().view(np.uint64)
        return w

    def pairs(self, m):
        """int32 [n_m, 2]: the contacts of pose m as (residue of the first chain, residue of the second), both indices
        into the table's residues, sorted"""
        if self.n_a == 0 or self.n_b == 0:
            return np.zeros((0, 2), np.int32)
        w = self.words(m)
        on = np.unpackbits(w.view(np.uint8).reshape(self.n_a, -1), axis=1, bitorder="little")[:, :self.n_b]
        a, b = np.nonzero(on)
        return np.stack((a, b + self.n_a), axis=1).astype(np.int32)

    def select(self, index):
        """the ``PoseContacts`` of the poses ``index`` (int [K], in that order; a pose may repeat), its bits gathered on
        the device: what carries the best few thousand of a large set into ``cluster_poses``"""
        idx = np.asarray(index)
        if idx.dtype == bool or idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
            raise ValueError("index must be a list of pose indices")
        idx = idx.astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise ValueError("index must lie in [0, %d)" % len(self))
        bits = self.bits.index_select(0, torch.from_numpy(idx).to(self.bits.device))
        return PoseContacts(self.table, bits, self.n_contacts[idx], self.api, self.device, self.cutoff, self.heavy_only)


def pose_contacts_raw(api, xyz, atom_ptr, n_chain_a, cutoff=5.0, device="cpu"):
    """One drgnn_pose_contacts call (include/drgnn.h) over numpy arrays: xyz float32 [M, T, 3] of the counted atoms.
    Returns (bits int64 [M, nA, WB], n_contacts int32 [M]) as tensors on ``device``."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    r = Request(_lib.PoseContactsRequest, device)
    r.input("xyz", xyz, torch.float32)
    M, R, nA = int(xyz.shape[0]), len(r.table("atom_ptr", atom_ptr)[0]) - 1, int(n_chain_a)
    r.set(n_poses=M, n_atoms=int(xyz.shape[1]), n_residues=R, n_chain_a=nA, cutoff=float(cutoff))
    bits = r.output("bits", (M, max(nA, 0), (max(R - nA, 0) + 63) // 64), torch.int64)
    count = r.output("n_contacts", M, torch.int32)
    r.run(api, "pose_contacts")
    return bits, count


def pose_contacts(poses, cutoff=5.0, heavy_only=None, device=None, api=None, chunk=None, table=None):
    """The interface contacts of M poses of one topology (an ``AtomTable.poses`` batch, a table, or xyz float32 [M,T,3]
    in the grouped atom order of ``table``), on the device: residue a of the first chain and residue b of the second are
    in contact when a counted atom of each lie within ``cutoff`` A (d^2 <= float32(cutoff^2) on the float32 coordinates,
    the rule of ``fnat``).  ``heavy_only``: hydrogens do not count (the default when the table has atom names).  Returns a
    ``PoseContacts``; a pose's bits do not depend on M, on ``chunk`` (poses per launch), on its place or on the run."""
    if not float(cutoff) > 0.0 or not float(cutoff) < 1e18:
        raise ValueError("cutoff must be > 0")
    t, xyz = _pose_batch(poses, table)
    keep, atom_ptr = counted_atoms(t, heavy_only)
    api = api or _lib.get()
    device = _default_device(api, device)
    if t.n_residues > api.fcc_capacity(0):
        _lib._check(-2, "drgnn_pose_contacts")
    if chunk is None:
        chunk = FCC_XYZ_BUDGET // (12 * max(len(keep), 1))
    chunk = max(1, int(chunk))
    nA, WB = t.split, (t.n_residues - t.split + 63) // 64
    parts = [pose_contacts_raw(api, xyz[lo:lo + chunk][:, keep], atom_ptr, nA, cutoff, device)
             for lo in range(0, xyz.shape[0], chunk)]
    if parts:
        bits = torch.cat([p[0] for p in parts]) if len(parts) > 1 else parts[0][0]
        count = np.concatenate([p[1].cpu().numpy() for p in parts]).astype(np.int64)
    else:
        bits, count = torch.empty((0, nA, WB), dtype=torch.int64, device=torch.device(device)), np.zeros(0, np.int64)
    return PoseContacts(t, bits, count, api, device, float(cutoff), len(keep) != t.n_atoms)


def pose_common_raw(api, bits_a, bits_b):
    """One drgnn_pose_common call over tensors of words [Ma, W] and [Mb, W] (one device): int32 [Ma, Mb] on that device"""
    Ma, Mb, W = int(bits_a.shape[0]), int(bits_b.shape[0]), int(bits_a.shape[1])
    r = Request(_lib.PoseCommonRequest, bits_a.device)
    r.input("bits_a", bits_a)
    r.input("bits_b", bits_b)
    r.set(n_a=Ma, n_b=Mb, n_words=W)
    out = r.output("common", (Ma, Mb), torch.int32)
    r.run(api, "pose_common")
    return out


def _blocked_pairs(raw, A, B, block, dtype, symmetric=False):
    """``raw(rows of A, rows of B)`` over blocks of at most ``block`` rows a side, as one tensor [len(A), len(B)].
    ``symmetric`` (B is A): a diagonal block gets one tensor object as both sides, a block above the diagonal is computed
    once and mirrored by ``.t()``"""
    if len(A) <= block and len(B) <= block:
        return raw(A, B)
    out = torch.empty((len(A), len(B)), dtype=dtype, device=A.device)
    for i in range(0, len(A), block):
        for j in range(i if symmetric else 0, len(B), block):
            rows = A[i:i + block]
            part = raw(rows, rows if symmetric and j == i else B[j:j + block])
            out[i:i + block, j:j + block] = part
            if symmetric and j > i:
                out[j:j + block, i:i + block] = part.t()
    return out


def _common_device(a, b=None):
    """common contacts of two ``PoseContacts`` as an int32 tensor [M, M2] on their device; calls of at most
    drgnn_fcc_capacity(1) poses a side"""
    b = a if b is None else b
    if not isinstance(a, PoseContacts) or not isinstance(b, PoseContacts):
        raise ValueError("common contacts are taken between PoseContacts (pose_contacts)")
    if (a.n_a, a.n_b) != (b.n_a, b.n_b) or a.api is not b.api or torch.device(a.device) != torch.device(b.device):
        raise ValueError("the two sets of contacts must be of one topology, library and device")
    W = a.n_a * ((a.n_b + 63) // 64)
    wa, wb = a.bits.reshape(len(a), W), b.bits.reshape(len(b), W)
    if len(a) == 0 or len(b) == 0:
        return torch.zeros((len(a), len(b)), dtype=torch.int32, device=wa.device)
    return _blocked_pairs(lambda x, y: pose_common_raw(a.api, x, y), wa, wb, a.api.fcc_capacity(1), torch.int32)


def common_contacts(a, b=None):
    """int32 [M, M2]: the number of contacts pose i of ``a`` shares with pose j of ``b`` (``b`` None: of ``a`` itself; the
    diagonal is then ``n_contacts``).  ``a`` and ``b`` are ``PoseContacts`` of one topology."""
    return _common_device(a, b).cpu().numpy()


def fcc_matrix(a, b=None):
    """float64 [M, M2]: the fraction of the contacts of pose i of ``a`` that pose j of ``b`` has too, ``common[i, j] /
    n_contacts[i]`` as one float64 division; a pose without contacts has a row of zeros.  Not symmetric."""
    common = common_contacts(a, b).astype(np.float64)
    n = a.n_contacts.astype(np.float64)
    out = np.zeros_like(common)
    has = n > 0
    out[has] = common[has] / n[has, None]
    return out


class PoseClusters(object):
    """``cluster_poses``: ``labels`` int64 [M] (the cluster of every pose in order of discovery, -1: in none),
    ``centres`` / ``sizes`` int64 [K] per cluster, ``n_contacts`` int64 [M] (None from ``cluster_poses_rmsd``)."""

    def __init__(self, labels, centres, sizes, n_contacts):
        self.labels, self.centres, self.sizes, self.n_contacts = labels, centres, sizes, n_contacts

    def __len__(self):
        return int(self.centres.shape[0])

    def rank(self, scores, top=4, ascending=False):
        """(order int64 [K], means float64 [K]): the clusters ordered by the mean of their ``top`` best member scores
        (HADDOCK's convention; all members of a smaller cluster), best first, ties by cluster ordinal; ``means`` per
        cluster ordinal.  ``scores`` [M]: what ``Ensemble.predict`` or ``docking_scores()[key]`` gives for the same
        poses; ``ascending``: the smaller score is the better one."""
        if torch.is_tensor(scores):
            scores = scores.detach().cpu().numpy()
        scores = np.asarray(scores, dtype=np.float64).reshape(-1)
        if scores.shape[0] != self.labels.shape[0]:
            raise ValueError("%d scores for %d poses" % (scores.shape[0], self.labels.shape[0]))
        if int(top) < 1:
            raise ValueError("top must be >= 1")
        means = np.zeros(len(self))
        for k in range(len(self)):
            s = np.sort(scores[self.labels == k])
            means[k] = (s if ascending else s[::-1])[:int(top)].mean()
        order = np.lexsort((np.arange(len(self)), means if ascending else -means))
        return order.astype(np.int64), means

    def consensus(self, contacts):
        """the ``ContactFrequency`` of every cluster: ``contact_frequency(contacts, groups=self.labels,
        n_groups=len(self))`` for the ``PoseContacts`` of the clustered poses"""
        if not isinstance(contacts, PoseContacts):
            raise ValueError("a consensus is taken from PoseContacts (pose_contacts)")
        if len(contacts) != self.labels.shape[0]:
            raise ValueError("%d poses for %d labels" % (len(contacts), self.labels.shape[0]))
        return contact_frequency(contacts, groups=self.labels, n_groups=len(self))


def _cluster_launch(api, method, r, n_poses, min_size):
    """One clustering call, whatever the rule (csrc/drgnn_posecluster.h): the Request ``r`` holds the rule's own fields;
    this adds the shared fields and the outputs, runs the entry point ``method`` and returns the dict
    ``pose_cluster_raw`` documents"""
    M = int(n_poses)
    nb = r.output(("neighbours", "transposed"), (2, M, (M + 63) // 64), torch.int64, zeros=True)
    res = r.output(("labels", "centres", "sizes"), (3, M), torch.int32, zeros=True)
    k = r.output("n_clusters", 1, torch.int32, zeros=True)
    r.set(n_poses=M, min_size=int(min_size))
    r.run(api, method)
    K = int(k.cpu()[0])
    res, nb = res.cpu().numpy(), nb.cpu().numpy().view(np.uint64)
    return {"labels": res[0].copy(), "centres": res[1, :K].copy(), "sizes": res[2, :K].copy(), "neighbours": nb[0].copy(),
            "transposed": nb[1].copy()}


def _check_min_size(min_size):
    if int(min_size) != min_size or int(min_size) < 1:
        raise ValueError("min_size must be an integer >= 1")


def _pose_clusters(r, n_contacts):
    """the ``PoseClusters`` of a raw result (None: of no poses)"""
    r = r or dict.fromkeys(("labels", "centres", "sizes"), np.zeros(0, np.int32))
    return PoseClusters(r["labels"].astype(np.int64), r["centres"].astype(np.int64), r["sizes"].astype(np.int64), n_contacts)


def pose_cluster_raw(api, common, n_contacts, cutoff_fcc=0.6, cutoff_reverse=0.45, min_size=4, device="cpu"):
    """One drgnn_pose_cluster call (include/drgnn.h): ``common`` int32 [M, M] and ``n_contacts`` int32 [M] as numpy arrays
    or tensors on ``device``.  Returns a dict of numpy arrays: labels int32 [M], centres / sizes int32 [K], neighbours /
    transposed uint64 [M, ceil(M/64)] (the directed relation and its transpose as bit rows)."""
    error = "common int32 [M, M] and n_contacts int32 [M]"
    r = Request(_lib.PoseClusterRequest, n_contacts.device if torch.is_tensor(n_contacts) else device)
    M = int(r.input("n_contacts", n_contacts, torch.int32, (None,), error).shape[0])
    r.input("common", common, torch.int32, (M, M), error)
    r.set(cutoff_fcc=float(cutoff_fcc), cutoff_reverse=float(cutoff_reverse))
    return _cluster_launch(api, "pose_cluster", r, M, min_size)


def cluster_poses(poses_or_contacts, cutoff_fcc=0.6, strictness=0.75, min_size=4, **contact_options):
    """FCC clustering of docking poses on the device (Rodrigues et al. 2012: the rule of HADDOCK's ``cluster_fcc``, with
    the tie between equally connected centres broken towards the smaller index; tests/fcc_ref.py states it in numpy).
    ``fcc[i, j]`` is the fraction of pose i's interface contacts that pose j has too.  Pose j is a neighbour of i when
    ``fcc[i, j] >= cutoff_fcc`` and ``fcc[j, i] >= cutoff_fcc * strictness``.  The alive pose with the most alive
    neighbours (the smallest index on a tie) becomes a centre as long as it has ``min_size - 1`` of them; it and they
    form a cluster and die.  ``poses_or_contacts``: a ``PoseContacts``, or what ``pose_contacts`` takes together with its
    options (cutoff, heavy_only, table, device, api, chunk).  Returns a ``PoseClusters``.  More poses than
    drgnn_fcc_capacity(2) (4096) are refused (DrgnnError, capacity)."""
    for name, v in (("cutoff_fcc", cutoff_fcc), ("strictness", strictness)):
        if not (float(v) > 0.0 and float(v) <= 1.0):
            raise ValueError("%s must lie in (0, 1]" % name)
    _check_min_size(min_size)
    c = poses_or_contacts
    if isinstance(c, PoseContacts):
        if contact_options:
            raise ValueError("contact options %s come with poses, not with PoseContacts" % sorted(contact_options))
    else:
        c = pose_contacts(c, **contact_options)
    M = len(c)
    if M == 0:
        return _pose_clusters(None, c.n_contacts)
    if M > c.api.fcc_capacity(2):
        _lib._check(-2, "drgnn_pose_cluster")
    count = torch.from_numpy(c.n_contacts.astype(np.int32)).to(c.bits.device)
    r = pose_cluster_raw(c.api, _common_device(c), count, float(cutoff_fcc), float(cutoff_fcc) * float(strictness),
                         int(min_size), c.device)
    return _pose_clusters(r, c.n_contacts)


# ---- contact consensus of poses (csrc/drgnn_consensus.h) ------------------------------------------------------------
def _contact_words(bits, n_b):
    """(the contiguous tensor, M, nA) of contact words int64 [M, nA, ceil(n_b / 64)]"""
    if bits.dtype != torch.int64 or bits.dim() != 3 or int(bits.shape[2]) != (int(n_b) + 63) // 64:
        raise ValueError("bits int64 [M, nA, %d]" % ((int(n_b) + 63) // 64))
    return bits.contiguous(), int(bits.shape[0]), int(bits.shape[1])


def contact_counts_raw(api, bits, n_b, order, group_ptr):
    """One drgnn_pose_contact_counts call (include/drgnn.h): ``bits`` a tensor of words int64 [M, nA, WB], ``order`` int
    [L] and ``group_ptr`` int [G+1] numpy arrays.  Returns (counts int32 [G, nA, n_b], residues int32 [G, nA + n_b]) as
    tensors on the device of ``bits``."""
    bits, M, nA = _contact_words(bits, n_b)
    r = Request(_lib.ContactCountsRequest, bits.device)
    r.input("bits", bits)
    L, G = len(r.table("order", order)[0]), max(len(r.table("group_ptr", group_ptr)[0]) - 1, 0)
    r.set(n_poses=M, n_chain_a=nA, n_chain_b=int(n_b), n_groups=G, n_listed=L)
    counts = r.output("counts", (G, nA, int(n_b)), torch.int32)
    residues = r.output("residues", (G, nA + int(n_b)), torch.int32)
    r.run(api, "pose_contact_counts")
    return counts, residues


def consensus_numerators_raw(api, bits, n_b, counts, row):
    """One drgnn_pose_consensus_numerators call: ``bits`` words int64 [M, nA, WB] and ``counts`` int32 [G, nA, n_b] as
    tensors on one device, ``row`` int [M] a numpy array (-1: no row).  Returns int64 [M] on that device."""
    bits, M, nA = _contact_words(bits, n_b)
    if counts.dtype != torch.int32 or counts.dim() != 3 or tuple(counts.shape[1:]) != (nA, int(n_b)) or counts.device != bits.device:
        raise ValueError("counts int32 [G, %d, %d] on the device of bits" % (nA, int(n_b)))
    r = Request(_lib.ConsensusNumeratorsRequest, bits.device)
    r.input("bits", bits)
    r.input("counts", counts)
    if len(r.table("row", row)[0]) != M:
        raise ValueError("%d rows for %d poses" % (np.size(row), M))
    r.set(n_poses=M, n_chain_a=nA, n_chain_b=int(n_b), n_groups=int(counts.shape[0]))
    out = r.output("numerators", M, torch.int64)
    r.run(api, "pose_consensus_numerators")
    return out


def consensus_bits_raw(api, counts, min_count):
    """One drgnn_pose_consensus_bits call: ``counts`` int32 [G, nA, nB] a tensor, ``min_count`` int [G] a numpy array.
    Returns (bits int64 [G, nA, WB], n_contacts int32 [G]) as tensors on the device of ``counts``."""
    if counts.dtype != torch.int32 or counts.dim() != 3:
        raise ValueError("counts int32 [G, nA, nB]")
    G, nA, nB = (int(v) for v in counts.shape)
    r = Request(_lib.ConsensusBitsRequest, counts.device)
    r.input("counts", counts)
    if len(r.table("min_count", min_count)[0]) != G:
        raise ValueError("%d thresholds for %d groups" % (np.size(min_count), G))
    r.set(n_chain_a=nA, n_chain_b=nB, n_groups=G)
    bits = r.output("bits", (G, nA, (nB + 63) // 64), torch.int64)
    n = r.output("n_contacts", G, torch.int32)
    r.run(api, "pose_consensus_bits")
    return bits, n


def _group_rows(groups, M, G, what="groups"):
    """int64 [M] from ``groups`` (None: all 0), checked against [-1, G)"""
    if groups is None:
        g = np.zeros(M, dtype=np.int64)
    else:
        if torch.is_tensor(groups):
            groups = groups.detach().cpu().numpy()
        g = np.asarray(groups)
        if g.ndim != 1 or g.shape[0] != M:
            raise ValueError("%d %s for %d poses" % (g.shape[0] if g.ndim == 1 else g.size, what, M))
        if g.size and not np.issubdtype(g.dtype, np.integer):
            raise ValueError("%s must be integers" % what)
        g = g.astype(np.int64)
    if g.size and (g.min() < -1 or g.max() >= G):
        raise ValueError("%s must lie in [-1, %d)" % (what, G))
    return g


class ContactFrequency(object):
    """``contact_frequency``: ``counts`` int32 [G, nA, nB] (the poses of group g that have residue a of the first chain
    and residue b of the second in contact) and ``residues`` int32 [G, nA + nB] (the poses of g in which a residue has any
    contact) on the device, ``n_poses`` int64 [G] on the host; ``table``, ``n_a`` / ``n_b``, ``cutoff`` and
    ``heavy_only`` of the ``PoseContacts`` it was counted from.  The accessors copy to the host once."""

    def __init__(self, contacts, counts, residues, n_poses):
        self.counts, self.residues, self.n_poses = counts, residues, n_poses
        self.table, self.api, self.device = contacts.table, contacts.api, contacts.device
        self.cutoff, self.heavy_only, self.n_a, self.n_b = contacts.cutoff, contacts.heavy_only, contacts.n_a, contacts.n_b
        self._host = {}

    def __len__(self):
        return int(self.n_poses.shape[0])

    def _on_host(self, name, g):
        if not 0 <= int(g) < len(self):
            raise ValueError("group must lie in [0, %d)" % len(self))
        if name not in self._host:
            self._host[name] = getattr(self, name).cpu().numpy()
        return self._host[name][int(g)]

    def _fraction(self, name, g):
        c, n = self._on_host(name, g).astype(np.float64), self.n_poses[int(g)]
        return c / np.float64(n) if n > 0 else np.zeros_like(c)

    def fraction(self, g=0):
        """float64 [nA, nB]: the fraction of the poses of group g with each contact (zeros for a group without poses)"""
        return self._fraction("counts", g)

    def residue_fraction(self, g=0):
        """float64 [R]: the fraction of the poses of group g in which each residue of the table is in contact: a
        per-residue array for ``attach_residue_features``"""
        return self._fraction("residues", g)

    def pairs(self, g=0, min_count=1):
        """int32 [n, 3]: (residue of the first chain, residue of the second, count) of the contacts at least
        ``min_count`` poses of group g have, both indices into the table's residues, sorted by the pair"""
        if int(min_count) != min_count or int(min_count) < 1:
            raise ValueError("min_count must be an integer >= 1")
        c = self._on_host("counts", g)
        a, b = np.nonzero(c >= int(min_count))
        return np.stack((a, b + self.n_a, c[a, b]), axis=1).astype(np.int32)

    def interface_residues(self, g=0, min_poses=1):
        """int64 [n], sorted: the residues in contact in at least ``min_poses`` poses of group g (for one group of all
        poses: ``interface_residues(contacts, min_poses)``)"""
        if int(min_poses) != min_poses or int(min_poses) < 1:
            raise ValueError("min_poses must be an integer >= 1")
        return np.flatnonzero(self._on_host("residues", g) >= int(min_poses)).astype(np.int64)


def contact_frequency(contacts, groups=None, n_groups=None):
    """How often the poses of a ``PoseContacts``, or of every group of them, have each residue pair in contact: the
    consensus map of CONSRANK (Oliva, Vangone and Cavallo 2013; tests/consensus_ref.py states the rule), counted on the
    device in one launch, linear in the poses.  ``groups`` int [M]: the group of every pose, -1 for none
    (``PoseClusters.labels`` as it is); None: one group of all poses.  ``n_groups``: G (default: the largest group + 1).
    A group lists its poses in index order.  Returns a ``ContactFrequency``."""
    if not isinstance(contacts, PoseContacts):
        raise ValueError("a contact frequency is taken from PoseContacts (pose_contacts)")
    M = len(contacts)
    if n_groups is not None and (int(n_groups) != n_groups or int(n_groups) < 0):
        raise ValueError("n_groups must be an integer >= 0")
    if groups is None:
        G = 1 if n_groups is None else int(n_groups)
        g = _group_rows(None, M, max(G, 1)) if G > 0 else np.full(M, -1, dtype=np.int64)
    else:
        g = _group_rows(groups, M, np.iinfo(np.int32).max if n_groups is None else int(n_groups))
        G = int(n_groups) if n_groups is not None else int(g.max()) + 1 if g.size else 0
    order = np.argsort(g, kind="stable")
    order = order[g[order] >= 0]
    group_ptr = np.concatenate(([0], np.cumsum(np.bincount(g[order], minlength=G)))).astype(np.int64)
    counts, residues = contact_counts_raw(contacts.api, contacts.bits, contacts.n_b, order, group_ptr)
    return ContactFrequency(contacts, counts, residues, np.diff(group_ptr).astype(np.int64))


def consensus_scores(contacts, frequency=None, groups=None, leave_one_out=False, return_numerators=False):
    """float64 [M]: the CONSRANK score of every pose of a ``PoseContacts``, the mean frequency of its contacts:
    ``num / (n * N)`` with num the sum of ``counts[row]`` over the pose's n contacts and N the poses of its row, one
    float64 division on the integers; 0.0 for a pose without contacts or in no group.  Without ``frequency`` the one of
    ``contacts`` and ``groups`` is built and every pose is scored against its own group; ``leave_one_out`` then leaves
    the pose itself out of its frequency, ``(num - n) / (n * (N - 1))`` (0.0 in a group of one).  With a ``frequency``
    any ``PoseContacts`` of its topology, library and device is scored, ``groups`` naming the row of every pose (None:
    row 0).  ``return_numerators``: (scores, num int64 [M])."""
    if not isinstance(contacts, PoseContacts):
        raise ValueError("consensus scores are taken of PoseContacts (pose_contacts)")
    M = len(contacts)
    if frequency is None:
        frequency = contact_frequency(contacts, groups)
        row = _group_rows(groups, M, max(len(frequency), 1))
    else:
        if leave_one_out:
            raise ValueError("leave_one_out needs the frequency built in the same call: a given frequency may not list the pose once")
        f = frequency
        if not isinstance(f, ContactFrequency):
            raise ValueError("frequency is a ContactFrequency (contact_frequency)")
        if (contacts.n_a, contacts.n_b) != (f.n_a, f.n_b) or contacts.api is not f.api or torch.device(contacts.device) != torch.device(f.device):
            raise ValueError("the contacts and the frequency must be of one topology, library and device")
        row = _group_rows(groups, M, len(f))
    api, step = contacts.api, max(1, contacts.api.consensus_capacity(3))
    parts = [consensus_numerators_raw(api, contacts.bits[lo:lo + step], contacts.n_b, frequency.counts, row[lo:lo + step])
             for lo in range(0, M, step)]
    num = np.concatenate([p.cpu().numpy() for p in parts]).astype(np.int64) if parts else np.zeros(0, np.int64)
    n = contacts.n_contacts.astype(np.int64)
    N = np.where(row >= 0, frequency.n_poses[np.maximum(row, 0)] if len(frequency) else 0, 0).astype(np.int64)
    top, den = (num - n, n * (N - 1)) if leave_one_out else (num, n * N)
    scores = np.zeros(M, dtype=np.float64)
    has = den > 0
    scores[has] = top[has].astype(np.float64) / den[has].astype(np.float64)
    return (scores, num) if return_numerators else scores


def consensus_contacts(frequency, min_fraction=0.5, min_count=None):
    """The consensus map of every group of a ``ContactFrequency`` as a ``PoseContacts`` of G rows: contact (a, b) of row g
    is set when at least ``min_count`` poses of g have it; ``min_fraction`` in (0, 1] means ``max(1, ceil(min_fraction *
    N_g))`` (float64), ``min_count`` an integer >= 1 (or one per group) instead.  ``fcc_matrix(poses, consensus)``,
    ``common_contacts``, ``interface_residues`` and ``pose_rmsd(kind="interface", residues=...)`` take it like any
    pose."""
    if not isinstance(frequency, ContactFrequency):
        raise ValueError("consensus contacts are taken from a ContactFrequency (contact_frequency)")
    G = len(frequency)
    if min_count is None:
        if not (float(min_fraction) > 0.0 and float(min_fraction) <= 1.0):
            raise ValueError("min_fraction must lie in (0, 1]")
        least = np.array([max(1, int(np.ceil(np.float64(min_fraction) * np.float64(n)))) for n in frequency.n_poses], dtype=np.int64)
    else:
        least = np.asarray(min_count)
        if (least.size and not np.issubdtype(least.dtype, np.integer)) or least.shape not in ((), (G,)) or (least < 1).any():
            raise ValueError("min_count must be an integer >= 1, or one per group")
        least = np.broadcast_to(least, (G,)).astype(np.int64)
    bits, n = consensus_bits_raw(frequency.api, frequency.counts, least)
    return PoseContacts(frequency.table, bits, n.cpu().numpy().astype(np.int64), frequency.api, frequency.device,
                        frequency.cutoff, frequency.heavy_only)


# ---- pairwise pose RMSD and RMSD clustering of poses (csrc/drgnn_rmsd.h) --------------------------------------------
RMSD_KINDS = ("ligand", "interface", "fixed", "all")
RMSD_WORKSPACE_BUDGET = 1 << 30    # bytes of fp64 pose records one drgnn_pose_rmsd call may ask for (sets the default chunk)


def _atom_list(what, idx, n_atoms, least):
    a = np.asarray(idx)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError("%s must be a list of atom indices" % what)
    if a.size < least:
        raise ValueError("%s needs at least %d atom%s" % (what, least, "" if least == 1 else "s"))
    if a.min() < 0 or a.max() >= n_atoms:
        raise ValueError("%s must be indices into the table's %d atoms" % (what, n_atoms))
    return np.ascontiguousarray(a, dtype=np.int32)


def rmsd_selection(table, rms=None, fit=None, kind=None, residues=None):
    """(rms int32 [nR], fit int32 [nF] or None) of ``pose_rmsd``: the two lists as given, or what ``kind`` stands for"""
    if kind is None:
        if rms is None:
            raise ValueError("pose_rmsd needs rms= (atom indices) or kind= (one of %s)" % ", ".join(RMSD_KINDS))
        if residues is not None:
            raise ValueError("residues= goes with kind=\"interface\"")
        return _atom_list("rms", rms, table.n_atoms, 1), None if fit is None else _atom_list("fit", fit, table.n_atoms, 3)
    if kind not in RMSD_KINDS:
        raise ValueError("kind must be one of %s" % ", ".join(RMSD_KINDS))
    if rms is not None or fit is not None:
        raise ValueError("kind= stands for rms= and fit=: give one or the other")
    if (kind == "interface") != (residues is not None):
        raise ValueError("residues= goes with kind=\"interface\", and that kind needs it")
    long_chain = 0 if table.split >= table.n_residues - table.split else 1
    if kind == "ligand":
        rms, fit = select_atoms(table, chain=1 - long_chain), select_atoms(table, chain=long_chain)
    elif kind == "fixed":
        rms, fit = select_atoms(table, chain=1 - long_chain), None
    else:
        rms = fit = select_atoms(table, residues=residues)
    return _atom_list("the rms atoms of kind %r" % kind, rms, table.n_atoms, 1), \
        None if fit is None else _atom_list("the fit atoms of kind %r" % kind, fit, table.n_atoms, 3)


def pose_rmsd_raw(api, xyz_a, xyz_b, rms_idx, fit_idx=None, phases=0, workspace=None, out=None):
    """One drgnn_pose_rmsd call (include/drgnn.h): ``xyz_a`` / ``xyz_b`` float32 tensors [Ma, T, 3] / [Mb, T, 3] on one
    device (the same tensor: the square matrix of one batch), the lists as numpy int32.  Returns float64 [Ma, Mb] on
    that device.  ``workspace`` / ``out``: tensors kept between calls that run the launches one by one (``phases``)."""
    r = Request(_lib.PoseRmsdRequest, xyz_a.device)
    error = "xyz float32 [Ma, T, 3] and [Mb, T, 3]"
    xyz_a = r.input("xyz_a", xyz_a, torch.float32, (None, None, 3), error)
    xyz_b = r.input("xyz_b", xyz_b, torch.float32, (None,) + tuple(xyz_a.shape[1:]), error)
    Ma, Mb, nR = int(xyz_a.shape[0]), int(xyz_b.shape[0]), len(r.table("rms_idx", rms_idx)[0])
    nF = 0 if fit_idx is None else len(r.table("fit_idx", fit_idx)[0])
    nbytes = api.rmsd_workspace(Ma, Mb, nF, nR)[0]
    if workspace is None:
        workspace = r.output("workspace", max(nbytes // 8, 1), torch.float64)
    else:
        r.input("workspace", workspace)
    d = r.output("d", (Ma, Mb), torch.float64) if out is None else r.input("d", out)
    r.set(n_a=Ma, n_b=Mb, n_atoms=int(xyz_a.shape[1]), n_fit=nF, n_rms=nR, phases=int(phases),
          workspace_bytes=workspace.numel() * 8)
    r.run(api, "pose_rmsd")
    return d


def pose_rmsd(poses, rms=None, fit=None, kind=None, other=None, residues=None, device=None, api=None, chunk=None, table=None):
    """The pose-by-pose RMSD matrix of M poses of one topology (an ``AtomTable.poses`` batch, a table, or xyz float32
    [M,T,3] in the grouped atom order of ``table``), on the device: a float64 tensor [M, M], or [M, M'] against the poses
    ``other`` of the same table.  ``rms``: the atoms the RMSD is taken over (indices in the table's grouped order, as
    ``select_atoms`` returns them); ``fit``: the atoms (at least 3, not collinear) that pose i is superposed on pose j
    by, with the optimal proper rotation and translation, before the RMSD is taken; None: no superposition.  ``kind``
    stands for both: ``"ligand"`` fit on the backbone of the chain with more residues (the first on a tie), RMSD of the
    other chain's backbone (pairwise l-RMSD); ``"interface"`` fit = rms = the backbone of ``residues`` (``interface_residues``;
    pairwise i-RMSD); ``"fixed"`` no superposition, the shorter chain's backbone (rigid-body runs with a fixed receptor);
    ``"all"`` fit = rms = every backbone atom.  tests/rmsd_ref.py states the rule.  The matrix is exactly symmetric with
    a zero diagonal; an entry does not depend on M, on ``chunk`` (poses per side of one launch, at most
    drgnn_rmsd_capacity(0)), on the side or the place of its poses or on the run."""
    t, xyz = _pose_batch(poses, table)
    xyz2 = None
    if other is not None:
        xyz2 = _pose_batch(other, t, "the other poses must be of the same AtomTable")[1]
    rms_idx, fit_idx = rmsd_selection(t, rms, fit, kind, residues)
    api = api or _lib.get()
    device = _default_device(api, device)
    dev = torch.device(device)
    # only the selected atoms are uploaded
    cols = np.unique(np.concatenate((rms_idx, fit_idx if fit_idx is not None else rms_idx[:0])))
    rms_idx = np.searchsorted(cols, rms_idx).astype(np.int32)
    fit_idx = None if fit_idx is None else np.searchsorted(cols, fit_idx).astype(np.int32)
    record = 8 * (3 * (len(rms_idx) + (0 if fit_idx is None else len(fit_idx))) + 2)
    cap = min(api.rmsd_capacity(0), max(1, RMSD_WORKSPACE_BUDGET // (2 * record)))
    chunk = cap if chunk is None else max(1, min(int(chunk), cap))
    M, M2 = int(xyz.shape[0]), int(xyz.shape[0] if xyz2 is None else xyz2.shape[0])
    if M == 0 or M2 == 0:
        return torch.zeros((M, M2), dtype=torch.float64, device=dev)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x[:, cols], dtype=np.float32)).to(dev)
    A = up(xyz)
    B = A if xyz2 is None else up(xyz2)
    return _blocked_pairs(lambda x, y: pose_rmsd_raw(api, x, y, rms_idx, fit_idx), A, B, chunk, torch.float64, xyz2 is None)


def interface_residues(contacts, min_poses=1):
    """int64 [n], sorted: the residues (indices into the table's residues, both chains) that are in contact in at least
    ``min_poses`` poses of a ``PoseContacts``: what ``pose_rmsd(kind="interface", residues=...)`` takes"""
    if not isinstance(contacts, PoseContacts):
        raise ValueError("interface residues are taken from PoseContacts (pose_contacts)")
    if int(min_poses) != min_poses or int(min_poses) < 1:
        raise ValueError("min_poses must be an integer >= 1")
    w = contacts.words()                                               # uint64 [M, nA, WB]
    if w.size == 0:
        return np.zeros(0, np.int64)
    in_a = (w != 0).any(axis=2).sum(axis=0)                            # poses in which a row has a bit
    cols = np.bitwise_or.reduce(w, axis=1)                             # [M, WB]: the OR over the rows
    in_b = np.unpackbits(np.ascontiguousarray(cols).view(np.uint8), axis=1, bitorder="little")[:, :contacts.n_b].sum(axis=0)
    return np.concatenate((np.flatnonzero(in_a >= int(min_poses)), contacts.n_a + np.flatnonzero(in_b >= int(min_poses)))).astype(np.int64)


def pose_cluster_dist_raw(api, d, cutoff=7.5, min_size=4, device="cpu"):
    """One drgnn_pose_cluster_dist call (include/drgnn.h): ``d`` float64 [M, M] as a numpy array or a tensor on
    ``device``.  Returns what ``pose_cluster_raw`` returns."""
    r = Request(_lib.PoseClusterDistRequest, d.device if torch.is_tensor(d) else device)
    M = int(np.shape(d)[0]) if np.ndim(d) else -1
    r.input("d", d, torch.float64, (M, M), "d float64 [M, M]")
    r.set(cutoff=float(cutoff))
    return _cluster_launch(api, "pose_cluster_dist", r, M, min_size)


def cluster_poses_rmsd(poses_or_matrix, cutoff=7.5, min_size=4, **rmsd_options):
    """RMSD clustering of docking poses on the device (the rule of HADDOCK's ``cluster_struc`` and of ClusPro, with the
    tie between equally connected centres broken towards the smaller index; tests/rmsd_ref.py states it in numpy).  Pose
    j is a neighbour of i when ``D[i, j] <= cutoff`` (A).  The alive pose with the most alive neighbours (the smallest
    index on a tie) becomes a centre as long as it has ``min_size - 1`` of them; it and they form a cluster and die.
    ``poses_or_matrix``: a square float64 matrix (a tensor, as ``pose_rmsd`` returns it, or a numpy array; ``api`` and
    ``device`` are then the only options), or what ``pose_rmsd`` takes together with its options (rms, fit, kind,
    residues, table, device, api, chunk).  Returns a ``PoseClusters`` with ``n_contacts`` None.  More poses than
    drgnn_rmsd_capacity(1) (4096) are refused (DrgnnError, capacity)."""
    if not (float(cutoff) > 0.0 and float(cutoff) < float("inf")):
        raise ValueError("cutoff must be a positive finite number")
    _check_min_size(min_size)
    if "other" in rmsd_options:
        raise ValueError("clustering takes the square matrix of one batch: no other=")
    p = poses_or_matrix
    is_matrix = (torch.is_tensor(p) or isinstance(p, np.ndarray)) and p.ndim == 2
    api = rmsd_options.get("api") or _lib.get()
    device = _default_device(api, rmsd_options.get("device") or (str(p.device) if torch.is_tensor(p) and is_matrix else None))
    if is_matrix:
        if set(rmsd_options) - {"api", "device"}:
            raise ValueError("rmsd options %s come with poses, not with a matrix" % sorted(set(rmsd_options) - {"api", "device"}))
        if p.shape[0] != p.shape[1]:
            raise ValueError("a distance matrix is square")
        M = int(p.shape[0])
    else:
        M = len(p) if isinstance(p, Poses) else 1 if isinstance(p, AtomTable) else int(np.asarray(p).shape[0])
    if M > api.rmsd_capacity(1):
        _lib._check(-2, "drgnn_pose_cluster_dist")
    if M == 0:
        if not is_matrix:
            pose_rmsd(p, **dict(rmsd_options, api=api, device=device))             # (the options are checked; nothing is launched)
        return _pose_clusters(None, None)
    d = p if is_matrix else pose_rmsd(p, **dict(rmsd_options, api=api, device=device))
    if torch.is_tensor(d):
        d = d.to(torch.float64)
    r = pose_cluster_dist_raw(api, d, float(cutoff), int(min_size), device)
    return _pose_clusters(r, None)
