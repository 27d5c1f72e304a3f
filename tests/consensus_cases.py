"""Inputs and checks shared by tests/test_consensus.py (host emulation) and tests/test_gpu_consensus.py (the device): the
contact consensus of deeprank_gnn_amd.interface (drgnn_pose_contact_counts / drgnn_pose_consensus_numerators /
drgnn_pose_consensus_bits, csrc/drgnn_consensus.h) against the numpy statement of the rule in tests/consensus_ref.py, and
against the O(M^2) route the package already has: a pose's numerator over the set it was counted from is the row sum of
common_contacts.

Every comparison is exact equality; the scores are compared bit for bit with the reference's own single division."""
import numpy as np

import consensus_ref as R
import fcc_cases as F
import fcc_ref
from bsa_cases import same_bits

# the four 1ATN poses, heavy atoms / all atoms, cutoff 5 A (computed on the CPU with the rule of fcc_ref)
ATN_NUM = {True: [142, 128, 154, 67], False: [175, 163, 187, 79]}
ATN_OCCURRENCES = {True: [27, 20, 16, 15], False: [32, 29, 24, 15]}      # contacts in exactly 1, 2, 3, 4 poses
ATN_RES_ANY = {True: (33, 28), False: (37, 32)}                         # residues of chain 0 / 1 in contact in >= 1 pose
ATN_RES_ALL = {True: (12, 12), False: (13, 14)}                         # ... in all four
# the 130-pose family batch of fcc_cases (nA = 108, nB = 95), on the reference alone
FAMILY_SIZES = [45, 23, 22, 12, 8]
FAMILY_CONSENSUS = {0.5: 26, 0.25: 68, 0.75: 3}
FAMILY_CLUSTER_CONSENSUS = [58, 21, 99, 8, 90]
FAMILY_LARGEST = 117
HAND_NB = (64, 65, 128, 129)
HAND_M = (1, 2, 63, 64, 65, 130)
ONES_M = (255, 256, 257, 1023, 1024, 1025)
FILL = -7
_CACHE = {}


# ---- words -------------------------------------------------------------------------------------------------------------
def pack(maps):
    """int64 words [M, nA, WB] of bool maps [M, nA, nB] in pose_contacts' layout, the tail bits zero"""
    maps = np.asarray(maps, dtype=bool)
    M, nA, nB = maps.shape
    WB = (nB + 63) // 64
    padded = np.zeros((M, nA, 64 * WB), dtype=bool)
    padded[:, :, :nB] = maps
    return np.ascontiguousarray(np.packbits(padded, axis=2, bitorder="little")).view(np.int64).reshape(M, nA, WB)


def with_tail(words, n_b):
    """the same words with every bit at or past n_b of a row's last word set"""
    out = words.copy()
    if n_b % 64 and out.size:
        out.view(np.uint64)[:, :, -1] |= np.uint64((2 ** 64 - 1) ^ (2 ** (n_b % 64) - 1))
    return out


def unpack(words, n_b):
    """bool [M, nA, n_b] of words; asserts the zero tail"""
    w = np.ascontiguousarray(words)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], w.shape[1], 8 * w.shape[2]), axis=2, bitorder="little")
    assert not bits[:, :, n_b:].any()
    return bits[:, :, :n_b].astype(bool)


def raw_outputs(api, device, words, n_b, order, group_ptr, row, min_count):
    """the three entry points over hand-packed words: (counts, residues, numerators, consensus words, n_contacts) as numpy"""
    import torch
    from deeprank_gnn_amd.interface import consensus_bits_raw, consensus_numerators_raw, contact_counts_raw
    d = torch.from_numpy(words).to(device)
    counts, residues = contact_counts_raw(api, d, n_b, order, group_ptr)
    num = consensus_numerators_raw(api, d, n_b, counts, row)
    bits, n = consensus_bits_raw(api, counts, min_count)
    return tuple(t.cpu().numpy() for t in (counts, residues, num, bits, n))


def check_raw(api, device, maps, order, group_ptr, row, min_count, tail=False, what=""):
    """raw_outputs against consensus_ref; returns them"""
    maps = np.asarray(maps, dtype=bool)
    n_b = maps.shape[2]
    words = pack(maps)
    got = raw_outputs(api, device, with_tail(words, n_b) if tail else words, n_b, order, group_ptr, row, min_count)
    counts, residues = R.counts_of(maps, order, group_ptr), R.residues_of(maps, order, group_ptr)
    want_bits = R.consensus_of(counts, min_count)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], counts), what
    assert got[1].dtype == np.int32 and np.array_equal(got[1], residues), what
    assert got[2].dtype == np.int64 and np.array_equal(got[2], R.numerators_of(maps, counts, row)), what
    assert np.array_equal(unpack(got[3], n_b), want_bits), what                       # (and the tail is zero)
    assert got[4].dtype == np.int32 and np.array_equal(got[4], want_bits.reshape(len(want_bits), -1).sum(axis=1)), what
    return got


def one_group(M):
    return np.arange(M), np.array([0, M])


# ---- 1 the rule, without a kernel ----------------------------------------------------------------------------------------
def check_ref_literals():
    """consensus_ref against the literals of the four 1ATN poses"""
    for heavy in (True, False):
        maps = F.atn_maps(heavy)
        order, ptr = one_group(4)
        counts, residues = R.counts_of(maps, order, ptr), R.residues_of(maps, order, ptr)
        num = R.numerators_of(maps, counts, np.zeros(4, dtype=np.int64))
        assert list(num) == ATN_NUM[heavy] and np.array_equal(num, fcc_ref.common_of(maps).sum(axis=1))
        assert [int((counts[0] == k).sum()) for k in (1, 2, 3, 4)] == ATN_OCCURRENCES[heavy]
        nA = maps.shape[1]
        assert ((residues[0, :nA] >= 1).sum(), (residues[0, nA:] >= 1).sum()) == ATN_RES_ANY[heavy]
        assert ((residues[0, :nA] == 4).sum(), (residues[0, nA:] == 4).sum()) == ATN_RES_ALL[heavy]
        assert sum(ATN_OCCURRENCES[heavy]) == int((counts[0] > 0).sum())
    n = np.array(F.ATN_N[True])
    s = R.scores_of(ATN_NUM[True], n, np.full(4, 4))
    assert s.dtype == np.float64 and s[0] == 142 / 212 and all(s[m] == ATN_NUM[True][m] / (n[m] * 4) for m in range(4))
    loo = R.scores_of(ATN_NUM[True], n, np.full(4, 4), leave_one_out=True)
    assert loo[0] == (142 - 53) / (53 * 3)
    assert list(R.scores_of([5, 0, 7], [0, 3, 2], [4, 0, 1], leave_one_out=False)) == [0.0, 0.0, 3.5]
    assert list(R.scores_of([5, 0, 7], [0, 3, 2], [4, 0, 1], leave_one_out=True)) == [0.0, 0.0, 0.0]
    assert list(R.min_count_of(0.5, [130, 1, 0, 3])) == [65, 1, 1, 2]


def family():
    """the reference on the 130-pose family batch, once: a dict; asserts what the batch is there for"""
    if "family" not in _CACHE:
        maps, common, n, (labels, centres, sizes, _) = F.family_ref()
        M, nA, nB = maps.shape
        assert (M, nA, nB) == (130, 108, 95) and list(sizes) == FAMILY_SIZES and (labels == -1).sum() == 20 and (n == 0).sum() == 2
        order, ptr = one_group(M)
        counts, residues = R.counts_of(maps, order, ptr), R.residues_of(maps, order, ptr)
        for frac, want in FAMILY_CONSENSUS.items():
            assert int(R.consensus_of(counts, R.min_count_of(frac, [M])).sum()) == want, frac
        assert list(R.min_count_of(0.5, [M])) == [65] and int(counts.max()) == FAMILY_LARGEST
        c_order, c_ptr = R.lists_of(labels, len(sizes))
        c_counts, c_residues = R.counts_of(maps, c_order, c_ptr), R.residues_of(maps, c_order, c_ptr)
        c_maps = R.consensus_of(c_counts, R.min_count_of(0.5, sizes))
        assert [int(m.sum()) for m in c_maps] == FAMILY_CLUSTER_CONSENSUS and list(np.diff(c_ptr)) == FAMILY_SIZES
        _CACHE["family"] = dict(maps=maps, common=common, n=n, labels=labels.astype(np.int64), sizes=sizes, counts=counts,
                                residues=residues, c_counts=c_counts, c_residues=c_residues, c_maps=c_maps)
    return _CACHE["family"]


def family_contacts(api, device):
    """the PoseContacts of the family batch on ``api`` / ``device``, once"""
    key = ("contacts", id(api), str(device))
    if key not in _CACHE:
        from deeprank_gnn_amd.interface import AtomTable, pose_contacts
        table, xyz = F.family_batch()
        _CACHE[key] = pose_contacts(AtomTable.poses(table, xyz), **F.kw(api, device))
        F.check_contacts(_CACHE[key], family()["maps"], "the family batch")
    return _CACHE[key]


# ---- 2 the identity with common_contacts ------------------------------------------------------------------------------------
def check_identity(api, device):
    from deeprank_gnn_amd.interface import (ContactFrequency, PoseContacts, cluster_poses, common_contacts, consensus_contacts,
                                            consensus_scores, contact_frequency, fcc_matrix, interface_residues)
    ref, c = family(), family_contacts(api, device)
    M, nA = len(c), c.n_a
    common = common_contacts(c)
    assert np.array_equal(common, ref["common"])
    # one group of all poses
    f = contact_frequency(c)
    assert isinstance(f, ContactFrequency) and len(f) == 1 and list(f.n_poses) == [M] and f.n_poses.dtype == np.int64
    assert (f.table, f.cutoff, f.heavy_only, f.n_a, f.n_b) == (c.table, c.cutoff, c.heavy_only, c.n_a, c.n_b)
    counts, residues = f.counts.cpu().numpy(), f.residues.cpu().numpy()
    assert counts.dtype == np.int32 and np.array_equal(counts, ref["counts"]) and int(counts.max()) == FAMILY_LARGEST
    assert residues.dtype == np.int32 and np.array_equal(residues, ref["residues"])
    s, num = consensus_scores(c, return_numerators=True)
    assert num.dtype == np.int64 and np.array_equal(num, common.astype(np.int64).sum(axis=1))
    assert np.array_equal(num, R.numerators_of(ref["maps"], ref["counts"], np.zeros(M, dtype=np.int64)))
    assert same_bits(s, R.scores_of(num, ref["n"], np.full(M, M))) and same_bits(s, consensus_scores(c, frequency=f))
    assert same_bits(consensus_scores(c, leave_one_out=True), R.scores_of(num, ref["n"], np.full(M, M), leave_one_out=True))
    assert (s[ref["n"] == 0] == 0.0).all() and (s[ref["n"] > 0] > 0.0).all()
    assert same_bits(f.fraction(0), ref["counts"][0].astype(np.float64) / np.float64(M))
    assert same_bits(f.residue_fraction(), ref["residues"][0].astype(np.float64) / np.float64(M))
    a, b = np.nonzero(ref["counts"][0] >= 3)
    assert same_bits(f.pairs(0, min_count=3), np.stack((a, b + nA, ref["counts"][0][a, b]), axis=1).astype(np.int32))
    assert len(f.pairs()) == int((ref["counts"][0] > 0).sum())
    for frac, want in FAMILY_CONSENSUS.items():
        cons = consensus_contacts(f, min_fraction=frac)
        assert isinstance(cons, PoseContacts) and len(cons) == 1 and list(cons.n_contacts) == [want] and cons.n_contacts.dtype == np.int64
        assert np.array_equal(unpack(cons.words(), c.n_b), R.consensus_of(ref["counts"], R.min_count_of(frac, [M])))
    # the clusters of the batch as groups
    clusters = cluster_poses(c)
    assert np.array_equal(clusters.labels, ref["labels"]) and list(clusters.sizes) == FAMILY_SIZES
    fc = clusters.consensus(c)
    assert len(fc) == 5 and list(fc.n_poses) == FAMILY_SIZES
    assert np.array_equal(fc.counts.cpu().numpy(), ref["c_counts"]) and np.array_equal(fc.residues.cpu().numpy(), ref["c_residues"])
    s, num = consensus_scores(c, groups=clusters.labels, return_numerators=True)
    same = (ref["labels"][:, None] == ref["labels"][None, :]) & (ref["labels"][:, None] >= 0)
    assert np.array_equal(num, (common.astype(np.int64) * same).sum(axis=1)) and not num[ref["labels"] < 0].any()
    N = np.where(ref["labels"] >= 0, ref["sizes"][np.maximum(ref["labels"], 0)], 0)
    assert same_bits(s, R.scores_of(num, ref["n"], N)) and same_bits(s, consensus_scores(c, frequency=fc, groups=clusters.labels))
    assert same_bits(consensus_scores(c, groups=clusters.labels, leave_one_out=True), R.scores_of(num, ref["n"], N, leave_one_out=True))
    cons = consensus_contacts(fc)
    assert list(cons.n_contacts) == FAMILY_CLUSTER_CONSENSUS and np.array_equal(unpack(cons.words(), c.n_b), ref["c_maps"])
    # a consensus map is a pose like any other
    both = fcc_ref.common_of(ref["maps"], ref["c_maps"])
    assert np.array_equal(common_contacts(c, cons), both)
    assert same_bits(fcc_matrix(c, cons), fcc_ref.fcc_of(both, ref["n"]))
    assert same_bits(fcc_matrix(cons, c), fcc_ref.fcc_of(both.T, ref["c_maps"].reshape(5, -1).sum(axis=1)))
    for k in (1, 2, 5):
        want = np.concatenate((np.flatnonzero(ref["c_maps"].any(axis=2).sum(axis=0) >= k),
                               nA + np.flatnonzero(ref["c_maps"].any(axis=1).sum(axis=0) >= k))).astype(np.int64)
        assert same_bits(interface_residues(cons, k), want)
    return c


def check_other_set(api, device):
    """the frequency of the first 100 poses scores the last 30"""
    from deeprank_gnn_amd.interface import common_contacts, consensus_scores, contact_frequency
    ref, c = family(), family_contacts(api, device)
    first, last = c.select(np.arange(100)), c.select(np.arange(100, 130))
    f = contact_frequency(first)
    s, num = consensus_scores(last, frequency=f, return_numerators=True)
    assert np.array_equal(num, common_contacts(last, first).astype(np.int64).sum(axis=1))
    assert np.array_equal(num, ref["common"][100:, :100].astype(np.int64).sum(axis=1))
    assert same_bits(s, R.scores_of(num, ref["n"][100:], np.full(30, 100)))
    rows = np.where(np.arange(30) % 3 == 0, -1, 0)                      # some of them against no row
    s, num = consensus_scores(last, frequency=f, groups=rows, return_numerators=True)
    assert np.array_equal(num, np.where(rows < 0, 0, ref["common"][100:, :100].astype(np.int64).sum(axis=1)))
    assert same_bits(s, R.scores_of(num, ref["n"][100:], np.where(rows < 0, 0, 100)))


# ---- 3 hand-packed words ---------------------------------------------------------------------------------------------------
def hand_maps(n_b, M, n_a=3):
    return np.random.default_rng(1000 * n_b + M).random((M, n_a, n_b)) < 0.5


def check_hand_packed(api, device, n_b, M):
    """random bits at density 0.5: one group of all poses, then the same with every tail bit set"""
    maps = hand_maps(n_b, M)
    order, ptr = one_group(M)
    row = np.zeros(M, dtype=np.int64)
    least = [max(1, M // 2)]
    clean = check_raw(api, device, maps, order, ptr, row, least, what=(n_b, M))
    dirty = check_raw(api, device, maps, order, ptr, row, least, tail=True, what=(n_b, M, "tail"))
    assert all(same_bits(x, y) for x, y in zip(clean, dirty))
    return clean


def check_all_ones(api, device, M, n_a=2, n_b=65):
    """all-ones bits: where a bit-sliced or narrow counter would wrap"""
    maps = np.ones((M, n_a, n_b), dtype=bool)
    order, ptr = one_group(M)
    counts, residues, num, bits, n = check_raw(api, device, maps, order, ptr, np.zeros(M, dtype=np.int64), [M], tail=True, what=M)
    assert (counts == M).all() and (residues == M).all() and (num == n_a * n_b * M).all() and n_a * n_b == 130
    assert list(n) == [n_a * n_b]


# ---- 4 groups ----------------------------------------------------------------------------------------------------------------
def check_groups(api, device):
    rng = np.random.default_rng(3)
    M, n_b = 70, 70
    maps = rng.random((M, 3, n_b)) < 0.3
    for G in (1, 2, 3, 4, 5):
        groups = rng.integers(0, G, size=M)
        order, ptr = R.lists_of(groups, G)
        check_raw(api, device, maps, order, ptr, groups, np.maximum(1, np.diff(ptr) // 2), what="G = %d" % G)
    # an empty group in the middle, a group of one, a pose in no group
    groups = rng.integers(0, 4, size=M)
    groups[groups == 1] = 3
    groups[:2] = (2, -1)
    groups[2:][groups[2:] == 2] = 0
    order, ptr = R.lists_of(groups, 4)
    assert list(np.diff(ptr))[1:3] == [0, 1] and (groups == -1).sum() == 1
    counts, residues, num, bits, n = check_raw(api, device, maps, order, ptr, groups, [3, 1, 1, 3], what="empty group")
    assert not counts[1].any() and not residues[1].any() and not bits[1].any() and n[1] == 0 and num[1] == 0
    assert np.array_equal(counts[2], maps[0].astype(np.int32)) and num[0] == maps[0].sum() and n[2] == maps[0].sum()
    # a pose listed in two groups, a pose listed twice in one (it counts twice), rows of another group and of none
    order = np.array([0, 1, 2, 2, 5, 1, 6, 7])
    ptr = np.array([0, 5, 8])
    row = rng.integers(-1, 2, size=M)
    counts, residues, num, bits, n = check_raw(api, device, maps, order, ptr, row, [2, 3], what="lists")
    assert np.array_equal(counts[0], maps[[0, 1, 2, 2, 5]].sum(axis=0)) and np.array_equal(counts[1], maps[[1, 6, 7]].sum(axis=0))
    assert (row == -1).any() and not num[row == -1].any() and num[row >= 0].all()
    # nA or nB of 0: residue rows of zeros, nothing else
    for shape in ((4, 0, 70), (4, 3, 0)):
        check_raw(api, device, np.zeros(shape, dtype=bool), np.arange(4), np.array([0, 4]), np.zeros(4, dtype=np.int64), [1])


def check_leave_one_out(api, device):
    """leave-one-out through consensus_scores: a group of one gives 0.0"""
    from deeprank_gnn_amd.interface import consensus_scores
    ref, c = family(), family_contacts(api, device).select(np.arange(17))
    assert np.array_equal(c.n_contacts, ref["n"][:17]) and np.array_equal(unpack(c.words(), c.n_b), ref["maps"][:17])
    groups = np.array([0, 0, 0, 1, 2, 2, -1, 0, 0, 2, 2, 0, 3, 3, 0, -1, 0])
    order, ptr = R.lists_of(groups, 4)
    counts = R.counts_of(ref["maps"][:17], order, ptr)
    num = R.numerators_of(ref["maps"][:17], counts, groups)
    N = np.where(groups >= 0, np.diff(ptr)[np.maximum(groups, 0)], 0)
    for loo in (False, True):
        s, got = consensus_scores(c, groups=groups, leave_one_out=loo, return_numerators=True)
        assert np.array_equal(got, num) and same_bits(s, R.scores_of(num, ref["n"][:17], N, leave_one_out=loo)), loo
    assert s[3] == 0.0 and ref["n"][3] > 0 and s[6] == 0.0 and (s[groups == 0] > 0).all()


# ---- 5 thresholds ------------------------------------------------------------------------------------------------------------
def check_thresholds(api, device):
    import torch
    from deeprank_gnn_amd.interface import consensus_bits_raw, consensus_contacts, contact_frequency
    # counts exactly at min_count are in, one below is out
    rng = np.random.default_rng(8)
    counts = rng.integers(0, 12, size=(3, 5, 129)).astype(np.int32)
    least = np.array([6, 1, 12])
    counts[0, :, ::7], counts[0, :, 1::7] = 6, 5
    bits, n = consensus_bits_raw(api, torch.from_numpy(counts).to(device), least)
    got = unpack(bits.cpu().numpy(), 129)
    assert np.array_equal(got, counts >= least[:, None, None]) and got[0, :, ::7].all() and not got[0, :, 1::7].any()
    assert np.array_equal(n.cpu().numpy(), (counts >= least[:, None, None]).reshape(3, -1).sum(axis=1)) and n.dtype == torch.int32
    assert not got[2].any() and np.array_equal(got[1], counts[1] > 0)
    # a fraction and the count it means give the same bits
    ref, c = family(), family_contacts(api, device)
    f = contact_frequency(c, groups=ref["labels"], n_groups=5)
    for frac in (0.5, 0.3, 1.0, 1e-9):
        least = R.min_count_of(frac, ref["sizes"])
        a, b = consensus_contacts(f, min_fraction=frac), consensus_contacts(f, min_count=least)
        assert same_bits(a.words(), b.words()) and same_bits(a.n_contacts, b.n_contacts)
        assert np.array_equal(unpack(a.words(), c.n_b), R.consensus_of(ref["c_counts"], least))
    assert same_bits(consensus_contacts(f, min_count=4).words(), consensus_contacts(f, min_count=np.full(5, 4)).words())
    assert list(R.min_count_of(1e-9, ref["sizes"])) == [1] * 5 and list(R.min_count_of(1.0, ref["sizes"])) == FAMILY_SIZES


# ---- 6 select ----------------------------------------------------------------------------------------------------------------
def check_select(api, device):
    from deeprank_gnn_amd.interface import AtomTable, cluster_poses, contact_frequency, interface_residues, pose_contacts
    c = family_contacts(api, device)
    table, xyz = F.family_batch()
    idx = np.array([5, 3, 77, 12, 100, 101, 40, 41, 42, 8, 9, 10, 129, 0, 64, 63, 65, 20, 21, 22, 23, 90, 91, 3])
    sub, alone = c.select(idx), pose_contacts(AtomTable.poses(table, xyz[idx]), **F.kw(api, device))
    assert len(sub) == len(idx) and same_bits(sub.words(), alone.words()) and same_bits(sub.n_contacts, alone.n_contacts)
    assert (sub.table, sub.cutoff, sub.heavy_only, sub.api) == (c.table, c.cutoff, c.heavy_only, c.api)
    for min_size in (2, 4):
        x, y = cluster_poses(sub, min_size=min_size), cluster_poses(alone, min_size=min_size)
        assert all(same_bits(getattr(x, k), getattr(y, k)) for k in ("labels", "centres", "sizes", "n_contacts"))
    assert len(x) >= 1 and len(c.select(np.zeros(0, dtype=np.int64))) == 0
    f = contact_frequency(c)
    for k in (1, 5, len(c)):
        assert same_bits(f.interface_residues(0, k), interface_residues(c, k)), k
    assert len(f.interface_residues(0, 1)) > len(f.interface_residues(0, 5)) > 0


# ---- 7 independence ----------------------------------------------------------------------------------------------------------
def all_outputs(c, groups, n_groups):
    """(counts, residues, numerators, scores, consensus words, n_contacts) of a PoseContacts, as numpy"""
    from deeprank_gnn_amd.interface import consensus_contacts, consensus_scores, contact_frequency
    f = contact_frequency(c, groups=groups, n_groups=n_groups)
    s, num = consensus_scores(c, groups=groups, return_numerators=True)
    cons = consensus_contacts(f, min_fraction=0.4)
    return f.counts.cpu().numpy(), f.residues.cpu().numpy(), num, s, cons.words(), cons.n_contacts


def check_independence(api, device, M=17):
    """place, run and the chunks the contacts came in change no bit.  Returns the outputs of the whole family batch"""
    from deeprank_gnn_amd.interface import AtomTable, pose_contacts
    ref, c = family(), family_contacts(api, device)
    base = all_outputs(c, ref["labels"], 5)
    assert all(same_bits(x, y) for x, y in zip(base, all_outputs(c, ref["labels"], 5)))          # two runs
    perm = np.random.default_rng(5).permutation(len(c))
    moved = all_outputs(c.select(perm), ref["labels"][perm], 5)
    for k in (0, 1, 4, 5):
        assert same_bits(moved[k], base[k]), k
    assert same_bits(moved[2], base[2][perm]) and same_bits(moved[3], base[3][perm])
    table, xyz = F.family_batch()
    groups = np.arange(M) % 3 - (np.arange(M) % 5 == 0)
    small = all_outputs(c.select(np.arange(M)), groups, 3)
    for chunk in (1, 5, M):
        again = pose_contacts(AtomTable.poses(table, xyz[:M]), chunk=chunk, **F.kw(api, device))
        assert all(same_bits(x, y) for x, y in zip(small, all_outputs(again, groups, 3))), chunk
    return base


# ---- 8 capacities, refusals, the empty batch, value errors ------------------------------------------------------------------
REQUESTS = {
    "counts": ("ContactCountsRequest", "pose_contact_counts", "drgnn_pose_contact_counts"),
    "numerators": ("ConsensusNumeratorsRequest", "pose_consensus_numerators", "drgnn_pose_consensus_numerators"),
    "bits": ("ConsensusBitsRequest", "pose_consensus_bits", "drgnn_pose_consensus_bits"),
}
GOOD_ORDER, GOOD_PTR, GOOD_ROW, GOOD_MIN = [0, 2, 3, 1, 4, 4], [0, 3, 3, 6], [0, 2, -1, 1, 2], [2, 1, 1]      # 5 poses, 3 groups


def refusal_cases():
    """(entry point, name) -> what to change in a good request; "tab_*": the host copy of a list"""
    cases = {("counts", "null " + k): {k: None} for k in ("bits", "order", "group_ptr", "host_order", "host_group_ptr", "counts", "residues")}
    cases.update({("counts", "%s negative" % k): {k: -1} for k in ("n_poses", "n_chain_a", "n_chain_b", "n_groups", "n_listed")})
    cases.update({("counts", k): v for k, v in {
        "group_ptr starts at 1": {"tab_group_ptr": [1, 3, 3, 6]}, "group_ptr decreases": {"tab_group_ptr": [0, 3, 2, 6]},
        "group_ptr ends before the list": {"tab_group_ptr": [0, 3, 3, 5]}, "group_ptr ends past the list": {"tab_group_ptr": [0, 3, 3, 7]},
        "n_listed is not where group_ptr ends": {"n_listed": 5},
        "order entry negative": {"tab_order": [0, 2, 3, 1, -1, 4]}, "order entry past the poses": {"tab_order": [0, 2, 5, 1, 4, 4]},
        "n_poses below an order entry": {"n_poses": 4},
    }.items()})
    cases.update({("numerators", "null " + k): {k: None} for k in ("bits", "counts", "row", "host_row", "numerators")})
    cases.update({("numerators", "%s negative" % k): {k: -1} for k in ("n_poses", "n_chain_a", "n_chain_b", "n_groups")})
    cases.update({("numerators", k): v for k, v in {
        "row entry below -1": {"tab_row": [0, 2, -2, 1, 2]}, "row entry past the groups": {"tab_row": [0, 3, -1, 1, 2]},
        "n_groups below a row entry": {"n_groups": 2},
    }.items()})
    cases.update({("bits", "null " + k): {k: None} for k in ("counts", "min_count", "host_min_count", "bits", "n_contacts")})
    cases.update({("bits", "%s negative" % k): {k: -1} for k in ("n_chain_a", "n_chain_b", "n_groups")})
    cases.update({("bits", k): v for k, v in {"min_count 0": {"tab_min_count": [2, 0, 1]}, "min_count negative": {"tab_min_count": [2, 1, -3]}}.items()})
    for entry in REQUESTS:
        cases[entry, "null request"] = None
        for what, over in capacity_refusals(entry).items():
            cases[entry, "capacity: " + what] = over
    return cases


def capacity_refusals(entry):
    """one beyond every documented capacity that entry point meets (the sizes are never touched: refused on the host)"""
    out = {"residues of a complex": {"n_chain_a": 3000, "n_chain_b": 73}, "groups": {"n_groups": 65536},
           "entries of counts": {"n_chain_a": 1536, "n_chain_b": 1536, "n_groups": 911}}
    if entry == "counts":
        out.update({"poses": {"n_poses": 2 ** 31}, "listed poses": {"n_listed": 2 ** 31}})
    if entry == "numerators":
        out["poses"] = {"n_poses": 4194304}
    return out


def refusal_names():
    return sorted("%s: %s" % k for k in refusal_cases())


def check_refusal(api, device, name):
    """one malformed field: refused on the host, before a launch (the outputs keep their fill); the good request then runs"""
    import pytest
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd._lib import DrgnnError
    entry, what = name.split(": ", 1)
    over = refusal_cases()[entry, what]
    dev = torch.device(device)
    up = lambda a, t=np.int32: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(dev)
    M, nA, nB, G = 5, 3, 70, 3
    maps = np.random.default_rng(12).random((M, nA, nB)) < 0.4
    want_counts, want_res = R.counts_of(maps, GOOD_ORDER, GOOD_PTR), R.residues_of(maps, GOOD_ORDER, GOOD_PTR)
    d_bits = up(pack(maps), np.int64)
    d_lists = {"order": up(GOOD_ORDER), "group_ptr": up(GOOD_PTR), "row": up(GOOD_ROW), "min_count": up(GOOD_MIN)}
    in_counts = up(want_counts)
    counts = torch.full((G, nA, nB), FILL, dtype=torch.int32, device=dev)
    residues = torch.full((G, nA + nB), FILL, dtype=torch.int32, device=dev)
    num = torch.full((M,), FILL, dtype=torch.int64, device=dev)
    out_bits = torch.full((G, nA, 2), FILL, dtype=torch.int64, device=dev)
    out_n = torch.full((G,), FILL, dtype=torch.int32, device=dev)
    outputs = {"counts": (counts, residues), "numerators": (num,), "bits": (out_bits, out_n)}[entry]
    keep = []

    def host(ch, key, good):
        a = np.ascontiguousarray(ch.pop("tab_" + key, good), dtype=np.int32)
        keep.append(a)
        return a.ctypes.data

    def request(**ch):
        q = getattr(_lib, REQUESTS[entry][0])()
        if entry == "counts":
            q.bits, q.order, q.group_ptr = d_bits.data_ptr(), d_lists["order"].data_ptr(), d_lists["group_ptr"].data_ptr()
            q.host_order, q.host_group_ptr = host(ch, "order", GOOD_ORDER), host(ch, "group_ptr", GOOD_PTR)
            q.n_poses, q.n_chain_a, q.n_chain_b, q.n_groups, q.n_listed = M, nA, nB, G, len(GOOD_ORDER)
            q.counts, q.residues = counts.data_ptr(), residues.data_ptr()
        elif entry == "numerators":
            q.bits, q.counts, q.row, q.host_row = d_bits.data_ptr(), in_counts.data_ptr(), d_lists["row"].data_ptr(), host(ch, "row", GOOD_ROW)
            q.n_poses, q.n_chain_a, q.n_chain_b, q.n_groups, q.numerators = M, nA, nB, G, num.data_ptr()
        else:
            q.counts, q.min_count, q.host_min_count = in_counts.data_ptr(), d_lists["min_count"].data_ptr(), host(ch, "min_count", GOOD_MIN)
            q.n_chain_a, q.n_chain_b, q.n_groups, q.bits, q.n_contacts = nA, nB, G, out_bits.data_ptr(), out_n.data_ptr()
        for key, v in ch.items():
            setattr(q, key, v)
        return q

    call = getattr(api, REQUESTS[entry][1])
    stream = _lib.current_stream(d_bits)
    if what == "null request":
        with pytest.raises(DrgnnError, match="bad argument"):
            _lib._check(getattr(api.lib, REQUESTS[entry][2])(None, stream), REQUESTS[entry][2])
    else:
        with pytest.raises(DrgnnError, match="capacity" if what.startswith("capacity") else "bad argument"):
            call(request(**dict(over)), stream)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert all(bool((o == FILL).all()) for o in outputs)              # nothing was launched
    call(request(), stream)                                           # and the good request runs, whatever the outputs held
    if entry == "counts":
        assert np.array_equal(counts.cpu().numpy(), want_counts) and np.array_equal(residues.cpu().numpy(), want_res)
    elif entry == "numerators":
        assert np.array_equal(num.cpu().numpy(), R.numerators_of(maps, want_counts, GOOD_ROW))
    else:
        want = R.consensus_of(want_counts, GOOD_MIN)
        assert np.array_equal(unpack(out_bits.cpu().numpy(), nB), want)
        assert np.array_equal(out_n.cpu().numpy(), want.reshape(G, -1).sum(axis=1))


def check_capacity(api, device):
    """at each documented capacity that needs no large allocation the call is served and right; one beyond is refused"""
    import pytest
    import torch
    from deeprank_gnn_amd._lib import DrgnnError
    from deeprank_gnn_amd.interface import consensus_bits_raw, consensus_numerators_raw, contact_counts_raw
    rcap, gcap, ecap, ncap, pcap = (api.consensus_capacity(k) for k in range(5))
    assert rcap == api.fcc_capacity(0) and gcap == 65535 and ecap == pcap == 2 ** 31 - 1 and ncap == 4194303
    assert api.consensus_capacity(5) == -1 and api.consensus_capacity(-1) == -1
    # residues of a complex: the last residue of either chain is in contact in one pose of two
    nA, nB = rcap - 65, 65
    maps = np.zeros((2, nA, nB), dtype=bool)
    maps[0, nA - 1, nB - 1] = maps[0, 0, 0] = maps[1, 0, 0] = True
    counts, residues, num, bits, n = check_raw(api, device, maps, *one_group(2), np.zeros(2, dtype=np.int64), [2], tail=True)
    assert counts[0, nA - 1, nB - 1] == 1 and counts[0, 0, 0] == 2 and list(num) == [3, 2] and list(n) == [1]
    assert residues[0, nA - 1] == 1 and residues[0, nA + nB - 1] == 1 and residues[0, 0] == 2 and residues.sum() == 6
    words = torch.zeros((2, nA + 1, 2), dtype=torch.int64, device=device)
    with pytest.raises(DrgnnError, match="capacity"):
        contact_counts_raw(api, words, nB, *one_group(2))
    # groups of one call: every second group lists pose 1, the last one both poses
    maps = np.array([[[True]], [[True]], [[True]]])
    ptr = np.concatenate(([0], np.cumsum(np.arange(gcap) % 2))).astype(np.int64)
    ptr[-1] += 2
    order = np.concatenate((np.full(ptr[-1] - 2, 2), [0, 1]))
    d = torch.from_numpy(pack(maps)).to(device)
    counts, residues = contact_counts_raw(api, d, 1, order, ptr)
    want = (np.arange(gcap) % 2).astype(np.int32)
    want[-1] = 2
    assert np.array_equal(counts.cpu().numpy().reshape(-1), want) and np.array_equal(residues.cpu().numpy(), np.stack((want, want), axis=1))
    bits, n = consensus_bits_raw(api, counts, np.full(gcap, 2))
    assert np.array_equal(n.cpu().numpy(), want // 2) and np.array_equal(bits.cpu().numpy().reshape(-1), want // 2)
    with pytest.raises(DrgnnError, match="capacity"):
        contact_counts_raw(api, d, 1, np.zeros(0, dtype=np.int64), np.zeros(gcap + 2, dtype=np.int64))
    with pytest.raises(DrgnnError, match="capacity"):
        consensus_bits_raw(api, torch.zeros((gcap + 1, 1, 1), dtype=torch.int32, device=device), np.ones(gcap + 1))
    # poses of one numerator call
    d = torch.zeros((ncap + 1, 1, 1), dtype=torch.int64, device=device)
    d[::2] = 1
    d[-2:] = 1
    c1 = torch.full((2, 1, 1), 7, dtype=torch.int32, device=device)
    row = np.arange(ncap + 1) % 3 - 1
    num = consensus_numerators_raw(api, d[:ncap], 1, c1, row[:ncap]).cpu().numpy()
    assert np.array_equal(num, np.where((row[:ncap] >= 0) & (d[:ncap, 0, 0].cpu().numpy() != 0), 7, 0)) and num[-1] == 7
    with pytest.raises(DrgnnError, match="capacity"):
        consensus_numerators_raw(api, d, 1, c1, row)


def check_scores_are_split(api, device, monkeypatch):
    """consensus_scores splits its calls at the capacity: the same numerators through calls of at most 7 poses"""
    from deeprank_gnn_amd.interface import consensus_scores
    ref, c = family(), family_contacts(api, device)
    whole = consensus_scores(c, groups=ref["labels"], return_numerators=True)
    monkeypatch.setattr(type(api), "consensus_capacity", lambda self, what: 7 if what == 3 else 2 ** 31 - 1)
    again = consensus_scores(c, groups=ref["labels"], return_numerators=True)
    assert same_bits(whole[0], again[0]) and same_bits(whole[1], again[1])


def check_empty_batch(api, device):
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd.interface import (consensus_bits_raw, consensus_contacts, consensus_numerators_raw, consensus_scores,
                                            contact_counts_raw, contact_frequency)
    c = family_contacts(api, device)
    none = c.select(np.zeros(0, dtype=np.int64))
    f = contact_frequency(none)                                        # one group without poses: rows of zeros
    assert len(f) == 1 and list(f.n_poses) == [0] and f.counts.shape == (1, c.n_a, c.n_b) and not f.counts.any() and not f.residues.any()
    assert not f.fraction().any() and not f.residue_fraction().any() and f.pairs().shape == (0, 3) and f.interface_residues().shape == (0,)
    s, num = consensus_scores(none, return_numerators=True)
    assert s.shape == (0,) and s.dtype == np.float64 and num.shape == (0,) and num.dtype == np.int64
    cons = consensus_contacts(f)
    assert len(cons) == 1 and list(cons.n_contacts) == [0] and not cons.words().any()
    assert not consensus_scores(c, frequency=f).any()                  # scored against a set of no poses: 0.0
    g0 = contact_frequency(none, groups=np.zeros(0, dtype=np.int64))    # no groups at all
    assert len(g0) == 0 and g0.counts.shape == (0, c.n_a, c.n_b) and g0.residues.shape == (0, c.n_a + c.n_b) and len(consensus_contacts(g0)) == 0
    # no groups, no poses: served without a launch (the entry points of a null stream and null arrays)
    for entry, fields in (("counts", {"n_poses": 9, "n_chain_a": 3, "n_chain_b": 70, "host_group_ptr": "zero"}),
                          ("numerators", {"n_chain_a": 3, "n_chain_b": 70, "n_groups": 2}), ("bits", {"n_chain_a": 3, "n_chain_b": 70})):
        q = getattr(_lib, REQUESTS[entry][0])()
        zero = np.zeros(1, dtype=np.int32)
        for k, v in fields.items():
            setattr(q, k, zero.ctypes.data if v == "zero" else v)
        if entry == "counts":
            q.group_ptr = zero.ctypes.data                             # (never read: there is no group)
        assert getattr(api.lib, REQUESTS[entry][2])(q, None) == 0, entry


def fake_contacts(M, n_a=3, n_b=70, api=None):
    """a PoseContacts that no library ever saw"""
    import torch
    from deeprank_gnn_amd.interface import PoseContacts

    class Table(object):
        split, n_residues = n_a, n_a + n_b

    return PoseContacts(Table(), torch.zeros((M, n_a, (n_b + 63) // 64), dtype=torch.int64), np.zeros(M, dtype=np.int64), api or object(),
                        "cpu", 5.0, True)


def check_value_errors():
    """the Python side refuses before anything is launched (api=object() would fail at the first call)"""
    import pytest
    import torch
    from deeprank_gnn_amd.interface import (ContactFrequency, PoseClusters, consensus_contacts, consensus_scores, contact_frequency)
    api = object()
    c = fake_contacts(6, api=api)
    f = ContactFrequency(c, torch.zeros((2, 3, 70), dtype=torch.int32), torch.zeros((2, 73), dtype=torch.int32), np.array([4, 2]))
    for bad in (np.zeros(5, dtype=np.int64), np.zeros(7, dtype=np.int64), np.zeros((6, 1), dtype=np.int64)):
        with pytest.raises(ValueError, match="groups for 6 poses"):
            contact_frequency(c, groups=bad)
        with pytest.raises(ValueError, match="groups for 6 poses"):
            consensus_scores(c, groups=bad)
        with pytest.raises(ValueError, match="groups for 6 poses"):
            consensus_scores(c, frequency=f, groups=bad)
    for bad, G in (([0, 0, -2, 0, 0, 0], None), ([0, 1, 2, 0, 0, 0], 2), ([0, 0, 0, 0, 0, 5], 5)):
        with pytest.raises(ValueError, match="must lie in"):
            contact_frequency(c, groups=np.array(bad), n_groups=G)
    with pytest.raises(ValueError, match="must lie in"):
        consensus_scores(c, frequency=f, groups=np.array([0, 1, 2, 0, 0, 0]))
    with pytest.raises(ValueError, match="integers"):
        contact_frequency(c, groups=np.zeros(6))
    with pytest.raises(ValueError, match="n_groups"):
        contact_frequency(c, n_groups=-1)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_fraction"):
            consensus_contacts(f, min_fraction=bad)
    for bad in (0, -1, 2.5, [1, 2, 3], [1, 0]):
        with pytest.raises(ValueError, match="min_count"):
            consensus_contacts(f, min_count=np.asarray(bad))
    with pytest.raises(ValueError, match="leave_one_out"):
        consensus_scores(c, frequency=f, leave_one_out=True)
    for other in (fake_contacts(6, n_b=71, api=api), fake_contacts(6, n_a=4, api=api), fake_contacts(6)):      # topology, library
        with pytest.raises(ValueError, match="one topology, library and device"):
            consensus_scores(other, frequency=f)
    for thing in (contact_frequency, consensus_scores, consensus_contacts):
        with pytest.raises(ValueError, match="PoseContacts|ContactFrequency"):
            thing(np.zeros((6, 3, 2)))
    with pytest.raises(ValueError, match="ContactFrequency"):
        consensus_scores(c, frequency=c)
    clusters = PoseClusters(np.zeros(5, dtype=np.int64), np.zeros(1, dtype=np.int64), np.full(1, 5), np.zeros(5, dtype=np.int64))
    with pytest.raises(ValueError, match="6 poses for 5 labels"):
        clusters.consensus(c)
    with pytest.raises(ValueError, match="PoseContacts"):
        clusters.consensus(np.zeros(5))
    for bad in (np.array([0, 6]), np.array([-1]), np.array([True, False]), np.zeros((2, 2), dtype=np.int64), np.array([0.5])):
        with pytest.raises(ValueError, match="index"):
            c.select(bad)
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="group"):
            f.fraction(bad)
    with pytest.raises(ValueError, match="min_count"):
        f.pairs(0, min_count=0)
    with pytest.raises(ValueError, match="min_poses"):
        f.interface_residues(0, min_poses=0)


# ---- 9 the device against the emulation --------------------------------------------------------------------------------------
def assert_same_results(x, y):
    """two tuples of arrays (the device's and the emulation's), exactly"""
    assert len(x) == len(y) and all(same_bits(u, v) for u, v in zip(x, y))
