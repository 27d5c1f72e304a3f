"""Inputs and checks shared by tests/test_louvain.py (host emulation) and tests/test_gpu_louvain.py (the device) for
the deterministic Louvain (csrc/drgnn_louvain.h) beyond the committed fixture.

A case is (name, pairs, n) as in louvain_ref: `pairs` are LOCAL node ids as the edge slice lists them -- raw: any
direction, repetition, order, self-loops, and ends outside [0, n), which in a batch point into a neighbour's node range
or below node_ptr[g] and which the kernel has to drop.

    raw_cases()        the level-0 input handling, straight into api.louvain (raw_louvain), no _distinct_pairs
    threshold_cases()  graphs on which lv_below decides: the gain of a pass or of a level next to 1e-7 (2m)^2
    lane_cases()       node counts, row lengths and community counts on the edges of the 64 lanes
    tiny_cases()       graphs of at most 9 nodes whose best partition is found by enumeration

No expectation here comes from the code under test: they come from louvain_ref (R.louvain, with its trace for the
intermediate state), from exact rational arithmetic on the returned labels (check_invariants), from the enumeration of
all set partitions (best_partition_N), and, for the threshold graphs, from the arithmetic written next to them.
"""
import functools
from fractions import Fraction

import numpy as np
import torch

import louvain_ref as R

LDS_LIMIT = 160 * 1024          # DRGNN_LDS_LIMIT
FILL = -7                       # what raw_louvain puts into labels before the launch


def lds_bytes(cap_n, cap_e):
    """louvain_lds_words (csrc/drgnn_louvain.h) in bytes"""
    return 4 * (3 * 64 + 4 + 6 * cap_n + 3 + 8 * max(cap_e, 1))


def clean(pairs, n):
    """the distinct (min, max) pairs of a raw list with both ends inside [0, n)"""
    return sorted({(min(int(u), int(v)), max(int(u), int(v))) for u, v in pairs
                   if 0 <= int(u) < n and 0 <= int(v) < n})


_REFERENCE = {}


def reference(case):
    """R.louvain of a case on its cleaned list, computed once per case name and left unchanged"""
    name, pairs, n = case
    key = (name, n, np.asarray(pairs, dtype=np.int64).tobytes())
    if key not in _REFERENCE:
        _REFERENCE[key] = R.louvain(clean(pairs, n), n)
    return _REFERENCE[key]


# ---- the two ways into the kernel ------------------------------------------------------------------------------------
def raw_louvain(ei, nptr, eptr, api, cap_n=None, cap_e=None, fill=FILL):
    """api.louvain on the edge list as it is (no _distinct_pairs).  The caps default to the largest raw slice.
    Tensors on the CPU go to the emulation library, tensors on the device to the product library.
    Returns numpy (labels, info, modularity); labels hold `fill` wherever the kernel wrote nothing."""
    from deeprank_gnn_amd import _lib
    dev = nptr.device
    B = nptr.numel() - 1
    n_nodes = int(nptr[-1])
    if cap_n is None:
        cap_n = int((nptr[1:] - nptr[:-1]).max())
    if cap_e is None:
        cap_e = int((eptr[1:] - eptr[:-1]).max())
    ei = ei.to(torch.int64).contiguous()
    labels = torch.full((max(n_nodes, 1),), fill, dtype=torch.int64, device=dev)
    info = torch.full((B, 2), 99, dtype=torch.int32, device=dev)
    q = torch.full((B,), -1.0, dtype=torch.float64, device=dev)
    api.louvain(ei, ei.size(1), nptr.contiguous(), eptr.contiguous(), B, cap_n, cap_e, labels, info, q,
                _lib.current_stream(labels))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return labels[:n_nodes].cpu().numpy(), info.cpu().numpy(), q.cpu().numpy()


def labelled(cases, api, device="cpu"):
    """clustering.louvain_labels on the batch of `cases`, numpy (labels, info, modularity)"""
    from deeprank_gnn_amd.clustering import louvain_labels
    ei, nptr, eptr = (t.to(device) for t in R.batch_of(cases))
    labels, info, q = louvain_labels(ei, nptr, eptr, api=api)
    if device != "cpu":
        torch.cuda.synchronize()
    return labels.cpu().numpy(), info.cpu().numpy(), q.cpu().numpy()


def raw(cases, api, device="cpu", **kw):
    return raw_louvain(*(t.to(device) for t in R.batch_of(cases)), api=api, **kw)


def bits(x):
    return np.asarray([x], dtype=np.float64).view(np.int64)[0]


def check_case(case, labels, info, q):
    """one graph's result against the reference and against what does not restate the algorithm"""
    name, pairs, n = case
    lab, inf, mod = reference(case)
    np.testing.assert_array_equal(labels, lab, err_msg=name)
    assert tuple(int(x) for x in info) == inf, (name, tuple(info), inf)
    assert bits(q) == bits(mod), (name, q, mod)
    check_invariants(case, labels, q)


def check_batch(cases, got, skip=()):
    """`got` = (labels, info, modularity) of the batch of `cases`; `skip`: indices checked by the caller"""
    labels, info, q = got
    off = 0
    for g, case in enumerate(cases):
        n = case[2]
        if g not in skip:
            check_case(case, labels[off:off + n], info[g], q[g])
        off += n
    assert off == len(labels)


# ---- checks that do not restate the algorithm ------------------------------------------------------------------------
def exact_modularity(pairs, n, labels):
    """Q of `labels` on the cleaned pairs as a Fraction: sum_c (2m A_c - K_c^2) / (2m)^2, A[u][u] = 2 per self-loop"""
    deg = [0] * n
    inside = 0
    for u, v in clean(pairs, n):
        w = 2 if u == v else 1
        deg[u] += w
        deg[v] += 0 if u == v else w
        if labels[u] == labels[v]:
            inside += 2
    two_m = sum(deg)
    if two_m == 0:
        return Fraction(0)
    K = {}
    for u in range(n):
        K[labels[u]] = K.get(labels[u], 0) + deg[u]
    return Fraction(two_m * inside - sum(k * k for k in K.values()), two_m * two_m)


def check_invariants(case, labels, q):
    """The modularity is the correctly rounded exact value of the returned partition (the kernel divides two exact
    integers below 2^53 once, so no tolerance); labels are consecutive in order of first appearance; every community
    induces a connected subgraph; isolated nodes are singletons."""
    name, pairs, n = case
    labels = [int(x) for x in labels]
    assert bits(q) == bits(float(exact_modularity(pairs, n, labels))), (name, q)
    first = list(dict.fromkeys(labels))
    assert first == list(range(len(first))), name
    adj = [set() for _ in range(n)]
    for u, v in clean(pairs, n):
        if u != v:
            adj[u].add(v)
            adj[v].add(u)
    members = {}
    for u, c in enumerate(labels):
        members.setdefault(c, []).append(u)
    for c, nodes in members.items():
        if not adj[nodes[0]]:
            assert len(nodes) == 1, (name, "isolated node in a community", nodes)
        seen, todo = {nodes[0]}, [nodes[0]]
        while todo:
            for v in adj[todo.pop()]:
                if labels[v] == c and v not in seen:
                    seen.add(v)
                    todo.append(v)
        assert len(seen) == len(nodes), (name, "community %d is not connected" % c)


def best_partition_N(pairs, n):
    """max over ALL set partitions of N(P) = sum_c (2m A_c - K_c^2), and 2m: exact integers, by enumeration of the
    restricted growth strings with N kept up to date (n <= 9: at most 21 147 partitions)."""
    assert n <= 9
    A = [[0] * n for _ in range(n)]
    for u, v in clean(pairs, n):
        A[u][v] += 2 if u == v else 1
        if u != v:
            A[v][u] += 1
    deg = [sum(row) for row in A]
    two_m = sum(deg)
    block = [0] * n
    K = [0] * n
    best = [None]

    def place(i, used, cur):
        if i == n:
            if best[0] is None or cur > best[0]:
                best[0] = cur
            return
        for b in range(used + 1):
            link = A[i][i] + 2 * sum(A[i][j] for j in range(i) if block[j] == b)
            gain = two_m * link - (2 * K[b] + deg[i]) * deg[i]
            block[i] = b
            K[b] += deg[i]
            place(i + 1, max(used, b + 1), cur + gain)
            K[b] -= deg[i]

    place(0, 0, 0)
    return best[0], two_m


# ---- graph makers ----------------------------------------------------------------------------------------------------
def clique(nodes):
    nodes = list(nodes)
    return [(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:]]


def both_directions(pairs):
    return list(pairs) + [(v, u) for u, v in pairs]


def modular_graph(n, seed, block=16, cross=0.15):
    """(pairs, n): about 3 n distinct random pairs (all C(n, 2) when that is fewer), inside blocks of `block`
    consecutive nodes except for a share `cross`; one direction, (min, max), sorted"""
    rng = np.random.default_rng(seed)
    want = min(3 * n, n * (n - 1) // 2)
    pairs = set()
    while len(pairs) < want:
        u, v = (int(x) for x in rng.integers(0, n, size=2))
        if u != v and (u // block == v // block or rng.random() < cross):
            pairs.add((min(u, v), max(u, v)))
    return sorted(pairs), n


def blocks(sizes, bridges=(), loose_edges=0):
    """(pairs, n, first node of every block): disjoint cliques of `sizes`, laid out one after the other, the
    `bridges` (block a, member i, block b, member j), then `loose_edges` disjoint edges on nodes of their own"""
    pairs, start, n = [], [], 0
    for s in sizes:
        start.append(n)
        pairs += clique(range(n, n + s))
        n += s
    pairs += [(start[a] + i, start[b] + j) for a, i, b, j in bridges]
    for _ in range(loose_edges):
        pairs.append((n, n + 1))
        n += 2
    return pairs, n, start


# ---- A: raw edge lists -----------------------------------------------------------------------------------------------
def raw_cases():
    """[(name, raw pairs, n)], n <= 140: what the header of drgnn_louvain.h promises to take at level 0"""
    name, both, n = R.fixture_pairs()[0]
    both = np.asarray(both, dtype=np.int64)
    one = both[: len(both) // 2]
    rng = np.random.default_rng(20)
    mixed = one.copy()
    mixed[::3] = mixed[::3, ::-1]                                  # (max, min) on every third entry
    triple = np.vstack((one, one[::-1, ::-1], mixed))[rng.permutation(3 * len(one))]
    ring = [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 5), (5, 3)]
    foreign = np.vstack((mixed, [(-3, 2), (n + 1, 4), (5, n), (-1, -2), (n, n), (0, -1), (2 * n, 1), (7, -n)]))
    return [
        ("raw_both_directions", both, n),
        ("raw_shuffled", both[rng.permutation(len(both))], n),
        ("raw_one_direction_mixed", mixed, n),
        ("raw_three_times", triple, n),
        ("raw_loop_once", ring[:3] + [(2, 2)] + ring[3:], 6),
        ("raw_loop_three_times", [(2, 2)] + ring[:3] + [(2, 2)] + ring[3:] + [(2, 2)], 6),
        ("raw_pair_and_loop_in_one_row", [(0, 1), (1, 1), (1, 0), (1, 2), (1, 1), (2, 1)], 3),
        ("raw_ends_outside", foreign[rng.permutation(len(foreign))], n),
        ("raw_nothing_inside", [(-1, 2), (5, 0), (8, -2), (-4, -4), (6, 6)], 5),
    ]


def refusal_batch():
    """three graphs, the middle one the largest in nodes and in entries"""
    cases = raw_cases()
    return [cases[4], cases[1], cases[6]]


# ---- B: the threshold decides ----------------------------------------------------------------------------------------
# A K8 and a K12 joined by one edge are two communities after level 0, of degree sums 8*7 + 1 = 57 and 12*11 + 1 = 133.
# Merging two communities a, b joined by w edges changes N = sum_c (2m A_c - K_c^2) by 2 (2m w - K_a K_b); here by
# 2 (2m - 7581).  The threshold is 1e-7 (2m)^2: 5.7487 at 2m = 7582.
#
# What no graph within the kernel's capacity can show: N is always even (2m, A_c and sum K_c^2 are), so a gain meets the
# threshold only where 1e-7 (2m)^2 is an even integer, which needs 2m = 10 000 k.  Over every even 2m the 160 KiB carve
# admits (2m <= 10 038) the threshold otherwise stays 8.6e-6 (relative) or more away from an even integer (6.0000516 at
# 2m = 7746), far beyond the error of an fp32 product.  So `<=` in place of `<`, or the product formed in fp32, decides
# differently from the kernel at 2m = 10 000 alone: 5 000 pairs on at most 126 nodes (6 n + 8 E <= 40 761 words) with a
# pass or a level that gains exactly 10.  One merge cannot (10 000 w - 5 = K_a K_b has no factorisation with degree sums
# that fit next to a filler of 4 500 pairs on the remaining nodes for w <= 4), several merges leave the filler too few
# nodes; no such graph was found.
def threshold_cases():
    """[(name, pairs listed once, n)]
    thr_below     2m = 7582: the one merge of level 1 gains 2 < 5.7487: the pass ends on the threshold with one node moved
                  (no further pass: 4 passes, not 5) and the level is not recorded: (1, 4), 58 communities, 0 and 8 apart.
    thr_above     one more loose edge, 2m = 7584: the merge gains 6 > 5.7517: (2, 6), 0 and 8 together.
    thr_sum       2m = 7582 again, three bridged pairs: each merge gains 2, below the threshold, the pass gains 6, above
                  it: the threshold is held against the pass and the level, not against a move: (2, 6).
    thr_two_sites 2m = 4682, threshold 2.1921.  K6 = X, K8 = A, K10 = B, X - A one edge, A - B two: K_X = 31, K_A = 59,
                  K_B = 92.  Level 1, pass 1: X joins A (2m - K_X K_A = 2853 > 0), A leaves for B
                  (2 * 2m - K_A K_B = 3936 > 2853), the pass gains 2 * 3936 = 7872.  Pass 2: X follows,
                  2m - K_X (K_A + K_B) = 1, a gain of 2 < 2.1921 with one node moved: the pass site ends the level after
                  2 passes (3 without it) while the record site records it (7874 above the threshold): (2, 6)."""
    one = (0, 0, 1, 0)
    return [
        ("thr_below",) + blocks([8, 12] + [12] * 56, [one])[:2],
        ("thr_above",) + blocks([8, 12] + [12] * 56, [one], loose_edges=1)[:2],
        ("thr_sum",) + blocks([8, 12] * 3 + [13] * 44 + [12, 4], [one, (2, 0, 3, 0), (4, 0, 5, 0)], loose_edges=2)[:2],
        ("thr_two_sites",) + blocks([6, 8, 10] + [13] * 28 + [12], [one, (1, 1, 2, 0), (1, 2, 2, 1)])[:2],
    ]


# what the reference returned for them when they were built, and what the arithmetic above says it must
THRESHOLD_EXPECTED = {
    "thr_below": dict(n=692, pairs=3791, info=(1, 4), communities=58, together=[], apart=[(0, 8)]),
    "thr_above": dict(n=694, pairs=3792, info=(2, 6), communities=58, together=[(0, 8)], apart=[]),
    "thr_sum": dict(n=652, pairs=3791, info=(2, 6), communities=51, together=[(0, 8), (20, 28), (40, 48)],
                    apart=[(0, 20), (20, 40)]),
    "thr_two_sites": dict(n=400, pairs=2341, info=(2, 6), communities=30, together=[(0, 6), (6, 14)], apart=[(0, 24)]),
}


def check_threshold_expectations(case, labels, info):
    want = THRESHOLD_EXPECTED[case[0]]
    assert (case[2], len(case[1])) == (want["n"], want["pairs"])
    assert tuple(int(x) for x in info) == want["info"], (case[0], tuple(info))
    assert len(set(labels.tolist())) == want["communities"], case[0]
    for u, v in want["together"]:
        assert labels[u] == labels[v], (case[0], u, v)
    for u, v in want["apart"]:
        assert labels[u] != labels[v], (case[0], u, v)


# ---- C: lane and chunk edges -----------------------------------------------------------------------------------------
LANE_NODE_COUNTS = (63, 64, 65, 127, 128, 129)
HUB_DEGREES = (63, 64, 65, 128, 129)
COMMUNITY_COUNTS = (63, 64, 65)


def hub_graph(degree, seed, n0=128, size=16):
    """(pairs, n, first node of every tied clique, hub): a modular graph on n0 nodes, then t = (degree - 8) // size
    disjoint cliques of `size` nodes, then the hub, the last node: linked to every node of every clique and to
    degree - t * size nodes of the modular part, which come first in its row.  When the hub is first visited the t
    cliques are t communities of equal degree sum and equal link count, and they attain its best score."""
    t = (degree - 8) // size
    pairs = list(modular_graph(n0, seed)[0])
    n, first = n0, []
    for _ in range(t):
        pairs += clique(range(n, n + size))
        first.append(n)
        n += size
    rng = np.random.default_rng(seed + 1000)
    pairs += [(int(o), n) for o in sorted(rng.permutation(n0)[: degree - t * size])]
    for c in first:
        pairs += [(c + j, n) for j in range(size)]
    return pairs, n + 1, first, n


def triangles(k, stragglers):
    """(pairs, n): k - stragglers disjoint triangles with `stragglers` isolated nodes between them: k communities"""
    pairs, n = [], 0
    for c in range(k - stragglers):
        if c % 7 == 3 and c // 7 < stragglers:
            n += 1
        pairs += clique(range(n, n + 3))
        n += 3
    return pairs, n


def long_induced_row():
    """(pairs, n): 70 K5, then a K10 every node of which has one edge to 7 of them, then 25 K13.  The K5 (degree sum
    21, formed first) outweigh a K10 node (degree 16), so the K10 stays one community: the last of 71 + 25 nodes of level
    1, its row 70 neighbours and itself, summed from 160 staged entries.  2m = 5530: the first five K5 join it at level
    1 (5530 > 21 * (160 + 21 j) for j < 5)."""
    return blocks([5] * 70 + [10] + [13] * 25, [(70, i % 10, i, 0) for i in range(70)])[:2]


def lane_cases():
    out = [("modular%d" % n,) + modular_graph(n, seed=n) for n in LANE_NODE_COUNTS]
    out += [("hub%d" % d,) + hub_graph(d, seed=d)[:2] for d in HUB_DEGREES]
    out += [("communities%d" % k,) + triangles(k, k - 60) for k in COMMUNITY_COUNTS]
    out.append(("long_induced_row",) + long_induced_row())
    return out


def check_lane_cases_sit_on_their_edges():
    """from the reference's intermediate state: the cases are where their names say"""
    for d in HUB_DEGREES:
        pairs, n, first, hub = hub_graph(d, seed=d)
        assert sum(1 for u, v in pairs if hub in (u, v)) == d and hub == n - 1
        trace = []
        labels = R.louvain(pairs, n, trace=trace)[0]
        tied = trace[0]["ties"][(0, hub)]                    # its first visit: the last of pass 0 of level 0
        assert len(tied) >= 3 and len(tied) == len(first), (d, tied)
        row = [u for u, v in pairs if v == hub]
        assert labels[row[0]] != labels[first[0]]            # the smallest tied community is not the first neighbour
        assert labels[hub] == labels[first[0]] and all(labels[hub] != labels[c] for c in first[1:]), d
    for k in COMMUNITY_COUNTS:
        pairs, n = triangles(k, k - 60)
        trace = []
        labels, info, _ = R.louvain(pairs, n, trace=trace)
        assert max(labels) + 1 == k and info[0] == 1 and trace[1]["nodes"] == k
    for n in LANE_NODE_COUNTS:
        assert 2 <= R.louvain(*modular_graph(n, seed=n))[1][0] <= 3
    trace = []
    pairs, n = long_induced_row()
    R.louvain(pairs, n, trace=trace)
    assert trace[1]["recorded"] and trace[1]["longest_row"] == 71 and trace[1]["passes"][0][0] == 5, trace[1]


# ---- D: graphs small enough to enumerate -----------------------------------------------------------------------------
def tiny_cases():
    """[(name, pairs, n)], n <= 9"""
    rng = np.random.default_rng(5)
    special = {c[0]: c for c in R.special_cases()}
    out = [
        special["toy6"],
        special["isolated_nodes"],
        special["self_loop"],
        special["K8"],
        ("two_triangles",) + blocks([3, 3])[:2],
        ("two_K4",) + blocks([4, 4])[:2],
        ("three_triangles",) + blocks([3, 3, 3])[:2],
        ("K4_K3_edge",) + blocks([4, 3], loose_edges=1)[:2],
        ("path_of_triangles",) + blocks([3, 3, 3], [(0, 2, 1, 0), (1, 2, 2, 0)])[:2],
        ("barbell_K4",) + blocks([4, 4], [(0, 3, 1, 0)])[:2],
        ("path8", [(i, i + 1) for i in range(7)], 8),
        ("cycle9", [(i, (i + 1) % 9) for i in range(9)], 9),
        ("star9", [(0, i) for i in range(1, 9)], 9),
    ]
    for k in range(3):
        pairs = {tuple(sorted(int(x) for x in rng.choice(9, size=2, replace=False))) for _ in range(14)}
        out.append(("random9_%d" % k, sorted(pairs), 9))
    return out


# the graphs on which Louvain must reach the best partition: chosen with the reference (R.louvain's N equals
# best_partition_N on them), before the kernel was run on any of them
REACHES_THE_MAXIMUM = ("toy6", "two_triangles", "two_K4", "three_triangles", "K4_K3_edge", "path_of_triangles",
                       "barbell_K4", "K8")


@functools.lru_cache(maxsize=None)
def tiny_maxima():
    """{name: (max N over all set partitions, 2m)}"""
    return {name: best_partition_N(pairs, n) for name, pairs, n in tiny_cases()}

