"""Inputs, reference and robustness filter shared by tests/test_mcl.py (host-emulation build) and
tests/test_gpu_mcl.py (MI355X) for the Markov clustering kernel (deeprank-gnn_amd/csrc/drgnn_mcl.h).

Reference: oracle/mcl_ref.py (labels and iteration count).  MCL is NOT a stable function of its input: on
symmetric graphs (cycles, some paths and grids) two columns carry mathematically equal values, rounding
breaks the tie, and the pruning / arg-max / convergence decisions -- hence the labels and the iteration
count -- follow the rounding.  A kernel that sums in another order, or contracts a * b + c into an FMA, may
then legitimately differ from the oracle.  So a case is compared exactly only if it is ROBUST: three
restatements of the algorithm, computed here from the reference alone (the code under test is never
consulted), agree on labels AND iteration count:

    (a) fp64: oracle.mcl_ref itself (BLAS product);
    (b) numpy.longdouble (x87 80-bit), for graphs of at most 150 nodes;
    (c) fp64 with a seeded relative perturbation of up to +-4 ulp on every entry of the expansion product
        before inflation (what another summation order or FMA contraction does to it).

Everything is generated from fixed seeds; nothing is read from disk except the committed fixture.
"""
import functools

import numpy as np

import louvain_ref as R
from oracle import mcl_ref

LONGDOUBLE_MAX_NODES = 150
ITERATIONS = 100          # fixed in the C entry point (drgnn_mcl)
PRUNE = 1e-3

# named cases that are NOT compared with the reference: deliberately symmetric inputs on which the three
# restatements disagree (see the module docstring).  Every other named case must pass the filter.
SYMMETRIC = ("cycle8", "cycle11")


# ---- reference and its restatements ------------------------------------------------------------------------
def adjacency(pairs, n):
    """dense 0/1 adjacency of (pairs, n): undirected, duplicates merged.  Every entry must lie inside the graph."""
    adj = np.zeros((n, n), dtype=np.float64)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(p):
        assert p.min() >= 0 and p.max() < n, "entry outside the graph: pass the cleaned list to the reference"
        adj[p[:, 0], p[:, 1]] = 1.0
        adj[p[:, 1], p[:, 0]] = 1.0
    return adj


def _colnorm(m):
    s = np.abs(m).sum(axis=0)
    s[s == 0] = 1
    return m / s


def restated_mcl(adj, dtype=np.float64, perturb_seed=None):
    """mcl_ref.run_mcl with its defaults, written out again in plain numpy in ``dtype``; ``perturb_seed``:
    every entry of the expansion product is scaled by 1 + k * eps, k a seeded integer in [-4, 4].
    Returns (matrix, iterations, converged)."""
    m = np.array(adj, dtype=dtype)
    n = m.shape[0]
    idx = np.arange(n)
    m[idx, idx] = 1
    m = _colnorm(m)
    rng = None if perturb_seed is None else np.random.default_rng(perturb_seed)
    eps = np.finfo(dtype).eps
    rtol, atol, thr = dtype(1e-5), dtype(1e-8), dtype(PRUNE)
    for it in range(1, ITERATIONS + 1):
        last = m
        prod = m @ m
        if rng is not None:
            prod = prod * (1 + eps * rng.integers(-4, 5, size=prod.shape).astype(dtype))
        m = _colnorm(prod * prod)
        pruned = np.where(m >= thr, m, 0)
        top = m.argmax(axis=0)
        pruned[top, idx] = m[top, idx]
        m = pruned
        if (np.abs(m - last) - rtol * np.abs(last)).max() <= atol:
            return m, it, True
    return m, ITERATIONS, False


def labels_of(m):
    """(labels, clusters) of a converged matrix, as community_detection_mcl numbers them."""
    clusters = mcl_ref.get_clusters(m)
    labels = np.zeros(m.shape[0], dtype=np.int64)
    for k, members in enumerate(clusters):
        labels[list(members)] = k
    return labels, clusters


@functools.lru_cache(maxsize=None)
def _reference_cached(key, n):
    pairs = np.frombuffer(key, dtype=np.int64).reshape(-1, 2)
    if n == 0:
        return np.zeros(0, dtype=np.int64), 0, []
    m, it = mcl_ref.run_mcl(adjacency(pairs, n))
    labels, clusters = labels_of(m)
    return labels, it, clusters


def _key(pairs):
    return np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2)).tobytes()


def reference(pairs, n):
    """(labels int64 [n], iterations, sorted clusters) of oracle.mcl_ref on the graph (pairs, n)."""
    return _reference_cached(_key(pairs), n)


@functools.lru_cache(maxsize=None)
def _robust_cached(key, n, use_longdouble):
    pairs = np.frombuffer(key, dtype=np.int64).reshape(-1, 2)
    if n == 0:
        return True
    labels, it, _ = _reference_cached(key, n)
    if it >= ITERATIONS:
        return False
    adj = adjacency(pairs, n)
    variants = [(np.float64, 20240607)]
    if use_longdouble and n <= LONGDOUBLE_MAX_NODES:
        variants.insert(0, (np.longdouble, None))
    for dtype, seed in variants:
        m, it2, ok = restated_mcl(adj, dtype, seed)
        if not ok or it2 != it or not np.array_equal(labels_of(m)[0], labels):
            return False
    return True


def robust(pairs, n, use_longdouble=True):
    """the robustness filter: variants (a), (b) (n <= 150 and ``use_longdouble``) and (c) agree on labels and
    iteration count, and all converge within the kernel's 100 iterations."""
    return _robust_cached(_key(pairs), n, bool(use_longdouble))


def has_overlap(pairs, n):
    return sum(len(c) for c in reference(pairs, n)[2]) > n


def has_prefix(pairs, n):
    """one attractor's member tuple is a proper prefix of another's (mcl_tuple_cmp's prefix branch decides)"""
    cl = reference(pairs, n)[2]
    return any(len(a) < len(b) and b[:len(a)] == a for a, b in zip(cl, cl[1:]))


def has_gap(pairs, n):
    """a cluster every member of which is relabelled by a later cluster: its number is missing from the labels"""
    labels, _, cl = reference(pairs, n)
    return len(set(labels.tolist())) < len(cl)


# ---- inputs ------------------------------------------------------------------------------------------------
def path(n):
    return [(i, i + 1) for i in range(n - 1)]


def cycle(n):
    return [(i, (i + 1) % n) for i in range(n)]


def grid(r, c):
    pairs = [(i * c + j, i * c + j + 1) for i in range(r) for j in range(c - 1)]
    return pairs + [(i * c + j, (i + 1) * c + j) for i in range(r - 1) for j in range(c)]


def bipartite(a, b):
    return [(i, a + j) for i in range(a) for j in range(b)]


def barbell(k=5, bridge=3):
    left = [(i, j) for i in range(k) for j in range(i + 1, k)]
    right = [(k + bridge + i, k + bridge + j) for i in range(k) for j in range(i + 1, k)]
    chain = [(k - 1 + i, k + i) for i in range(bridge + 1)]
    return left + chain + right, 2 * k + bridge


# the same 9-node graph twice: once clean, once with entries whose end lies outside the graph (negative, beyond
# the last node; inside a batch they point into the neighbouring graphs).  The kernel drops such entries.
_DIRTY_CLEAN = [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 5), (5, 3), (6, 7), (7, 6)]
_DIRTY = _DIRTY_CLEAN[:3] + [(0, 9), (9, 0), (-1, 2)] + _DIRTY_CLEAN[3:6] + [(8, 11), (4, -3), (30, 31), (-2, -1),
                                                                             (3, 9)] + _DIRTY_CLEAN[6:]
# Cases whose sorted cluster list holds a proper prefix, or whose labels have a gap (a cluster wholly relabelled by
# later ones): NONE found.  prefix_and_gap_search and a wider one (800 000 random graphs and trees of 3-16 nodes,
# 37 000 of them with overlapping clusters) found neither, and neither can exist at a converged state: the
# attractor of the smaller (or overwritten) cluster would itself belong to another attractor's row without being
# in that attractor's system, i.e. its column p e_a + (1 - p) e_b would have to be a fixed point of the expansion,
# which needs p^2 = p.
FOUND_CASES = []


def named_cases():
    """[(name, pairs, n)]"""
    cases = list(R.special_cases())
    cases += [("path%d" % n, path(n), n) for n in (2, 3, 4, 5, 6, 7, 8, 9, 12, 17)]
    cases += [("grid%dx%d" % (r, c), grid(r, c), r * c) for r in range(2, 6) for c in range(r, 6)]
    cases += [("K%d_%d" % (a, b), bipartite(a, b), a + b) for a, b in ((2, 2), (2, 3), (3, 3), (1, 4), (3, 5))]
    cases += [("barbell",) + barbell()]
    cases += [("single_cluster", [(i, j) for i in range(5) for j in range(i + 1, 5)], 5)]
    cases += [("two_nodes", [(1, 0)], 2), ("two_nodes_apart", [], 2)]
    cases += [("out_of_range", _DIRTY, 9)]
    cases += [("cycle8", cycle(8), 8), ("cycle11", cycle(11), 11)]
    cases += [("chords300", ) + big_graph(300, seed=3)]
    return cases + list(FOUND_CASES)


def clean(case):
    """the case without the entries the kernel drops (what the reference is given)"""
    name, pairs, n = case
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if name == "out_of_range":
        assert sorted(map(tuple, p[((p >= 0) & (p < n)).all(axis=1)].tolist())) == sorted(_DIRTY_CLEAN)
        return name, _DIRTY_CLEAN, n
    return case


def big_graph(n, seed):
    """(pairs, n): a path plus n random chords (one direction each)"""
    rng = np.random.default_rng(seed)
    chords = rng.integers(0, n, size=(n, 2))
    return np.vstack((np.asarray(path(n), dtype=np.int64), chords[chords[:, 0] != chords[:, 1]])), n


def cocktail_party(n=1030):
    """(pairs, n): the complete graph on n (even) nodes minus the perfect matching (0,1), (2,3), ...  After the first
    inflation every column is spread over n - 1 rows with entries just below 1 / 1000, the diagonal entry largest by a
    relative 1 / n: the pruning removes the whole column except the maximum it must keep.  Every node ends as its own
    cluster in 3 iterations; a pruning that forgets the maximum leaves a zero matrix and one label.  Only beyond 1000
    nodes can a column maximum lie below the pruning threshold at all."""
    iu = np.triu_indices(n, 1)
    keep = ~((iu[0] % 2 == 0) & (iu[1] == iu[0] + 1))
    return np.stack((iu[0][keep], iu[1][keep]), 1).astype(np.int64), n


def run_keep_maximum_case(run):
    pairs, n = cocktail_party()
    assert robust(pairs, n, use_longdouble=False)
    ref_labels, ref_it, _ = reference(pairs, n)
    assert ref_it == 3 and np.array_equal(ref_labels, np.arange(n))
    check_exact([("cocktail1030", pairs, n)], *run([("cocktail1030", pairs, n)]))


N_RANDOM = 300
N_SYNTHETIC = 8


@functools.lru_cache(maxsize=None)
def random_cases():
    """[(name, pairs, n)]: N_RANDOM seeded graphs of 1-120 nodes with 0-4n entries (any direction, repeats and
    self loops as they fall), every third one banded (|u - v| <= 4, contact-like), and N_SYNTHETIC internal
    graphs of synthetic.make_graph."""
    rng = np.random.default_rng(977)
    out = []
    for k in range(N_RANDOM):
        n = int(rng.integers(1, 121))
        e = int(rng.integers(0, 4 * n + 1))
        u = rng.integers(0, n, size=e)
        if k % 3 == 2:
            v = np.clip(u + rng.integers(-4, 5, size=e), 0, n - 1)
        else:
            v = rng.integers(0, n, size=e)
        out.append(("rnd%03d" % k, np.stack((u, v), axis=1).astype(np.int64), n))
    return out + [("mcl_" + nm, p, n) for nm, p, n in R.synthetic_pairs(N_SYNTHETIC, n_nodes=90, n_pairs=150,
                                                                        n_feat=4, n_c1=4, n_internal=140)]


def is_symmetric(case):
    return case[0] in SYMMETRIC


def kept_named():
    return [c for c in named_cases() if not is_symmetric(c)]


@functools.lru_cache(maxsize=None)
def kept_random():
    """(kept cases, generated, dropped, with overlapping clusters)"""
    cases = random_cases()
    kept = [c for c in cases if robust(c[1], c[2])]
    overlapping = sum(1 for c in kept if has_overlap(c[1], c[2]))
    return kept, len(cases), len(cases) - len(kept), overlapping


def filter_report():
    """the figures the issue wants printed, and the caps it sets on them"""
    kept, generated, dropped, overlapping = kept_random()
    print("mcl robustness filter: %d random cases generated, %d dropped, %d of the kept have overlapping clusters"
          % (generated, dropped, overlapping))
    assert dropped <= 0.05 * generated, (dropped, generated)
    assert overlapping >= 10, overlapping
    return kept


def with_empty_and_single(cases):
    """the cases with an N = 0 graph and an N = 1 graph in the middle"""
    mid = len(cases) // 2
    return list(cases[:mid]) + [("empty", [], 0), ("single", [], 1)] + list(cases[mid:])


# ---- comparison --------------------------------------------------------------------------------------------
def split(cases, labels, info):
    """[(labels of graph g, info of graph g)] from the batch result"""
    out, off = [], 0
    for g, (_, _, n) in enumerate(cases):
        out.append((np.asarray(labels[off:off + n]), int(info[g])))
        off += n
    assert off == len(labels)
    return out


def check_exact(cases, labels, info):
    """labels and iteration count of every graph == oracle.mcl_ref (the graphs must be robust)"""
    for case, (lab, inf) in zip(cases, split(cases, labels, info)):
        name, pairs, n = clean(case)
        if n == 0:
            assert 1 <= inf <= ITERATIONS, (name, inf)
            continue
        ref_labels, ref_it, _ = reference(pairs, n)
        np.testing.assert_array_equal(lab, ref_labels, err_msg=name)
        assert inf == ref_it, (name, inf, ref_it)


def check_symmetric(case, first, second):
    """what holds on a rounding-dependent input: the launch returns, 1 <= |info| <= 100, labels in [0, N), and a
    second launch gives the same bytes"""
    (lab, inf), = split([case], first[0], first[1])
    assert 1 <= abs(inf) <= ITERATIONS, (case[0], inf)
    assert lab.min() >= 0 and lab.max() < case[2], case[0]
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes(), case[0]


def prefix_and_gap_search(count=4000, seed=5):
    """seeded random graphs of 4-12 nodes that pass the filter and whose reference result has a proper-prefix pair
    of clusters / a gap in the labels: ([(pairs, n)] with a prefix, [(pairs, n)] with a gap).  Run by hand when the
    named cases are chosen; the suite does not call it."""
    rng = np.random.default_rng(seed)
    prefix, gap = [], []
    for _ in range(count):
        n = int(rng.integers(4, 13))
        e = int(rng.integers(n - 1, 2 * n + 1))
        pairs = rng.integers(0, n, size=(e, 2)).astype(np.int64)
        if has_prefix(pairs, n) and robust(pairs, n):
            prefix.append((pairs.tolist(), n))
        if has_gap(pairs, n) and robust(pairs, n):
            gap.append((pairs.tolist(), n))
    return prefix, gap


# ---- precluster (both depths) ------------------------------------------------------------------------------
def precluster_graphs():
    """[(name, pairs both directions [E,2], n)]: synthetic internal-contact graphs, an edgeless graph and a graph that
    is one single cluster (it pools to one node without edges)."""
    out = []
    for nm, p, n in R.synthetic_pairs(6, n_nodes=48, n_pairs=60, n_feat=4, n_c1=4, n_internal=70):
        out.append(("pre_" + nm, np.asarray(p, dtype=np.int64), n))
    k5 = np.asarray([(i, j) for i in range(5) for j in range(5) if i != j], dtype=np.int64)
    out.insert(2, ("pre_edgeless", np.zeros((0, 2), dtype=np.int64), 4))
    out.insert(4, ("pre_single_cluster", k5, 5))
    bar, nb = barbell()
    out.append(("pre_barbell", np.asarray(bar + [(v, u) for u, v in bar], dtype=np.int64), nb))
    return out


def precluster_batch(graphs, device="cpu"):
    """what ``precluster`` reads of a Batch: internal_edge_index, batch, num_graphs"""
    import types
    import torch
    ei, nptr, _ = R.batch_of(graphs)
    sizes = (nptr[1:] - nptr[:-1]).to(torch.int64)
    bvec = torch.repeat_interleave(torch.arange(len(graphs)), sizes)
    return types.SimpleNamespace(internal_edge_index=ei.to(device), batch=bvec.to(device), num_graphs=len(graphs))


def check_precluster(graphs, d0, d1):
    """both depths against mcl_ref.precluster per graph; a depth is compared only if its input passes the filter
    (depth 1: the reference's pooled graph).  Returns (graphs compared at depth 0, at depth 1)."""
    n_off = c_off = 0
    compared = [0, 0]
    for name, pairs, n in graphs:
        lab0 = d0[n_off:n_off + n]
        c = len(set(lab0.tolist()))
        lab1 = d1[c_off:c_off + c]
        n_off += n
        c_off += c
        if not robust(pairs, n):
            continue
        ref0, ref1 = mcl_ref.precluster(pairs.T, n)
        np.testing.assert_array_equal(lab0, ref0, err_msg=name + " depth 0")
        compared[0] += 1
        pooled, n_pooled = mcl_ref.pool_edge_index(ref0, pairs.T)
        assert n_pooled == c, name
        if robust(pooled.T, n_pooled):
            np.testing.assert_array_equal(lab1, ref1, err_msg=name + " depth 1")
            compared[1] += 1
    assert n_off == len(d0) and c_off == len(d1)
    return tuple(compared)


# ---- drivers shared by the two builds: ``run(cases) -> (labels ndarray, info ndarray)`` launches one batch ------
def run_named_case(case, run):
    if is_symmetric(case):
        check_symmetric(case, run([case]), run([case]))
        return
    name, pairs, n = clean(case)
    assert robust(pairs, n), "%s fails the robustness filter: list it in SYMMETRIC only if it is symmetric" % name
    check_exact([case], *run([case]))


def one_batch_cases():
    """every kept case, named and random, with an empty and a one-node graph in the middle"""
    return with_empty_and_single(kept_named() + filter_report())


def run_position_independence(run):
    """a graph alone, then first, in the middle and last among neighbours of other sizes: same labels, same info"""
    named = {c[0]: c for c in named_cases()}
    neighbours = [named[k] for k in ("grid3x3", "clique_ring", "K8", "toy6", "path12", "isolated_nodes")]
    neighbours.insert(3, random_cases()[5])
    for key in ("grid5x5", "one_direction", "single_node", "two_nodes", "out_of_range", "cycle11"):
        target = named[key]
        alone = split([target], *run([target]))[0]
        for at in (0, len(neighbours) // 2, len(neighbours)):
            cases = neighbours[:at] + [target] + neighbours[at:]
            lab, inf = split(cases, *run(cases))[at]
            assert lab.tobytes() == alone[0].tobytes() and inf == alone[1], (key, at)


def run_precluster(precluster_fn, device="cpu"):
    """precluster on a batch of non-fixture graphs, both depths; every graph must have been compared at both"""
    graphs = precluster_graphs()
    d0, d1 = precluster_fn(precluster_batch(graphs, device))
    compared = check_precluster(graphs, d0.cpu().numpy(), d1.cpu().numpy())
    print("precluster: %d graphs, %d compared at depth 0, %d at depth 1" % ((len(graphs),) + compared))
    assert compared == (len(graphs), len(graphs)), compared


def run_PreCluster_in_chunks(device, api=None):
    """PreCluster over the fixture dataset in chunks of 3 (four chunks): both depths of all ten graphs == the
    groups the reference stored"""
    from helpers import GOLDEN, NODE_FEATURES
    from deeprank_gnn_amd.clustering import PreCluster
    from deeprank_gnn_amd.dataset import GraphDataSet, GraphStore
    path_ = GOLDEN + "/fixture_1ATN.npz"
    ds = GraphDataSet(path_, node_feature=NODE_FEATURES, edge_feature=["dist"], target="irmsd")
    full = GraphStore(path_)
    for mol in ds.store.mols():                               # so that a chunk that is never written shows
        for k in [k for k in ds.store._mols[mol] if k.startswith("clustering/")]:
            del ds.store._mols[mol][k]
    assert len(ds) == 10
    PreCluster(ds, method='mcl', batch_size=3, device=device, api=api)
    for mol in full.mols():
        for depth in ("depth_0", "depth_1"):
            np.testing.assert_array_equal(ds.store.get(mol, "clustering/mcl/" + depth),
                                          full.get(mol, "clustering/mcl/" + depth), err_msg=mol + " " + depth)
