"""Inputs and checks shared by tests/test_topology_paths.py (host emulation) and tests/test_gpu_topology_paths.py (the
device): the topology builder (csrc/drgnn_topology.h) at the sizes where it changes its code path.

Every case is a small batch around one SPECIAL graph whose node, edge or cluster count sits on a condition of the builder's
code; `Case.sits_on` quotes that condition and `Case.edge` states it over numbers recomputed from the batch in numpy
(`facts`), so a change of the graph maker cannot move a case off its edge unnoticed.  Cluster ids are labels drawn from
[0, N) -- distinct, not ranked -- which is what the lean chains accept; `ids=` makes them anything else.

The checks use no figure measured on the code under test: structure arrays are integers (equality with the oracle), `W0` is
a permutation of the input (equality), and `W1` is held to the error bound of the builder's own number format (check_w1).
"""
import numpy as np
import torch

from topo_check import check_against_oracle, check_tiles
from deeprank_gnn_amd import _lib
from deeprank_gnn_amd.data import Batch, Data
from deeprank_gnn_amd.topology import Topology

HIER, LEAN, TILES = _lib.TOPO_HIER, _lib.TOPO_LEAN, _lib.TOPO_TILES
NTHREADS = 1024                 # DRGNN_NTHREADS (csrc/drgnn_rt.h)
SPLIT_MAX_GRAPHS = 160          # DRGNN_TOPO_SPLIT_MAX_GRAPHS (csrc/drgnn_capi.hip)
LDS_LIMIT = 160 * 1024
FORCED_GLOBAL = 100000          # `_max_nodes` / `_max_edges` no LDS holds: the builder works out of global scratch

# request flags by name.  "default" is drgnn_topology_build: the general chains, the hierarchical order, nothing else.
FLAGS = {"default": HIER, "lean": HIER | LEAN, "lean_tiles": HIER | LEAN | TILES, "tiles": HIER | TILES}

# the arrays a lean workspace promises (tests/test_emu_topology.py), with TSLOT1 / W0 / W1 when edge weights are built
PROMISED = ["ROWPTR0", "COL0", "EID0", "CL0", "NC0", "ROWPTR1", "COL1", "NE1", "COLPTR1", "ROWIDX1", "CL1", "NC1", "MPTR1",
            "MEM1", "HORD", "HMP0", "HSPLIT"]


# ---------------------------------------------------------------------------------------------------------------------
# the graph maker
def random_sizes(rng, n, c):
    """c cluster sizes >= 1 that add up to n"""
    return 1 + rng.multinomial(n - c, np.full(c, 1.0 / c))


def make_graph(seed, n_nodes, sizes0, n_c1, n_pairs, weights="pos", ids="labels", one_way=0, dup=0, self_loops=0, c1_of=None,
               n_feat=8):
    """One graph: `sizes0` = the node counts of the depth-0 clusters, `n_c1` depth-1 clusters (every one inhabited),
    `n_pairs` distinct undirected pairs listed in both directions, `one_way` further pairs listed once, then `dup` repeats of
    the first directed edges and `self_loops` loops; the edge list is shuffled.
    ids: "labels" = distinct labels from [0, N) in random order; "one_out" = the same with one depth-0 label set to N;
    "arbitrary" = int64 values far from any small range.
    c1_of: the depth-1 cluster (its RANK) of every depth-0 cluster, in `sizes0` order (default: random).
    weights: "pos" uniform 0.1 - 2; "signed" normal * 10**k, k in -6 .. 5; "zero"."""
    rng = np.random.default_rng(seed)
    N = int(n_nodes)
    sizes0 = np.asarray(sizes0, dtype=np.int64)
    C = int(sizes0.size)
    assert sizes0.sum() == N and sizes0.min() >= 1 and 1 <= n_c1 <= C
    labels = rng.permutation(N)[:C].astype(np.int64)
    if ids == "one_out":
        labels[0] = N
    member = rng.permutation(np.repeat(np.arange(C), sizes0))       # cluster (position in sizes0) of every node
    rank = np.argsort(np.argsort(labels))                           # consecutive number of a cluster = rank of its label
    if c1_of is None:
        c1_of = rng.permutation(np.arange(C) % n_c1)
    c1_of = np.asarray(c1_of, dtype=np.int64)
    assert c1_of.size == C and np.unique(c1_of).size == n_c1 and c1_of.max() == n_c1 - 1
    labels1 = np.sort(rng.permutation(N)[:n_c1]).astype(np.int64)
    cluster1 = np.empty(C, dtype=np.int64)
    cluster1[rank] = labels1[c1_of]                                 # cluster1 is indexed by the consecutive depth-0 number
    cluster0 = labels[member]
    if ids == "arbitrary":
        cluster0 = cluster0 * 1000003 + 7 * 10 ** 11
        cluster1 = cluster1 * 99991 + 10 ** 12
    n_draw = n_pairs + one_way
    if n_draw:
        iu, iv = np.triu_indices(N, 1)
        pick = rng.choice(iu.size, size=n_draw, replace=False)
        u, v = iu[pick], iv[pick]
        flip = rng.random(n_draw) < 0.5
        u, v = np.where(flip, v, u), np.where(flip, u, v)
    else:
        u = v = np.zeros(0, dtype=np.int64)
    row = np.concatenate([u[:n_pairs], v[:n_pairs], u[n_pairs:]])
    col = np.concatenate([v[:n_pairs], u[:n_pairs], v[n_pairs:]])
    if dup:
        row, col = np.concatenate([row, row[:dup]]), np.concatenate([col, col[:dup]])
    if self_loops:
        loops = rng.integers(0, N, size=self_loops)
        row, col = np.concatenate([row, loops]), np.concatenate([col, loops])
    order = rng.permutation(row.size)
    row, col = row[order].astype(np.int64), col[order].astype(np.int64)
    E = int(row.size)
    if weights == "pos":
        w = rng.uniform(0.1, 2.0, size=E)
    elif weights == "signed":
        w = rng.standard_normal(E) * 10.0 ** rng.integers(-6, 6, size=E)
    else:
        assert weights == "zero"
        w = np.zeros(E)
    g = Data(x=torch.from_numpy(rng.standard_normal((N, n_feat)).astype(np.float32)),
             edge_index=torch.from_numpy(np.stack([row, col])),
             edge_attr=torch.from_numpy(w.astype(np.float32).reshape(-1, 1)),
             y=torch.tensor([float(rng.uniform(0.0, 20.0))]), pos=torch.zeros(N, 3))
    g.cluster0 = torch.from_numpy(cluster0)
    g.cluster1 = torch.from_numpy(cluster1)
    return g


def ordinary(seed, weights="pos", n_feat=8):
    """an ordinary 30-node graph: 10 clusters of random sizes, 3 depth-1 clusters, 50 pairs; the even-numbered ones repeat two
    edges and carry a self loop"""
    rng = np.random.default_rng(9000 + seed)
    extra = dict(dup=2, self_loops=1) if seed % 2 == 0 else {}
    return make_graph(9000 + seed, 30, random_sizes(rng, 30, 10), 3, 50, weights=weights, n_feat=n_feat, **extra)


def clusters_graph(C, n_c1, weights="pos", ids="labels", n_feat=8, seed=0):
    """3 C nodes in C clusters of random sizes >= 1, 4 C pairs"""
    rng = np.random.default_rng(100 + C + 1000 * seed)
    return make_graph(100 + C + 1000 * seed, 3 * C, random_sizes(rng, 3 * C, C), n_c1, 4 * C, weights=weights, ids=ids, n_feat=n_feat)


def small_graph(seed):
    """an 8 - 30 node graph"""
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.integers(8, 31))
    c = int(rng.integers(1, n + 1))
    return make_graph(7000 + seed, n, random_sizes(rng, n, c), int(rng.integers(1, min(c, 4) + 1)), int(rng.integers(0, 2 * n)))


# ---------------------------------------------------------------------------------------------------------------------
# the cases
class Case(object):
    """name; `graphs()` -> the list of Data; `special` = the graph that sits on the edge; `sits_on` = the condition in the
    code; `edge(f)` = that condition over `facts` (numpy only); global_scratch: built out of global memory;
    no_tiles: why the builder forms no aggregation tiles for this batch (None: it does)."""

    def __init__(self, name, graphs, special, sits_on, edge, global_scratch=False, no_tiles=None, status=0, force=True):
        self.name, self._graphs, self.special, self.sits_on, self.edge = name, graphs, special, sits_on, edge
        self.global_scratch, self.no_tiles, self.status = global_scratch, no_tiles, status
        self.force = global_scratch and force      # (False: the graph is beyond the LDS carve by itself)
        self._batch = None

    def graphs(self):
        return self._graphs()

    def batch(self):
        """the collated batch on the host, made once; never modified (clone it)"""
        if self._batch is None:
            b = Batch.from_data_list(self.graphs())
            if self.force:
                b.__dict__["_max_nodes"] = FORCED_GLOBAL
                b.__dict__["_max_edges"] = FORCED_GLOBAL
            self._batch = b
        return self._batch

    def flag_names(self):
        return [k for k in FLAGS if self.no_tiles is None or not (FLAGS[k] & TILES)]


def facts(batch, g, global_scratch=None):
    """What the builder's conditions depend on, for graph g, recomputed from the batch in numpy.  global_scratch: the batch is
    built out of global scratch (default: when its bounds are the forced ones) -- the scratch is then carved per graph."""
    b = batch.batch.numpy()
    B = int(batch.num_graphs)
    ei = batch.edge_index.numpy()
    nodes = np.bincount(b, minlength=B)
    edges = np.bincount(b[ei[0]], minlength=B)
    c0_all = batch.cluster0.numpy()
    n_c0 = [np.unique(c0_all[b == k]).size for k in range(B)]
    c0 = c0_all[b == g]
    N, E, C = int(nodes[g]), int(edges[g]), int(n_c0[g])
    c1_ptr = batch.__dict__["_c1_ptr"].numpy()
    c1 = batch.cluster1.numpy()[c1_ptr[g]:c1_ptr[g + 1]]
    C1 = int(np.unique(c1[:C]).size)
    forced = int(batch.__dict__["_max_nodes"]) >= FORCED_GLOBAL if global_scratch is None else bool(global_scratch)
    max_nodes, max_edges = int(nodes.max()), int(edges.max())
    capT = N + E + 1 if forced else max(max_nodes, max(max_edges, 1)) + 1
    capF = N + E + 2 if forced else max_nodes + max(max_edges, 1) + 2
    BW = (C + 31) // 32
    need = 2 * C * BW + 1
    in_range = bool(c0.min() >= 0 and c0.max() < N and (c1.size == 0 or (c1.min() >= 0 and c1.max() < N)))
    rc = 1 if (not in_range or 2 * N + 2 > capF) else 2 if need > capT else 0
    sizes = np.unique(c0, return_counts=True)[1]
    return dict(B=B, N=N, E=E, C=C, C1=C1, BW=BW, need=need, capT=capT, capF=capF, in_range=in_range, rc=rc, forced=forced,
                max_nodes=max_nodes, max_edges=max_edges, sizes=sizes, c1_len=int(c1.size),
                # the end of the lean clusters chain an unweighted device build takes
                tail=None if rc else ("single" if need <= NTHREADS else "scan"))


def _around(make_special, weights="pos"):
    return lambda: [ordinary(1, weights), make_special(), ordinary(2, weights)]


def _c_case(C, n_c1, sits_on, edge):
    return Case("C%d" % C, _around(lambda: clusters_graph(C, n_c1)), 1, sits_on, edge)


def _huge(tie):
    # 150 nodes: one cluster of 100 and 50 singletons in 3 depth-1 clusters.  tie: the depth-1 clusters hold 20 | 100 + 10 | 20
    # nodes -> the split candidates are 0, 20, 130, 150 nodes, |2 pos - N| = 150, 110, 110, 150: k = 1 and k = 2 tie, 1 wins
    sizes = [100] + [1] * 50
    c1_of = [1] + [0] * 20 + [1] * 10 + [2] * 20 if tie else None
    return make_graph(31 + tie, 150, sizes, 3, 300, c1_of=c1_of)


def _nodes_graph(N):
    sizes = [8] * (N // 8) + ([N % 8] if N % 8 else [])
    return make_graph(N, N, sizes, 65, N)


def _edges_graph(E):
    rng = np.random.default_rng(E)
    one_way = 3 if E % 2 else 2
    return make_graph(E, 40, random_sizes(rng, 40, 10), 3, (E - one_way) // 2, one_way=one_way)


def _weights_graphs(kind):
    rng = np.random.default_rng(5)
    return [make_graph(51, 60, random_sizes(rng, 60, 15), 4, 150, weights=kind),
            make_graph(52, 120, random_sizes(rng, 120, 3), 2, 2000, weights=kind),      # ~6 pooled edges of ~440 addends each
            ordinary(3, kind)]


def _packed_graphs():
    rng = np.random.default_rng(6)
    return [ordinary(4), make_graph(61, 600, random_sizes(rng, 600, 300), 9, 32768),
            make_graph(62, 600, random_sizes(rng, 600, 300), 9, 32768, one_way=1)]


def _b_graphs(B):
    if B == 1:
        return [clusters_graph(33, 7)]
    return [clusters_graph(33, 7)] + [small_graph(k) for k in range(B - 2)] + [clusters_graph(65, 7)]


def _c1_wrong(delta):
    def graphs():
        gs = [ordinary(1), clusters_graph(33, 7), ordinary(2)]
        c1 = gs[1].cluster1
        gs[1].cluster1 = torch.cat([c1, c1[:1]]) if delta > 0 else c1[:-1].clone()
        return gs
    return graphs


GLOBAL = "global scratch: tiles are formed by the LDS builder only"
CASES = [
    # ---- BW = ceil(C / 32) words per bitmap row going 1 -> 2 -> 3; a trip of topo_count_below<8> covers 32 keys
    _c_case(31, 7, "BW = (C + 31) >> 5 = 1; one trip of topo_count_below over C keys", lambda f: f["BW"] == 1 and f["C"] == 31 and f["rc"] == 0),
    _c_case(32, 7, "BW = 1, C = 32: the last full single-word row; exactly one trip", lambda f: f["BW"] == 1 and f["C"] == 32 and f["rc"] == 0),
    _c_case(33, 7, "BW = 2: the first two-word row; a second trip with one key", lambda f: f["BW"] == 2 and f["C"] == 33 and f["rc"] == 0),
    _c_case(64, 7, "BW = 2, C = 64: two full trips", lambda f: f["BW"] == 2 and f["C"] == 64 and f["rc"] == 0),
    _c_case(65, 7, "BW = 3; a third trip with one key", lambda f: f["BW"] == 3 and f["C"] == 65 and f["rc"] == 0),
    # ---- !has_w && 2 * C * BW + 1 <= DRGNN_NTHREADS: the single-pass tail (device only); else the wg_exscan tail.
    # C1 + 1 = 71 > 64 wraps the one-wave loop over the split candidates (k += 64).
    # capT = 8 C + 1 here (4 C pairs): C = 127 / 128 fit it EXACTLY (1017 / 1025); C = 129 needs 1291 > 1033 and is refused
    # with rc == 2 -- the same graph next to a larger one (C129_roomy) or out of global scratch (global_C129) is not.
    _c_case(127, 70, "2*C*BW+1 = 1017 <= 1024: single-pass tail; = capT: the bitmaps just fit", lambda f: f["need"] == 1017 == f["capT"] and f["tail"] == "single" and f["C1"] + 1 > 64),
    _c_case(128, 70, "2*C*BW+1 = 1025 > 1024: scan tail; = capT", lambda f: f["need"] == 1025 == f["capT"] and f["tail"] == "scan" and f["C1"] + 1 > 64),
    _c_case(129, 70, "BW = 5: 2*C*BW+1 = 1291 > capT = 1033: rc == 2, topo_lean_rows_tail and the general chain", lambda f: f["BW"] == 5 and f["need"] == 1291 > f["capT"] == 1033 and f["rc"] == 2 and f["C1"] + 1 > 64),
    Case("C129_roomy", lambda: [ordinary(1), clusters_graph(129, 70), make_graph(71, 120, [40, 40, 40], 2, 700)], 1,
         "the C129 graph next to one of 1400 edges: capT = 1401 >= 1291: the lean chain, scan tail, BW = 5",
         lambda f: f["need"] == 1291 <= f["capT"] == 1401 and f["tail"] == "scan"),
    # ---- rc == 2: the bitmaps do not fit
    Case("singletons_few_edges", _around(lambda: make_graph(21, 200, [1] * 200, 90, 300)), 1,
         "2 * C * BW + 1 = 2801 > capT = 601: rc == 2", lambda f: f["need"] == 2801 and f["capT"] == 601 and f["rc"] == 2 and f["C"] == f["N"] == 200),
    # (200 nodes and 3000 edges need 168 848 bytes of LDS, over the 160 KiB limit: the builder takes this batch out of global
    # scratch by itself, where capT = N + E + 1 = 3201)
    Case("singletons_many_edges", lambda: [make_graph(22, 200, [1] * 200, 200, 1500)], 0,
         "the bitmaps fit (2801 <= capT = 3201): the lean chain with C = N = C1 (alone in its batch)",
         lambda f: f["B"] == 1 and f["need"] == 2801 <= f["capT"] == 3201 and f["rc"] == 0 and f["C"] == f["C1"] == f["N"],
         global_scratch=True, force=False, no_tiles=GLOBAL),
    # ---- empty pooled graph, E = 0, N = 1
    Case("one_cluster", lambda: [ordinary(1), make_graph(23, 130, [130], 1, 200), make_graph(24, 1, [1], 1, 0),
                                 make_graph(25, 5, [2, 3], 2, 0), ordinary(2)], 1,
         "C = 1: every edge inside one cluster, E1 = 0; then N = 1 and E = 0", lambda f: f["C"] == 1 and f["C1"] == 1 and f["N"] == 130),
    Case("one_huge_rest_single", _around(lambda: _huge(0)), 1, "HMP0 / HSPLIT with sizes 100, 1, 1, ...",
         lambda f: f["sizes"].max() == 100 and (f["sizes"] == 1).sum() == 50 and f["C1"] == 3),
    Case("one_huge_tie", _around(lambda: _huge(1)), 1, "two split candidates tie (|2 pos - N| = 110 at k = 1 and k = 2): smallest k",
         lambda f: f["sizes"].max() == 100 and (f["sizes"] == 1).sum() == 50 and f["C1"] == 3),
    # ---- pre = run_clusters && N <= DRGNN_NTHREADS: the ids requested into registers ahead of the edge list (device only)
    Case("N1024", _around(lambda: _nodes_graph(1024)), 1, "N = 1024 <= DRGNN_NTHREADS: pre on; C = 128: scan tail",
         lambda f: f["N"] == 1024 and f["E"] == 2048 and f["rc"] == 0 and f["C1"] == 65, no_tiles="a graph past what the builder stages an x tile for"),
    Case("N1025", _around(lambda: _nodes_graph(1025)), 1, "N = 1025 > DRGNN_NTHREADS: pre off; a last cluster of 1",
         lambda f: f["N"] == 1025 and f["E"] == 2050 and f["rc"] == 0 and f["C"] == 129, no_tiles="a graph past what the builder stages an x tile for"),
    # ---- (threadIdx.x & ~63) < E: which waves take part in the wmax butterfly; the edge loops' last wave
    Case("E63", _around(lambda: _edges_graph(63)), 1, "E = 63: one partial wave", lambda f: f["E"] == 63 and f["N"] == 40 and f["C"] == 10),
    Case("E64", _around(lambda: _edges_graph(64)), 1, "E = 64: exactly one wave", lambda f: f["E"] == 64 and f["N"] == 40 and f["C"] == 10),
    Case("E65", _around(lambda: _edges_graph(65)), 1, "E = 65: a second wave with one edge", lambda f: f["E"] == 65 and f["N"] == 40 and f["C"] == 10),
    # ---- rc == 1
    Case("arbitrary_ids", _around(lambda: clusters_graph(65, 7, ids="arbitrary")), 1,
         "ids outside [0, N): rc == 1, then the O(n^2) rank-sort branch of wg_cluster_rank (span > capF - 1)",
         lambda f: not f["in_range"] and f["rc"] == 1 and f["C"] == 65),
    Case("one_id_out_of_range", _around(lambda: clusters_graph(33, 7, ids="one_out")), 1, "one depth-0 label == N: TOPO_OVF raised by the lanes of one cluster",
         lambda f: not f["in_range"] and f["rc"] == 1 and f["C"] == 33),
    Case("global_E_lt_N", _around(lambda: make_graph(26, 50, random_sizes(np.random.default_rng(26), 50, 12), 3, 10)), 1,
         "global scratch: 2 N + 2 = 102 > capF = N + E + 2 = 72: topo_lean_preclear raises the overflow word",
         lambda f: f["forced"] and 2 * f["N"] + 2 > f["capF"] == 72 and f["in_range"] and f["rc"] == 1, global_scratch=True, no_tiles=GLOBAL),
    # (one workgroup per graph runs BOTH lean chains: after rc == 1 it finishes the rows chain itself, topo_lean_rows, from a
    # histogram that is not scanned yet -- with two workgroups per graph, as in one_id_out_of_range, another workgroup does)
    Case("global_one_id_out_of_range", _around(lambda: clusters_graph(33, 7, ids="one_out")), 1,
         "rc == 1 raised by lanes, in the workgroup that also runs the rows chain: topo_lean_rows, not topo_lean_rows_tail",
         lambda f: f["forced"] and not f["in_range"] and 2 * f["N"] + 2 <= f["capF"] and f["rc"] == 1, global_scratch=True, no_tiles=GLOBAL),
    Case("global_C129", _around(lambda: clusters_graph(129, 70)), 1, "the C129 graph out of global scratch: capT = N + E + 1 = 1420 >= 1291: lean, scan tail",
         lambda f: f["forced"] and f["need"] == 1291 <= f["capT"] == 1420 and f["rc"] == 0, global_scratch=True, no_tiles=GLOBAL),
    # ---- the fixed-point sums of the pooled weights (a graph of 4000 edges is beyond the LDS carve: global scratch by itself)
    Case("signed_weights", lambda: _weights_graphs("signed"), 1, "weights of both signs over 12 orders of magnitude; runs of ~440 addends",
         lambda f: f["E"] == 4000 and f["C"] == 3 and f["rc"] == 0, global_scratch=True, force=False, no_tiles=GLOBAL),
    Case("zero_weights", lambda: _weights_graphs("zero"), 1, "wmax = 0: topo_wscale of a zero maximum",
         lambda f: f["E"] == 4000 and f["C"] == 3 and f["rc"] == 0, global_scratch=True, force=False, no_tiles=GLOBAL),
    Case("packed_edge_ids", _packed_graphs, 1, "packed = E <= 0x10000 in topo_pool: E = 65536 (graph 1) and 65537 (graph 2)",
         lambda f: f["E"] == 0x10000 and f["C"] == 300 and f["forced"], global_scratch=True, no_tiles=GLOBAL),
    # ---- a depth-1 id list of the wrong length: flagged, the other graphs untouched
    Case("c1_one_long", _c1_wrong(+1), 1, "c1_len != C: DRGNN_S_CLUSTER1_LEN", lambda f: f["c1_len"] == f["C"] + 1, status=8),
    Case("c1_one_short", _c1_wrong(-1), 1, "c1_len != C: DRGNN_S_CLUSTER1_LEN", lambda f: f["c1_len"] == f["C"] - 1, status=8),
]
# ---- roles == 2 (two workgroups per graph): blocks of 16 serve full groups of 8 graphs, the remainder alternates; beyond
# DRGNN_TOPO_SPLIT_MAX_GRAPHS one workgroup per graph.  B is the TOTAL number of graphs: a C33 graph first, a C65 graph last,
# small graphs in between (B1: the C33 graph alone).
for _B, _what, _edge in [(1, "no full group, a remainder of 1", lambda f: f["B"] == 1),
                         (7, "no full group, a remainder of 7", lambda f: f["B"] == 7 and f["B"] >> 3 == 0),
                         (9, "one full group, a remainder of 1", lambda f: f["B"] == 9 and f["B"] >> 3 == 1 and f["B"] & 7 == 1),
                         (17, "two full groups, a remainder of 1", lambda f: f["B"] == 17 and f["B"] >> 3 == 2 and f["B"] & 7 == 1),
                         (160, "B == DRGNN_TOPO_SPLIT_MAX_GRAPHS: still two workgroups per graph, 20 full groups", lambda f: f["B"] == SPLIT_MAX_GRAPHS and f["B"] & 7 == 0),
                         (161, "one graph beyond: one workgroup per graph", lambda f: f["B"] == SPLIT_MAX_GRAPHS + 1)]:
    CASES.append(Case("B%d" % _B, (lambda B: lambda: _b_graphs(B))(_B), 0, _what, _edge))
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
WELL_FORMED = [c for c in CASES if c.status == 0]
MALFORMED = [c for c in CASES if c.status != 0]

STRIPPED = ["C128", "one_cluster", "B9"]                                       # also built without the collate-time tables
ALONE = ["C128", "C129_roomy", "singletons_few_edges", "N1025", "signed_weights"]          # check_alone_equals_batch
DEVICE_VS_EMU = ["C127", "C128", "singletons_few_edges", "N1024", "N1025", "signed_weights", "B17"]
TWICE = ["C128", "signed_weights"]


def variants(cases=None):
    """(case name, need_weights, flags name) of every build variant that applies; a tiles variant is left out exactly where
    the case says why (`no_tiles`), and tests assert `topo.tiles is None` for those."""
    return [(c.name, w, k) for c in (WELL_FORMED if cases is None else cases) for w in (False, True) for k in c.flag_names()]


def strip_layout(batch):
    """forget the collate-time tables: the builder derives the offsets (one workgroup per graph, depth 1 in a second pass)"""
    for k in ("_node_ptr", "_edge_ptr", "_c1_ptr", "_max_nodes", "_max_edges", "_max_c0", "_host_node_ptr", "_host_edge_ptr"):
        batch.__dict__.pop(k, None)
    return batch


def build(batch_cpu, api, device, weights, flags, **kw):
    """a Topology of a copy of `batch_cpu` on `device` (api None: the device library)"""
    b = batch_cpu.clone()
    if device is not None:
        b = b.to(device)
    return Topology.from_batch(b, api=api, need_weights=weights, flags=flags, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the checks
def check_w1(a, topo, batch_cpu):
    """W1 against float64.  S = the sum of the k float32 raw weights of a pooled edge, formed in float64; wmax = the graph's
    largest |w|.  The builder rounds every addend to a step of at most 2**-40 * wmax (topo_wscale / topo_wfix), adds the
    integers exactly and rounds once to float32:  |W1 - S| <= 2**-24 |S| + k wmax 2**-40."""
    ei = batch_cpu.edge_index.numpy()
    w = batch_cpu.edge_attr.numpy().reshape(-1).astype(np.float64)
    nptr, eptr = a["NPTR"], a["EPTR"]
    worst = 0.0
    for g in range(topo.n_graphs):
        n0, e0, e1 = nptr[g], eptr[g], eptr[g + 1]
        C, E1 = int(a["NC0"][g]), int(a["NE1"][g])
        cl0 = a["CL0"][n0:nptr[g + 1]].astype(np.int64)
        r, c = cl0[ei[0, e0:e1] - n0], cl0[ei[1, e0:e1] - n0]
        keep = r != c
        keys, inv, k = np.unique(r[keep] * C + c[keep], return_inverse=True, return_counts=True)
        rp1 = a["ROWPTR1"][n0 + g:n0 + g + C + 1]
        got_keys = np.repeat(np.arange(C, dtype=np.int64), np.diff(rp1)) * C + a["COL1"][e0:e0 + E1]
        np.testing.assert_array_equal(got_keys, keys, err_msg="pooled edges of graph %d" % g)
        S = np.bincount(inv.reshape(-1), weights=w[e0:e1][keep], minlength=keys.size)
        wmax = np.abs(w[e0:e1]).max() if e1 > e0 else 0.0
        err = np.abs(a["W1"][e0:e0 + E1].astype(np.float64) - S)
        bound = 2.0 ** -24 * np.abs(S) + k * wmax * 2.0 ** -40
        bad = np.nonzero(err > bound)[0]
        assert bad.size == 0, "W1 of graph %d: pooled edge %d is off by %.3e, bound %.3e (k = %d, wmax = %.3e)" % (
            g, bad[0], err[bad[0]], bound[bad[0]], k[bad[0]], wmax)
        if E1:
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def check_topology(topo, batch_cpu, weights):
    """check_against_oracle (+ check_tiles where the workspace holds tiles), IHORD = the inverse of HORD, W1 against float64"""
    a = check_against_oracle(topo, batch_cpu, weights=weights)
    if int(topo.flags) & TILES:
        check_tiles(topo, batch_cpu, weights)
    if int(topo.flags) & HIER:
        ihord = topo.array("IHORD").cpu().numpy()
        for g in range(topo.n_graphs):
            n0, n1 = a["NPTR"][g], a["NPTR"][g + 1]
            h = a["HORD"][n0:n1]
            np.testing.assert_array_equal(np.sort(h), np.arange(n1 - n0), err_msg="HORD of graph %d is no permutation" % g)
            np.testing.assert_array_equal(ihord[n0:n1][h], np.arange(n1 - n0), err_msg="IHORD of graph %d" % g)
    if weights:
        assert "W0" in a and "W1" in a          # (the lean workspaces included: check_against_oracle compared W0 by slot)
        return check_w1(a, topo, batch_cpu)
    return 0.0


def segments(topo, weights, graphs=None, hier=True):
    """{array name: {graph: the graph's part of that array}} for every promised array, with W0 / W1 (as bit patterns) and
    TSLOT1 when edge weights were built.  Everything a segment stores is local to its graph.  hier=False: without the
    hierarchical order (a workspace built without TOPO_HIER)."""
    names = [k for k in PROMISED if hier or k not in ("HORD", "HMP0", "HSPLIT")]
    arr = {k: topo.array(k).cpu().numpy() for k in names + ["NPTR", "EPTR"] + (["TSLOT1"] if weights else [])}
    if not hier:
        arr.update({k: topo.array(k).cpu().numpy() for k in ("NC0", "NE1", "NC1")})
    if weights:
        arr["W0"] = topo.weights("W0").cpu().numpy().view(np.int32)
        arr["W1"] = topo.weights("W1").cpu().numpy().view(np.int32)
    nptr, eptr, nc0, ne1, nc1 = arr["NPTR"], arr["EPTR"], arr["NC0"], arr["NE1"], arr["NC1"]
    out = {}
    for g in (range(topo.n_graphs) if graphs is None else graphs):
        n0, N, e0, E, C, E1, C1 = nptr[g], nptr[g + 1] - nptr[g], eptr[g], eptr[g + 1] - eptr[g], nc0[g], ne1[g], nc1[g]
        seg = {"ROWPTR0": (n0 + g, N + 1), "COL0": (e0, E), "EID0": (e0, E), "CL0": (n0, N), "NC0": (g, 1),
               "ROWPTR1": (n0 + g, C + 1), "COL1": (e0, E1), "NE1": (g, 1), "COLPTR1": (n0 + g, C + 1), "ROWIDX1": (e0, E1),
               "TSLOT1": (e0, E1), "CL1": (n0, C), "NC1": (g, 1), "MEM1": (n0, C), "MPTR1": (n0 + g, C1 + 1), "HORD": (n0, N),
               "HMP0": (n0 + g, C + 1), "HSPLIT": (4 * g, 4), "W0": (e0, E), "W1": (e0, E1)}
        for name in arr:
            if name in seg:
                lo, n = seg[name]
                out.setdefault(name, {})[g] = arr[name][lo:lo + n]
    return out


def assert_segments_equal(sa, sb, pairs, what):
    assert sorted(sa) == sorted(sb), (sorted(sa), sorted(sb))
    for name in sa:
        for ga, gb in pairs:
            np.testing.assert_array_equal(sa[name][ga], sb[name][gb], err_msg="%s: %s, graph %d / %d" % (what, name, ga, gb))


def check_same_bits(one, other, weights, what="full / lean", hier=True):
    """every array a lean workspace promises, graph segment by graph segment, W0 and W1 bit for bit"""
    assert one.n_graphs == other.n_graphs
    assert_segments_equal(segments(one, weights, hier=hier), segments(other, weights, hier=hier),
                          [(g, g) for g in range(one.n_graphs)], what)


def check_alone_equals_batch(case, api, device, weights, flags):
    """the special graph built in a batch of one and inside its batch: the same bits, whichever chain either build took"""
    batch = case.batch()
    g = case.special
    alone = Batch.from_data_list([case.graphs()[g]])
    if case.force:
        alone.__dict__["_max_nodes"] = alone.__dict__["_max_edges"] = FORCED_GLOBAL
    ta = build(alone, api, device, weights, flags)
    tb = build(batch, api, device, weights, flags)
    assert ta.status()[0] == 0 and tb.status()[0] == 0
    check_topology(ta, alone, weights)
    assert_segments_equal(segments(ta, weights), segments(tb, weights, [g]), [(0, g)], "%s alone / in its batch" % case.name)
    return facts(alone, 0, case.global_scratch), facts(batch, g, case.global_scratch)


def check_malformed(case, api, device, weights, flags):
    """a cluster1 list of the wrong length for the middle graph: DRGNN_S_CLUSTER1_LEN, reported for that graph; the other
    graphs' segments are those of the well-formed batch"""
    bad = case.batch()
    good = BY_NAME["C33"].batch()
    tb = build(bad, api, device, weights, flags)
    tg = build(good, api, device, weights, flags)
    st = tb.status()
    assert st[0] & 8 and st[1] == case.special and st[2] == 1, list(st)
    assert tg.status()[0] == 0
    others = [g for g in range(tg.n_graphs) if g != case.special]
    assert_segments_equal(segments(tb, weights, others), segments(tg, weights, others), [(g, g) for g in others],
                          "%s / the well-formed batch" % case.name)
