"""Time the deterministic Louvain pre-clustering (drgnn_louvain) on the device next to the CPU implementations.

usage: python tools/louvain_time.py [--graphs 4096] [--repeats 7] [--out FILE]
Device rows: HIP events around the bare drgnn_louvain launch (outputs preallocated, one entry per pair) and
around the whole clustering.louvain_labels call (its pair reduction and host-side sizing included), warm-up first, median over the repeats; on the
internal graphs of synthetic.make_graph (200 nodes / 350 pairs, both directions listed) and on the 10 fixture graphs.
CPU rows: tests/louvain_ref.py (the plain-Python statement the kernel is tested against) and networkx's
louvain_communities (seed 0), median per graph over the fixture graphs and the first 64 synthetic ones.  Needs the GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import louvain_ref as R                                        # noqa: E402
from deeprank_gnn_amd import _lib                              # noqa: E402
from deeprank_gnn_amd.clustering import _distinct_pairs, louvain_labels  # noqa: E402


def device_times(cases, repeats):
    ei, nptr, eptr = (t.cuda() for t in R.batch_of(cases))
    pairs, pptr = _distinct_pairs(ei, nptr, eptr)
    api = _lib.get()
    B = len(cases)
    max_nodes = max(c[2] for c in cases)
    max_edges = int((pptr[1:] - pptr[:-1]).max())
    labels = torch.empty(int(nptr[-1]), dtype=torch.int64, device="cuda")
    info = torch.empty((B, 2), dtype=torch.int32, device="cuda")
    q = torch.empty(B, dtype=torch.float64, device="cuda")
    stream = _lib.current_stream(labels)

    def bare():
        api.louvain(pairs, pairs.size(1), nptr, pptr, B, max_nodes, max_edges, labels, info, q, stream)

    def call():
        louvain_labels(ei, nptr, eptr)

    out = {}
    for name, fn in (("kernel", bare), ("louvain_labels", call)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        out[name] = float(np.median(ts))
    bare()
    torch.cuda.synchronize()
    got = labels.cpu().numpy()
    off = 0
    for name, pairs, n in cases[:16]:                 # the timed launch computes the reference's labels
        assert got[off:off + n].tolist() == R.louvain(pairs, n)[0], name
        off += n
    return out


def cpu_times(cases):
    import networkx as nx
    ref, nxt = [], []
    for _, pairs, n in cases:
        t = time.perf_counter()
        R.louvain(pairs, n)
        ref.append(time.perf_counter() - t)
        G = nx.Graph()
        G.add_nodes_from(range(n))
        G.add_edges_from(np.asarray(pairs).tolist())
        t = time.perf_counter()
        nx.community.louvain_communities(G, seed=0)
        nxt.append(time.perf_counter() - t)
    return float(np.median(ref)) * 1e3, float(np.median(nxt)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "louvain_time.py measures the device: it needs the MI355X"
    assert args.repeats >= 5
    t = time.perf_counter()
    syn = R.synthetic_pairs(args.graphs)
    gen_s = time.perf_counter() - t
    fix = R.fixture_pairs()
    lines = ["# drgnn_louvain (one 64-lane workgroup per graph) on %s, torch %s" %
             (torch.cuda.get_device_name(0), torch.__version__),
             "# device: HIP events, 3 warm-up calls, median of %d; CPU: median per graph" % args.repeats,
             "# the graphs of a launch run concurrently (one workgroup each): a launch takes about as long as its slowest",
             "# graph, so launch time / graphs is a throughput, not a per-graph latency"]
    for label, cases in (("synthetic 200 nodes / 350 pairs", syn), ("fixture 1ATN internal graphs", fix)):
        d = device_times(cases, args.repeats)
        lines.append("device  %-34s graphs %5d  kernel %9.3f ms  louvain_labels %9.3f ms  throughput %8.1f graphs/ms" %
                     (label, len(cases), d["kernel"], d["louvain_labels"], len(cases) / d["kernel"]))
    for label, cases in (("fixture graph", fix), ("synthetic graph (first 64)", syn[:64])):
        ref_ms, nx_ms = cpu_times(cases)
        lines.append("cpu     tests/louvain_ref.py (Python, int)   %8.3f ms per %s" % (ref_ms, label))
        lines.append("cpu     networkx louvain_communities seed 0  %8.3f ms per %s" % (nx_ms, label))
    lines.append("# (synthetic inputs generated in %.1f s, not timed above)" % gen_s)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
