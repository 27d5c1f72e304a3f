#!/usr/bin/env python
"""A/B of one optimisation step of K models: the cohort launches (Cohort: 2 launches per step of all K members) against the
same K models as K FusedTrainers stepped one after the other by train_step_cached with their DEFAULT plan (2 K launches: the
best a user can do without the cohort).

Quantity: microseconds per COHORT STEP (all K members advanced once), device events around >= 2000 steps after warm-up, two
ways: issued eagerly from Python, and as replays of a recorded hipGraph of 20 steps on one stream.  Host time per step is the
wall time of the eager issue loop alone (no synchronisation inside).  A and B alternate, five repetitions each, every
repetition is printed.  Cached topology, SYN graphs (synthetic.make_graph: 200 nodes, 32 features), GINet with its dropout.
All members step the same mini-batch (a cycle of 4 different mini-batches), as seeds or a learning-rate sweep do; the cases
marked "distinct" give every member a mini-batch of its own in every step, as cross-validation folds with their own shuffles do
(no graph is then shared between the members of a step, and the launch carries no host-known sizes).

    python tools/cohort_ab.py [--out profiles/cohort_train_ab.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import deeprank_gnn_amd.synthetic as synth                      # noqa: E402
from deeprank_gnn_amd import Cohort                             # noqa: E402
from deeprank_gnn_amd.ginet import GINet                        # noqa: E402
from deeprank_gnn_amd.sGAT import sGAT                          # noqa: E402
from deeprank_gnn_amd.foutnet import FoutNet                    # noqa: E402
from deeprank_gnn_amd.resident import ResidentGraphSet          # noqa: E402
from deeprank_gnn_amd.trainer import FusedTrainer               # noqa: E402

NETS = {"GINet": GINet, "sGAT": sGAT, "FoutNet": FoutNet}
DEV = "cuda:0"
PER_REPLAY, CYCLE = 20, 4


def timed(fn, n):
    """(device us per call, host us per call) of n calls of fn, device events around them"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    host = time.perf_counter() - t0
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n, host * 1e6 / n


def record(fn):
    """a hipGraph of PER_REPLAY calls of fn on one stream"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(3):
            fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(PER_REPLAY):
            fn(i)
    return g


def case(name, K, B, rs, steps, reps, say, distinct=False):
    Net = NETS[name]
    cache = rs.topology_cache(need_weights=Net is sGAT)
    torch.manual_seed(K * 1000 + B)
    sds = [{k: v.clone() for k, v in Net(rs.n_feat, 1, 1).state_dict().items()} for _ in range(K)]
    seeds = list(range(100, 100 + K))
    n_b = len(rs) // B
    # rows[c][m]: member m's mini-batch in step c of the cycle
    rows = [[list(range(((c + (m if distinct else 0)) % n_b) * B, ((c + (m if distinct else 0)) % n_b + 1) * B)) for m in range(K)]
            for c in range(CYCLE)]
    # A: the cohort
    coh = Cohort(Net, sds, lr=1e-3, seeds=seeds, device=DEV)
    stage, reason, _ = coh.stage(rs, rows)
    assert stage is not None, reason
    assert stage.plan.wgs_per_graph == 1

    def a_step(i):
        stage(i % CYCLE)
    # B: K trainers in turn, default plan
    trainers = []
    for m in range(K):
        net = Net(rs.n_feat, 1, 1)
        net.load_state_dict(sds[m])
        trainers.append(FusedTrainer(net.to(DEV), lr=1e-3, task="reg", seed=seeds[m]))
    ids_dev = [[rs.upload_ids(b) for b in row] for row in rows]
    plan_b = trainers[0]._cached_prepare(cache, rows[0][0], ids_dev[0][0])["plan"]

    def b_step(i):
        c = i % CYCLE
        for m, tr in enumerate(trainers):
            tr.train_step_cached(cache, rows[c][m], ids_dev[c][m])
    for i in range(8):
        a_step(i)
        b_step(i)
    ga, gb = record(a_step), record(b_step)
    n_replays = max(1, steps // PER_REPLAY)
    res = {"A eager": [], "B eager": [], "A graph": [], "B graph": [], "A host": [], "B host": []}
    for _ in range(reps):
        for tag, fn, g in (("A", a_step, ga), ("B", b_step, gb)):
            dev_us, host_us = timed(fn, steps)
            res[tag + " eager"].append(dev_us)
            res[tag + " host"].append(host_us)
            res[tag + " graph"].append(timed(lambda i: g.replay(), n_replays)[0] / PER_REPLAY)
    coh.raise_on_faults()
    for tr in trainers:
        tr.check_faults()
    fmt = lambda v: " ".join("%7.2f" % x for x in v)            # noqa: E731
    say("%s K=%d B=%d%s   (cohort: 1 workgroup per (member, graph), %d workgroups; sequential: %d workgroup(s) per graph, %d launches)"
        % (name, K, B, " distinct mini-batches per member" if distinct else "", K * B, plan_b.wgs_per_graph, 2 * K))
    for key in ("A graph", "B graph", "A eager", "B eager", "A host", "B host"):
        label = {"A": "cohort    ", "B": "sequential"}[key[0]] + " " + {"graph": "hipGraph replay", "eager": "eager, device ",
                                                                         "host": "eager, host   "}[key[2:]]
        say("    %s  us/step: %s   min %.2f max %.2f" % (label, fmt(res[key]), min(res[key]), max(res[key])))
    worst_a, best_b = max(res["A graph"]), min(res["B graph"])
    say("    replayed: slowest cohort %.2f us, fastest sequential %.2f us -> %s (x%.2f)"
        % (worst_a, best_b, "cohort faster" if worst_a < best_b else "COHORT NOT FASTER", best_b / worst_a))
    return worst_a, best_b, min(res["A graph"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="GINet K = 4, batch 64 only (profiling runs)")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# cohort_ab.py: %s, torch %s; %d steps per repetition, %d repetitions, A / B alternating; hipGraph: %d steps per replay"
        % (torch.cuda.get_device_name(0), torch.__version__, args.steps, args.reps, PER_REPLAY))
    graphs = [synth.make_graph(i) for i in range(1280)]
    rs = ResidentGraphSet(graphs, DEV)
    verdict, single = {}, {}
    cases = [("GINet", 4, 64)] if args.quick else \
        [("GINet", K, B) for B in (64, 128) for K in (1, 2, 4, 10)] + [("sGAT", 4, 64), ("FoutNet", 4, 64)]
    for name, K, B in cases:
        worst_a, best_b, best_a = case(name, K, B, rs, args.steps, args.reps, say)
        if name == "GINet":
            verdict[(K, B)] = worst_a < best_b
            if K == 1:
                single[B] = best_b
            if K == 10 and B in single:
                say("    K = 10: cohort %.2f us against 10 x the single step (%.2f us) = %.2f us" % (best_a, single[B], 10 * single[B]))
    if not args.quick:
        for K, B in ((4, 64), (10, 128)):
            case("GINet", K, B, rs, args.steps, args.reps, say, distinct=True)
        ok = verdict.get((4, 64)) and verdict.get((2, 128))
        say("# requirement (GINet K=4 B=64 and K=2 B=128: slowest cohort repetition faster than fastest sequential repetition): %s"
            % ("MET" if ok else "NOT MET"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
