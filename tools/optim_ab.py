#!/usr/bin/env python
"""What the optimiser options cost per optimisation step: GINet, SYN graphs (synthetic.make_graph: 200 nodes, 32 features),
batch 64, cached topology, train_step_cached.

    (a) options off                       step launch + k_update
    (b) AdamW + learning-rate table       step launch + k_update_opt             (one launch, one more load and product)
    (c) (b) + gradient-norm clipping      step launch + k_update_opt (sums, per-block norm words) + k_adam_opt
    (d) coupled L2 weight decay           step launch + k_update (sums) + k_adam (the route that existed before the options)

and the same (a) - (c) for a cohort of K = 4 (Cohort.stage: cohort step launch + cohort update [+ cohort Adam launch]).

Quantity: microseconds per step, device events around replays of a recorded hipGraph of 20 steps on one stream (a cycle of 4
mini-batches), after warm-up; the cases alternate, ``--reps`` repetitions each, every repetition is printed and the median is
the figure.  Expectations checked at the end: (b) within the run-to-run spread of (a); (c) about one launch more than (b) and
no more than (d) by more than that spread.

    python tools/optim_ab.py [--out profiles/optim_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import deeprank_gnn_amd.synthetic as synth                      # noqa: E402
from deeprank_gnn_amd import Cohort                             # noqa: E402
from deeprank_gnn_amd.ginet import GINet                        # noqa: E402
from deeprank_gnn_amd.resident import ResidentGraphSet          # noqa: E402
from deeprank_gnn_amd.trainer import FusedTrainer               # noqa: E402

DEV = "cuda:0"
PER_REPLAY, CYCLE, B, K = 20, 4, 64, 4
TABLE = [1e-3 * 0.999 ** i for i in range(4096)]
CASES = [("a", "options off", {}),
         ("b", "AdamW + table", dict(weight_decay=0.01, decoupled_weight_decay=True, lr_schedule=TABLE)),
         ("c", "AdamW + table + clip", dict(weight_decay=0.01, decoupled_weight_decay=True, lr_schedule=TABLE, max_grad_norm=1.0)),
         ("d", "coupled L2", dict(weight_decay=0.01))]


def record(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(CYCLE):
            fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(PER_REPLAY):
            fn(i)
    return g


def timed(g, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (n * PER_REPLAY)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# optim_ab.py: %s, torch %s; GINet, batch %d, cached topology; %d steps per repetition, %d repetitions, cases "
        "alternating; hipGraph: %d steps per replay" % (torch.cuda.get_device_name(0), torch.__version__, B, args.steps, args.reps,
                                                        PER_REPLAY))
    rs = ResidentGraphSet([synth.make_graph(i) for i in range(CYCLE * B)], DEV)
    cache = rs.topology_cache(need_weights=False)
    rows = [list(range(c * B, (c + 1) * B)) for c in range(CYCLE)]
    ids_dev = [rs.upload_ids(r) for r in rows]
    torch.manual_seed(0)
    sds = [{k: v.clone() for k, v in GINet(rs.n_feat, 1, 1).state_dict().items()} for _ in range(K)]
    graphs, keep = {}, []
    for tag, _, kw in CASES:
        net = GINet(rs.n_feat, 1, 1)
        net.load_state_dict(sds[0])
        tr = FusedTrainer(net.to(DEV), lr=1e-3, task="reg", seed=5, **kw)
        keep.append(tr)
        graphs["single " + tag] = record(lambda i, tr=tr: tr.train_step_cached(cache, rows[i % CYCLE], ids_dev[i % CYCLE]))
    for tag, _, kw in CASES[:3]:
        coh = Cohort(GINet, sds, lr=1e-3, seeds=list(range(100, 100 + K)), device=DEV, **kw)
        stage, reason, _ = coh.stage(rs, [[r] * K for r in rows])
        assert stage is not None, reason
        keep.append((coh, stage))
        graphs["cohort " + tag] = record(lambda i, stage=stage: stage(i % CYCLE))
    n = max(1, args.steps // PER_REPLAY)
    res = {k: [] for k in graphs}
    for g in graphs.values():
        timed(g, n)
    for _ in range(args.reps):
        for k, g in graphs.items():
            res[k].append(timed(g, n))
    for t in keep:
        if isinstance(t, FusedTrainer):
            t.check_faults()
            assert bool(torch.isfinite(t.flat_p).all())
        else:
            t[0].raise_on_faults()
    med = {k: statistics.median(v) for k, v in res.items()}
    names = {tag: what for tag, what, _ in CASES}
    for k, v in res.items():
        say("%-9s (%s) %-22s us/step: %s   median %.2f  min %.2f  max %.2f" % (
            k, k[-1], names[k[-1]], " ".join("%6.2f" % x for x in v), med[k], min(v), max(v)))
    for kind in ("single", "cohort"):
        a, b, c = (med["%s %s" % (kind, t)] for t in "abc")
        spread = max(max(res["%s %s" % (kind, t)]) - min(res["%s %s" % (kind, t)]) for t in "abc")
        say("# %s: run-to-run spread (largest max - min of a case) %.2f us; (b) - (a) = %+.2f us: %s; (c) - (b) = %+.2f us"
            % (kind, spread, b - a, "within the spread" if abs(b - a) <= spread else "OUTSIDE the spread", c - b))
        if kind == "single":
            d = med["single d"]
            spread = max(spread, max(res["single d"]) - min(res["single d"]))
            say("# single: (c) - (d) = %+.2f us: %s" % (c - d, "no more than (d) by more than the spread" if c - d <= spread
                                                        else "(c) costs MORE than (d) beyond the spread"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
