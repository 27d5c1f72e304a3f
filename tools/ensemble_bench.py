"""Ensemble inference: ONE fused ensemble launch (drgnn_ens_predict_cached) against K back-to-back single-model launches
(FusedTrainer.predict_cached, the single model's own plan) per mini-batch, K = 1 / 2 / 5 / 10, every net, two shapes:

  SYN64   200-node synthetic graphs, 32 features, batch 64, cached topology
  treg    the 48-feature graphs of the reference's docking-scoring folds (synthetic, 40 - 85 nodes), batch 64

Times with HIP events around `reps` launches enqueued back to back (after a warm-up), median of three repetitions; prints
one line per (shape, net, K) and the ratio fused / separate.

    python tools/ensemble_bench.py [--reps 200]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import deeprank_gnn_amd.synthetic as synth  # noqa: E402
from deeprank_gnn_amd import Ensemble, GINet, sGAT, FoutNet  # noqa: E402
from deeprank_gnn_amd.resident import ResidentGraphSet  # noqa: E402

SHAPES = {
    "SYN64": lambda: [synth.make_graph(i, n_nodes=200, n_pairs=500, n_feat=32, n_c1=16, n_internal=350) for i in range(64)],
    "treg": lambda: [synth.make_graph(i, n_nodes=40 + 9 * (i % 6), n_pairs=70 + 11 * (i % 6), n_feat=48, n_c1=4,
                                      n_internal=40) for i in range(64)],
}


def timed(fn, reps):
    for _ in range(10):
        fn()
    runs = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b) * 1000.0 / reps)
    return float(np.median(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print("ensemble_bench: %s, us per mini-batch of 64 graphs (median of 3 x %d launches)" %
          (torch.cuda.get_device_name(0), args.reps))
    print("%-6s %-8s %3s %12s %12s %8s  %s" % ("shape", "net", "K", "fused_us", "separate_us", "ratio", "plan"))
    for shape, make in SHAPES.items():
        graphs = make()
        F = graphs[0].num_features
        rs = ResidentGraphSet(graphs, dev)
        ids = list(range(64))
        for Net in (GINet, sGAT, FoutNet):
            cache = rs.topology_cache(need_weights=Net is sGAT)
            ids_dev = rs.upload_ids(ids)
            for K in (1, 2, 5, 10):
                torch.manual_seed(K)
                sds = [{k: v.clone() for k, v in Net(F, 1, 1).state_dict().items()} for _ in range(K)]
                ens = Ensemble(Net, sds, device=dev)
                p, _, _, _ = ens.plan(cache, ids)
                if p.family == 0:
                    print("%-6s %-8s %3d %12s %12s %8s  NONE (K launches)" % (shape, Net.__name__, K, "-", "-", "-"))
                    continue
                fused = timed(lambda: ens._launch(cache, ids, ids_dev), args.reps)
                sep = timed(lambda: [tr.predict_cached(cache, ids, ids_dev) for tr in ens.trainers], args.reps)
                for tr in ens.trainers:
                    tr.check_faults()
                print("%-6s %-8s %3d %12.2f %12.2f %8.3f  width %d cls %d from_memory %d lds %d B" %
                      (shape, Net.__name__, K, fused, sep, fused / sep, p.width, p.cls, p.from_memory, p.lds_bytes))
                sys.stdout.flush()


if __name__ == "__main__":
    main()
