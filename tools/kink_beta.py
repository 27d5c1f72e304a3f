"""Measures the constant c of tests/elementwise.py: check_step_kinks (beta = c * max|z64| over a channel of the batch).

CPU only.  For every net and parameter seed of the SYN64 kink sweep (tests/test_gpu_parity.py) it evaluates the oracle in
fp32 and in float64 with the trace on and prints, per net, the worst fp32 error of a ReLU pre-activation (pooled: z1 / z2 of
each branch; head: the fc1 output) relative to the largest |z64| of that channel, and the ratio of KINK_C / KINK_C_HID to it.
usage: python tools/kink_beta.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deeprank_gnn_amd.synthetic as synth  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from elementwise import KINK_C, KINK_C_HID, SWEEP_SEEDS, oracle64  # noqa: E402


def main():
    batch = synth.make_batch(0, 64)
    worst_all = {}
    for net, seeds in SWEEP_SEEDS.items():
        fw = {"looped": False} if net == "FoutNet" else {}
        worst = {}
        for seed in seeds:
            params = cpu_ref.init_params(net, 32, 1, 1, seed=seed)
            t32, t64 = {}, {}
            cpu_ref.loss_and_grads(net, params, batch, batch.y, trace=t32, **fw)
            oracle64(net, params, batch, trace=t64, **fw)
            for site in [k for k in t64 if k.endswith("z1") or k.endswith("z2") or k == "hid"]:
                z32, z64 = t32[site].detach().double().numpy(), t64[site].detach().numpy()
                scale = np.abs(z64).max(axis=0)
                rel = np.abs(z32 - z64).max(axis=0) / np.where(scale > 0, scale, 1.0)
                kind = "head" if site == "hid" else "pooled"
                if rel.max() > worst.get(kind, (0.0,))[0]:
                    worst[kind] = (float(rel.max()), "seed %d %s channel %d" % (seed, site, int(rel.argmax())))
        for kind, (w, at) in sorted(worst.items()):
            worst_all[kind] = max(worst_all.get(kind, 0.0), w)
            print("%-8s %-6s worst fp32 pre-activation error / channel max|z64| = %.3g (%s)" % (net, kind, w, at))
    for kind, c in (("pooled", KINK_C), ("head", KINK_C_HID)):
        print("%-6s worst %.3g; c = %.3g = %.1fx it" % (kind, worst_all[kind], c, c / worst_all[kind]))


if __name__ == "__main__":
    main()
