"""Time the docking-score kernel (drgnn_dock_scores, csrc/drgnn_score.h) on the device next to the float64 reference
of tests/score_ref.py on the CPU, in one run, and record how far the two are apart.

usage: python tools/score_ab.py [--repeats 10] [--out profiles/score_ab.txt]
Poses: the 1ATN topology (tests/golden/atoms_1ATN.npz, 6 003 atoms) against the reference structure of
tests/golden/scores_1ATN.npz; the four real poses, then rigid perturbations of the short chain of those four (a seeded
rotation of up to 20 degrees about the chain's centroid and a shift of up to 5 A), M = 64, 1 024 and 8 192 in all.
Device rows: HIP events around `calls` back-to-back library calls on device-resident poses and tables (no copy, no
allocation inside the window), 2 warm-up rounds, median over the repeats, divided by `calls`.  `docking_scores` is the
whole Python call from host arrays to the dict (wall clock, upload included).  The CPU row runs score_ref (SVD Kabsch,
every atom transformed, brute-force contacts) on the first 8 poses.  Deviations: the largest |kernel - score_ref| over the
four real poses (the suite's case 2) and over the 8 timed ones.  Needs the GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from deeprank_gnn_amd import _lib                                                # noqa: E402
from deeprank_gnn_amd import interface as I                                      # noqa: E402
import score_ref                                                                 # noqa: E402

FLOATS = ("irmsd", "lrmsd", "dockQ")


def load():
    g = os.path.join(ROOT, "tests", "golden")
    with np.load(os.path.join(g, "atoms_1ATN.npz")) as z, np.load(os.path.join(g, "scores_1ATN.npz")) as s:
        n = np.diff(z["atom_ptr"])
        chain = np.repeat(np.array(["A", "B"])[z["res_chain"]], n)
        seq, res = np.repeat(z["res_seq"], n), np.repeat(z["res_names"][z["res_name_index"]], n)
        names = s["atom_names"]
        decoy = (chain, seq, res, names[s["pose_name_index"]], z["xyz_milli"] / 1000.0)
        ref = (np.array(["A", "B"])[s["ref_chain"]], s["ref_res_seq"].copy(), names[s["ref_name_index"]],
               s["ref_xyz_milli"] / 1000.0)
    return decoy, ref


def perturbed(xyz4, short, M, seed=0):
    """float32 [M, T, 3]: the four poses, then copies with the atoms `short` turned and shifted rigidly"""
    rng = np.random.default_rng(seed)
    out = np.empty((M,) + xyz4.shape[1:], dtype=np.float32)
    out[:4] = xyz4
    for m in range(4, M):
        x = xyz4[m % 4].copy()
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = np.deg2rad(rng.uniform(-20.0, 20.0))
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        rot = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        c = x[short].mean(axis=0)
        x[short] = (x[short] - c) @ rot.T + c + rng.uniform(-5.0, 5.0, 3)
        out[m] = x
    return out


class DeviceCall(object):
    """one drgnn_dock_scores request on device-resident inputs, buffers allocated once"""

    def __init__(self, api, sref, xyz_grouped):
        self.api = api
        self.xyz = torch.from_numpy(xyz_grouped).cuda()
        self.tables = sref.device_tables("cuda")
        self.host = [sref.zone_atom, sref.zone_ptr, np.ascontiguousarray(sref.pair_res.reshape(-1)), sref.atom_ptr]
        M = int(xyz_grouped.shape[0])
        self.scores = torch.empty((M, 4), dtype=torch.float64, device="cuda")
        self.classes = torch.empty((M, 2), dtype=torch.int32, device="cuda")
        self.kept = torch.empty(M, dtype=torch.int32, device="cuda")
        q = _lib.ScoreRequest()
        q.xyz = self.xyz.data_ptr()
        q.zone_atom, q.zone_ref, q.pair_res, q.atom_ptr = [t.data_ptr() for t in self.tables]
        q.host_zone_atom, q.host_zone_ptr, q.host_pair_res, q.host_atom_ptr = [h.ctypes.data for h in self.host]
        q.n_poses, q.n_atoms, q.n_residues = M, int(xyz_grouped.shape[1]), len(sref.atom_ptr) - 1
        q.n_pairs, q.n_ref_pairs, q.fnat_cutoff = sref.n_pairs, sref.n_ref_pairs, sref.fnat_cutoff
        q.scores, q.classes, q.n_preserved = self.scores.data_ptr(), self.classes.data_ptr(), self.kept.data_ptr()
        self.q = q

    def run(self):
        self.api.dock_scores(self.q, _lib.current_stream(self.xyz))


def event_ms(fn, calls, repeats, warm=2):
    for _ in range(warm * calls):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / calls)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def deviation(got, want):
    return {k: max(abs(float(got[k][m]) - w[k]) for m, w in enumerate(want)) for k in FLOATS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024, 8192])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_ab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "score_ab.py measures on the GPU"
    api = _lib.get()
    (chain, seq, res, atom, xyz4), (rc, rs, rn, rx) = load()
    table = I.AtomTable(chain, seq, res, xyz4[0], atom_name=atom)
    sref = I.ScoreReference(table, rc, rs, rn, rx)
    ref = score_ref.Reference(rc, rs, rn, rx)
    short = chain == table.chains[1 - sref.long_chain]
    poses = perturbed(xyz4, short, max(args.sizes))
    lines = ["# docking scores on %s, torch %s; 1ATN: %d atoms per pose, %d reference pairs (%d in the decoy), zones %d / %d / %d atoms"
             % ((torch.cuda.get_device_name(0), torch.__version__, table.n_atoms, sref.n_ref_pairs, sref.n_pairs) + sref.zone_sizes),
             "# device: HIP events around back-to-back calls, 2 warm-up rounds, median (min - max) of %d; one workgroup per pose" % args.repeats]
    # the CPU side and the deviations
    t0 = time.perf_counter()
    want = [ref.score(chain, seq, atom, poses[m]) for m in range(8)]
    t_cpu = (time.perf_counter() - t0) / 8
    got = I.docking_scores(I.AtomTable.poses(table, poses[:8]), sref)
    for m, w in enumerate(want):
        assert int(got["n_preserved"][m]) == w["n_preserved"] and int(got["capri_class"][m]) == w["capri_class"], m
    d4, d8 = deviation({k: got[k][:4] for k in got}, want[:4]), deviation(got, want)
    lines += ["cpu score_ref (float64 numpy, one process)  %9.1f ms per pose   %10.1f poses/s" % (1e3 * t_cpu, 1.0 / t_cpu),
              "largest |kernel - score_ref|, the four real poses (case 2):  " + "  ".join("%s %.3g" % (k, d4[k]) for k in FLOATS),
              "largest |kernel - score_ref|, the 8 poses timed on the CPU:  " + "  ".join("%s %.3g" % (k, d8[k]) for k in FLOATS),
              "n_preserved, binclass, capri_class: equal on all 8", ""]
    print("\n".join(lines), flush=True)
    for M in args.sizes:
        call = DeviceCall(api, sref, np.ascontiguousarray(poses[:M][:, table.order]))
        calls = max(1, 2048 // M)
        med, lo, hi = event_ms(call.run, calls, args.repeats)
        batch = I.AtomTable.poses(table, poses[:M])
        I.docking_scores(batch, sref)
        t0 = time.perf_counter()
        I.docking_scores(batch, sref)
        t_all = time.perf_counter() - t0
        row = ["M = %5d  drgnn_dock_scores   %9.3f ms per call (%.3f - %.3f, %d calls per window)   %8.3f us per pose   %10.0f poses/s"
               % (M, med, lo, hi, calls, 1e3 * med / M, 1e3 * M / med),
               "           docking_scores (host arrays -> dict, wall clock, upload included)  %9.1f ms   %10.0f poses/s"
               % (1e3 * t_all, M / t_all),
               "           device call against score_ref  %9.0f x" % ((1e3 * M / med) * t_cpu)]
        lines += row
        print("\n".join(row), flush=True)
        del call
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
