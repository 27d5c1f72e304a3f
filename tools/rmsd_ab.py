"""Time the pose-by-pose RMSD matrix and RMSD clustering of docking poses (drgnn_pose_rmsd / drgnn_pose_cluster_dist,
csrc/drgnn_rmsd.h) on the device, launch by launch, next to the numpy statement of the rule in tests/rmsd_ref.py on the
CPU, after checking the device's matrix against that rule.

usage: python tools/rmsd_ab.py [--repeats 7] [--sizes 64 1024] [--limit 240] [--out profiles/rmsd_ab.txt]
Poses: the whole 1ATN topology (tests/golden/atoms_1ATN.npz: 627 residues) moved by the seeded generator of
tests/fcc_cases.py (family_batch); kind "ligand": fit on the backbone of the longer chain, RMSD of the other chain's
backbone.  Every batch size runs in a process of its own under a time limit (--limit seconds), started by this one,
which never touches the GPU.  Device rows: HIP events around back-to-back library calls on device-resident inputs (no
copy, no allocation inside the window), 2 warm-up rounds, median (min - max) over the repeats; rm_prepare, rm_pairs and
relation + greedy are timed one by one (drgnn_pose_rmsd's `phases`).  numpy row: rmsd_ref's explicit Kabsch, one process,
wall clock, timed on the pairs of the first 8 poses and quoted per pair.  FLOP/s of rm_pairs: 2 x 9 x (nF + nR)
floating-point operations for each of the M (M - 1) / 2 pairs the matrix needs (the two 3 x 3 cross sums; the fit of a
pair, ~2 000 operations, is not counted), over the vector fp64 peak of the MI355X, 78.6 TFLOP/s (half its fp32 vector
rate).  Needs the GPU: there is no fallback."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PEAK_FP64_VECTOR = 78.6e12
CUTOFF, MIN_SIZE = 7.5, 4


def one_size(M, repeats):
    """the rows of one batch size (run in a child process)"""
    import fcc_cases
    import rmsd_cases
    import rmsd_ref
    from deeprank_gnn_amd import interface as I
    table, xyz = fcc_cases.family_batch(n=M, within=None)
    poses = I.AtomTable.poses(table, xyz)
    rms, fit = I.rmsd_selection(table, kind="ligand")
    nR, nF = len(rms), len(fit)
    t0 = time.perf_counter()
    sq, scale = rmsd_ref.matrix_sq(poses.xyz[:8], rms, fit)
    n_small = min(M, 8)
    t_pair = (time.perf_counter() - t0) / max(1, n_small * (n_small - 1) // 2)
    import torch
    from deeprank_gnn_amd import _lib
    from score_ab import event_ms
    assert torch.cuda.is_available(), "rmsd_ab.py measures on the GPU"
    api = _lib.get()
    # ---- the rule first
    d = I.pose_rmsd(poses, kind="ligand")
    host = d.cpu().numpy()
    dev = np.abs(host[:8, :8] ** 2 - sq / nR)
    assert (dev <= rmsd_cases.TOL_K * rmsd_cases.EPS * scale / nR).all() and np.array_equal(host, host.T) and not np.diag(host).any()
    t0 = time.perf_counter()
    want = rmsd_ref.cluster_dist(host, CUTOFF, MIN_SIZE)
    t_cluster = time.perf_counter() - t0
    got = I.cluster_poses_rmsd(d, cutoff=CUTOFF, min_size=MIN_SIZE)
    assert np.array_equal(got.labels, want[0]) and np.array_equal(got.centres, want[1]) and np.array_equal(got.sizes, want[2])
    rows = ["M = %5d poses, %d fit + %d rms atoms: the first 8 poses' D^2 within %.3g A^2 of rmsd_ref's Kabsch form (bound %.3g);"
            % (M, nF, nR, dev.max(), (rmsd_cases.TOL_K * rmsd_cases.EPS * scale / nR).max()),
            "           D symmetric with a zero diagonal; labels, centres and sizes at %g A EQUAL the rule's on the device's D:" % CUTOFF,
            "           %d clusters of sizes %s, %d poses in none" % (len(want[1]), want[2].tolist(), int((want[0] == -1).sum()))]
    # ---- the launches on resident inputs
    cols = np.unique(np.concatenate((rms, fit)))
    x = torch.from_numpy(np.ascontiguousarray(poses.xyz[:, cols])).cuda()
    r_idx, f_idx = np.searchsorted(cols, rms).astype(np.int32), np.searchsorted(cols, fit).astype(np.int32)
    ws = torch.empty(api.rmsd_workspace(M, M, nF, nR)[0] // 8, dtype=torch.float64, device="cuda")
    out = torch.empty((M, M), dtype=torch.float64, device="cuda")
    d_r, d_f = torch.from_numpy(r_idx).cuda(), torch.from_numpy(f_idx).cuda()
    stream = _lib.current_stream(x)

    def request(phases):
        q = _lib.PoseRmsdRequest()
        q.xyz_a = q.xyz_b = x.data_ptr()
        q.rms_idx, q.fit_idx, q.host_rms_idx, q.host_fit_idx = d_r.data_ptr(), d_f.data_ptr(), r_idx.ctypes.data, f_idx.ctypes.data
        q.n_a, q.n_b, q.n_atoms, q.n_fit, q.n_rms, q.phases = M, M, len(cols), nF, nR, phases
        q.workspace, q.workspace_bytes, q.d = ws.data_ptr(), ws.numel() * 8, out.data_ptr()
        return q

    q1, q2 = request(1), request(2)
    MW = (M + 63) // 64
    rel = torch.empty((2, M, MW), dtype=torch.int64, device="cuda")
    res = torch.empty((3, M), dtype=torch.int32, device="cuda")
    k = torch.empty(1, dtype=torch.int32, device="cuda")
    q3 = _lib.PoseClusterDistRequest()
    q3.d, q3.n_poses, q3.cutoff, q3.min_size = out.data_ptr(), M, CUTOFF, MIN_SIZE
    q3.neighbours, q3.transposed = rel[0].data_ptr(), rel[1].data_ptr()
    q3.labels, q3.centres, q3.sizes, q3.n_clusters = res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), k.data_ptr()
    pairs = M * (M - 1) // 2
    flop = 18.0 * (nF + nR) * pairs
    t_numpy = {"rm_prepare": None, "rm_pairs": t_pair * pairs, "cluster": t_cluster}
    total = 0.0
    for name, fn in (("rm_prepare", lambda: api.pose_rmsd(q1, stream)), ("rm_pairs", lambda: api.pose_rmsd(q2, stream)),
                     ("cluster", lambda: api.pose_cluster_dist(q3, stream))):
        reps = max(1, min(20, 1024 // M))
        med, lo, hi = event_ms(fn, reps, repeats)
        total += med
        row = "           %-10s %10.4f ms per call (%.4f - %.4f), %d calls per timing" % (name, med, lo, hi, reps)
        if t_numpy[name] is not None:
            row += "   numpy %12.1f ms   x %.0f" % (1e3 * t_numpy[name], 1e3 * t_numpy[name] / med)
        if name == "rm_pairs":
            rate = flop / (med * 1e-3)
            row += "\n           %-10s %.3g FLOP over %d pairs: %.2f TFLOP/s fp64 = %.1f %% of the vector fp64 peak (%.1f TFLOP/s); numpy %.3f ms per pair" \
                   % ("", flop, pairs, rate / 1e12, 100.0 * rate / PEAK_FP64_VECTOR, PEAK_FP64_VECTOR / 1e12, 1e3 * t_pair)
        if name == "cluster":
            row += "   (relation + greedy loop)"
        rows.append(row)
    assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(res.cpu().numpy()[0], want[0])       # the timed calls computed the same
    t0 = time.perf_counter()
    I.cluster_poses_rmsd(poses, cutoff=CUTOFF, min_size=MIN_SIZE, kind="ligand")
    torch.cuda.synchronize()
    rows.append("           three launches %10.4f ms; cluster_poses_rmsd (host arrays -> labels, wall clock, upload included) %9.1f ms"
                % (total, 1e3 * (time.perf_counter() - t0)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--limit", type=int, default=240, help="seconds a batch size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmsd_ab.txt"))
    ap.add_argument("--one", type=int, default=0, help="(internal) run one batch size and print its rows")
    args = ap.parse_args()
    if args.one:
        import torch
        rows = one_size(args.one, args.repeats)
        print("\n".join(["#HEAD %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__)] + rows), flush=True)
        return
    lines = []
    for M in args.sizes:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(M), "--repeats", str(args.repeats)],
                               stdout=subprocess.PIPE, universal_newlines=True, timeout=args.limit)
        if child.returncode != 0:                                      # a step that failed ends the run: nothing more is started
            sys.exit("M = %d failed with status %d" % (M, child.returncode))
        rows = child.stdout.splitlines()
        head = [r for r in rows if r.startswith("#HEAD ")]
        if not lines:
            lines = ["# pairwise pose RMSD and RMSD clustering on %s; whole 1ATN, backbone, kind \"ligand\"; cutoff %g A, min_size %d"
                     % (head[0][6:], CUTOFF, MIN_SIZE),
                     "# device: HIP events around back-to-back calls, 2 warm-up rounds, median (min - max) of %d" % args.repeats,
                     "# numpy: tests/rmsd_ref.py (explicit Kabsch; fcc_ref's greedy loop), one process, wall clock",
                     "# a variant of rm_pairs on v_mfma_f64_16x16x4_f64 was not built: not measured",
                     ""]
        lines += [r for r in rows if not r.startswith("#HEAD ")]
        print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
