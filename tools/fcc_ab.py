"""Time FCC clustering of docking poses (drgnn_pose_contacts / drgnn_pose_common / drgnn_pose_cluster, csrc/drgnn_fcc.h)
on the device, stage by stage, next to the numpy statement of the rule in tests/fcc_ref.py on the CPU, after checking
that both give the same contacts, common contacts, relation and clusters.

usage: python tools/fcc_ab.py [--repeats 7] [--sizes 64 256 1024] [--out profiles/fcc_ab.txt]
Poses: the whole 1ATN topology (tests/golden/atoms_1ATN.npz: 627 residues, heavy atoms only) moved by the seeded generator
of tests/fcc_cases.py (family_batch: rigid moves of chain 1 around three placements, every tenth pose thrown far off); a
batch of M poses is the first M of the largest.  The reference contact maps are computed first, by worker processes
forked before the GPU is touched, and every device result is compared with them before anything is timed.  numpy rows: one
process, wall clock; the contact maps are timed on 8 poses and quoted per pose (every pose costs the same).  Device rows:
HIP events around back-to-back library calls on device-resident inputs (no copy, no allocation inside the window), 2
warm-up rounds, median (min - max) over the repeats.  Needs the GPU: there is no fallback."""
import argparse
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fcc_cases                                                                 # noqa: E402
import fcc_ref                                                                   # noqa: E402

_JOB = {}


def _maps_of(span):
    lo, hi = span
    t = _JOB["table"]
    return np.stack([fcc_ref.contact_map(x, t.atom_ptr, t.split, _JOB["counted"]) for x in _JOB["xyz"][lo:hi]])


def reference_maps(table, xyz32, workers):
    """fcc_ref's contact maps of all poses, by forked workers; and the time of one process per pose"""
    _JOB.update(table=table, xyz=xyz32, counted=fcc_ref.counted(table.atom_name, table.n_atoms, True))
    t0 = time.perf_counter()
    first = _maps_of((0, min(8, len(xyz32))))
    per_pose = (time.perf_counter() - t0) / len(first)
    spans = [(lo, min(lo + 16, len(xyz32))) for lo in range(len(first), len(xyz32), 16)]
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        rest = pool.map(_maps_of, spans)
    return np.concatenate([first] + rest), per_pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fcc_ab.txt"))
    args = ap.parse_args()
    from deeprank_gnn_amd import interface as I
    table, xyz = fcc_cases.family_batch(n=max(args.sizes), within=None)
    poses = I.AtomTable.poses(table, xyz)
    maps, t_map = reference_maps(table, poses.xyz, args.workers)                   # before the GPU is touched
    import torch
    from deeprank_gnn_amd import _lib
    from score_ab import event_ms
    assert torch.cuda.is_available(), "fcc_ab.py measures on the GPU"
    api = _lib.get()
    keep, atom_ptr = I.counted_atoms(table, True)
    nA, nB = table.split, table.n_residues - table.split
    W = nA * ((nB + 63) // 64)
    lines = ["# FCC clustering on %s, torch %s; 1ATN: %d residues (%d + %d), %d heavy atoms per pose; cutoff 5 A, cutoff_fcc 0.6,"
             % (torch.cuda.get_device_name(0), torch.__version__, table.n_residues, nA, nB, len(keep)),
             "# strictness 0.75, min_size 4; %d words of contact bits per pose (%d bytes)" % (W, 8 * W),
             "# device: HIP events around back-to-back calls, 2 warm-up rounds, median (min - max) of %d" % args.repeats,
             "# numpy: tests/fcc_ref.py, one process, wall clock; contact maps %.1f ms per pose (timed on 8 poses)" % (1e3 * t_map),
             "# the word-compaction variant of drgnn_pose_common (skip the words no pose of the batch sets) was not built: not measured;",
             "# each batch lists how many words it would keep",
             ""]
    print("\n".join(lines), flush=True)
    for M in args.sizes:
        batch = I.AtomTable.poses(table, xyz[:M])
        # ---- equality first
        c = I.pose_contacts(batch)
        common_ref = fcc_cases.check_contacts(c, maps[:M], "M = %d" % M)
        t0 = time.perf_counter()
        fcc_ref.common_of(maps[:M])
        t_common = time.perf_counter() - t0
        common = I.common_contacts(c)
        assert np.array_equal(common, common_ref)
        n = np.diag(common_ref).copy()
        t0 = time.perf_counter()
        nb = fcc_ref.neighbours_of(common_ref, n)
        want = fcc_ref.cluster(nb, 4)
        t_cluster = time.perf_counter() - t0
        raw = fcc_cases.check_raw_cluster(api, "cuda", common_ref, n)
        got = I.cluster_poses(c)
        fcc_cases.check_clusters(got, common_ref, n)
        row = ["M = %5d poses: contacts, counts, common, relation, labels, centres and sizes EQUAL fcc_ref's; %d contacts per pose on"
               % (M, int(np.median(n))),
               "           average (median), %d clusters of sizes %s, %d poses in none, %d tied centre choices"
               % (len(want[1]), want[2].tolist(), int((want[0] == -1).sum()), want[3]),
               "           words that some pose of the batch sets: %d of %d (what a compacted drgnn_pose_common would walk)"
               % (int((c.words().reshape(M, W) != 0).any(axis=0).sum()), W)]
        # ---- device stages on resident inputs
        d_xyz = torch.from_numpy(np.ascontiguousarray(batch.xyz[:, keep])).cuda()
        host_ap = np.ascontiguousarray(atom_ptr, dtype=np.int32)
        d_ap = torch.from_numpy(host_ap).cuda()
        bits = torch.empty((M, nA, (nB + 63) // 64), dtype=torch.int64, device="cuda")
        count = torch.empty(M, dtype=torch.int32, device="cuda")
        d_common = torch.empty((M, M), dtype=torch.int32, device="cuda")
        MW = (M + 63) // 64
        rel = torch.empty((2, M, MW), dtype=torch.int64, device="cuda")
        res = torch.empty((3, M), dtype=torch.int32, device="cuda")
        k = torch.empty(1, dtype=torch.int32, device="cuda")
        stream = _lib.current_stream(d_xyz)
        q1 = _lib.PoseContactsRequest()
        q1.xyz, q1.atom_ptr, q1.host_atom_ptr = d_xyz.data_ptr(), d_ap.data_ptr(), host_ap.ctypes.data
        q1.n_poses, q1.n_atoms, q1.n_residues, q1.n_chain_a, q1.cutoff = M, len(keep), table.n_residues, nA, 5.0
        q1.bits, q1.n_contacts = bits.data_ptr(), count.data_ptr()
        q2 = _lib.PoseCommonRequest()
        q2.bits_a = q2.bits_b = bits.data_ptr()
        q2.n_a, q2.n_b, q2.n_words, q2.common = M, M, W, d_common.data_ptr()
        q3 = _lib.PoseClusterRequest()
        q3.common, q3.n_contacts, q3.n_poses = d_common.data_ptr(), count.data_ptr(), M
        q3.cutoff_fcc, q3.cutoff_reverse, q3.min_size = 0.6, 0.6 * 0.75, 4
        q3.neighbours, q3.transposed = rel[0].data_ptr(), rel[1].data_ptr()
        q3.labels, q3.centres, q3.sizes, q3.n_clusters = res[0].data_ptr(), res[1].data_ptr(), res[2].data_ptr(), k.data_ptr()
        stages = (("contacts", lambda: api.pose_contacts(q1, stream), t_map * M, "%.1f ms per pose x M" % (1e3 * t_map)),
                  ("common", lambda: api.pose_common(q2, stream), t_common, "int32 matrix product"),
                  ("cluster", lambda: api.pose_cluster(q3, stream), t_cluster, "relation + greedy loop"))
        total = 0.0
        for name, fn, t_cpu, note in stages:
            reps = max(1, min(50, 4096 // M))
            med, lo, hi = event_ms(fn, reps, args.repeats)
            total += med
            row.append("           %-9s %10.4f ms per call (%.4f - %.4f), %d calls per timing   numpy %10.1f ms (%s)   x %.0f"
                       % (name, med, lo, hi, reps, 1e3 * t_cpu, note, 1e3 * t_cpu / med))
        K = int(k.cpu()[0])
        assert np.array_equal(bits.cpu().numpy(), c.bits.cpu().numpy()) and np.array_equal(d_common.cpu().numpy(), common_ref)
        assert K == len(want[1]) and np.array_equal(res.cpu().numpy()[0], want[0]) and np.array_equal(raw["labels"], want[0])
        t_all = t_map * M + t_common + t_cluster
        row.append("           three stages %10.4f ms   numpy %10.1f ms   x %.0f" % (total, 1e3 * t_all, 1e3 * t_all / total))
        t0 = time.perf_counter()
        I.cluster_poses(batch)
        torch.cuda.synchronize()
        row.append("           cluster_poses (host arrays -> labels, wall clock, upload included)   %9.1f ms" % (1e3 * (time.perf_counter() - t0)))
        lines += row
        print("\n".join(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
