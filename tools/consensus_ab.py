"""Time the contact consensus of docking poses (drgnn_pose_contact_counts / drgnn_pose_consensus_numerators /
drgnn_pose_consensus_bits, csrc/drgnn_consensus.h) on the device, call by call, next to the numpy statement of the rule in
tests/consensus_ref.py on the CPU and next to the route the package had before for the same numerators, the row sums of
common_contacts (O(M^2), up to its capacity), after checking that all of them give the same integers.

usage: python tools/consensus_ab.py [--repeats 7] [--sizes 64 1024 8192] [--out profiles/consensus_ab.txt]
Poses: the whole 1ATN topology (tests/golden/atoms_1ATN.npz: 627 residues, heavy atoms only) moved by the seeded generator
of tests/fcc_cases.py (family_batch(within=None)); a batch of M poses is the first M of the largest.  The contact bits come
from pose_contacts on the device (tests/test_gpu_fcc.py holds them to fcc_ref); the reference works on their unpacked
maps.  One group of all poses; consensus bits at min_fraction 0.5.  Every device result is compared with the reference
before anything is timed.  numpy rows: one process, wall clock.  Device rows: HIP events around back-to-back library calls
on device-resident inputs (no copy, no allocation inside the window), 2 warm-up rounds, median (min - max) over the
repeats.  Needs the GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import consensus_cases                                                           # noqa: E402
import consensus_ref                                                             # noqa: E402
import fcc_cases                                                                 # noqa: E402


# The counting kernel was built in two layouts.  The first had no atomics: a wave per word (a, w) of a group walked the list
# (the words of 64 poses staged through LDS, the non-zero ones broadcast by v_readlane), a wave per row counted the residues of
# chain 0, and one workgroup per word column those of chain 1, since the OR over ALL rows of a column cannot be split without
# a sum across workgroups.  It was measured with this tool on these poses and then replaced; its row is kept here.
ATOMIC_FREE_ROW = ("# counts, the atomic-free layout built first (a wave per word, one workgroup per word column for chain 1; measured on\n"
                   "# the same poses on the MI355X, then replaced): 0.0165 ms at 64 poses, 0.2775 ms at 1024, 2.1962 ms at 8192 (the 5 column\n"
                   "# workgroups read every line of the bit tensor on one compute unit each)")


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024, 8192])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus_ab.txt"))
    args = ap.parse_args()
    import torch
    from deeprank_gnn_amd import _lib
    from deeprank_gnn_amd import interface as I
    from score_ab import event_ms
    assert torch.cuda.is_available(), "consensus_ab.py measures on the GPU"
    api = _lib.get()
    table, xyz = fcc_cases.family_batch(n=max(args.sizes), within=None)
    nA, nB = table.split, table.n_residues - table.split
    WB = (nB + 63) // 64
    W = nA * WB
    whole = I.pose_contacts(I.AtomTable.poses(table, xyz))
    del xyz
    lines = ["# contact consensus on %s, torch %s; 1ATN: %d residues (%d + %d), heavy atoms, cutoff 5 A; %d words of contact bits"
             % (torch.cuda.get_device_name(0), torch.__version__, table.n_residues, nA, nB, W),
             "# per pose (%d bytes); one group of all poses, consensus bits at min_fraction 0.5" % (8 * W),
             "# device: HIP events around back-to-back calls, 2 warm-up rounds, median (min - max) of %d" % args.repeats,
             "# numpy: tests/consensus_ref.py on the unpacked maps, one process, wall clock",
             "# row sums of common: the numerators by the O(M^2) route, drgnn_pose_common in blocks and a sum on the device, up to",
             "# %d poses" % api.fcc_capacity(1),
             "# counts: the layout of csrc/drgnn_consensus.h: the outputs zeroed on the stream, then a wave per listed pose adding with",
             "# integer atomics (two per contact); the memsets are inside the timed call",
             ATOMIC_FREE_ROW,
             ""]
    print("\n".join(lines), flush=True)
    for M in args.sizes:
        c = whole.select(np.arange(M))
        maps = consensus_cases.unpack(c.words(), nB)
        order, ptr = consensus_cases.one_group(M)
        row_of = np.zeros(M, dtype=np.int64)
        least = consensus_ref.min_count_of(0.5, [M])
        # ---- equality first
        (counts, residues), t_counts = wall(lambda: (consensus_ref.counts_of(maps, order, ptr), consensus_ref.residues_of(maps, order, ptr)))
        num, t_num = wall(lambda: consensus_ref.numerators_of(maps, counts, row_of))
        cons, t_bits = wall(lambda: consensus_ref.consensus_of(counts, least))
        d_counts, d_res = I.contact_counts_raw(api, c.bits, nB, order, ptr)
        assert np.array_equal(d_counts.cpu().numpy(), counts) and np.array_equal(d_res.cpu().numpy(), residues)
        assert np.array_equal(I.consensus_numerators_raw(api, c.bits, nB, d_counts, row_of).cpu().numpy(), num)
        d_bits, d_n = I.consensus_bits_raw(api, d_counts, least)
        assert np.array_equal(consensus_cases.unpack(d_bits.cpu().numpy(), nB), cons) and int(d_n.cpu()[0]) == int(cons.sum())
        scores = I.consensus_scores(c)
        assert consensus_cases.same_bits(scores, consensus_ref.scores_of(num, c.n_contacts, np.full(M, M)))
        by_common = M <= api.fcc_capacity(1)
        if by_common:
            assert np.array_equal(I._common_device(c).sum(dim=1, dtype=torch.int64).cpu().numpy(), num)
        row = ["M = %5d poses: counts, residue counts, numerators, consensus bits and scores EQUAL consensus_ref's%s;"
               % (M, " and the row sums of common" if by_common else ""),
               "           %d contacts per pose (median), %d pairs seen in some pose, largest count %d, %d consensus contacts, best score %.4f"
               % (int(np.median(c.n_contacts)), int((counts > 0).sum()), int(counts.max()), int(cons.sum()), float(scores.max()))]
        del maps
        # ---- device calls on resident inputs
        h_order, h_ptr = np.ascontiguousarray(order, dtype=np.int32), np.ascontiguousarray(ptr, dtype=np.int32)
        h_row, h_min = np.ascontiguousarray(row_of, dtype=np.int32), np.ascontiguousarray(least, dtype=np.int32)
        up = lambda a: torch.from_numpy(a).cuda()
        d_order, d_ptr, d_row, d_min = up(h_order), up(h_ptr), up(h_row), up(h_min)
        out_num = torch.empty(M, dtype=torch.int64, device="cuda")
        stream = _lib.current_stream(c.bits)
        q1 = _lib.ContactCountsRequest()
        q1.bits, q1.order, q1.group_ptr = c.bits.data_ptr(), d_order.data_ptr(), d_ptr.data_ptr()
        q1.host_order, q1.host_group_ptr = h_order.ctypes.data, h_ptr.ctypes.data
        q1.n_poses, q1.n_chain_a, q1.n_chain_b, q1.n_groups, q1.n_listed = M, nA, nB, 1, M
        q1.counts, q1.residues = d_counts.data_ptr(), d_res.data_ptr()
        q2 = _lib.ConsensusNumeratorsRequest()
        q2.bits, q2.counts, q2.row, q2.host_row = c.bits.data_ptr(), d_counts.data_ptr(), d_row.data_ptr(), h_row.ctypes.data
        q2.n_poses, q2.n_chain_a, q2.n_chain_b, q2.n_groups, q2.numerators = M, nA, nB, 1, out_num.data_ptr()
        q3 = _lib.ConsensusBitsRequest()
        q3.counts, q3.min_count, q3.host_min_count = d_counts.data_ptr(), d_min.data_ptr(), h_min.ctypes.data
        q3.n_chain_a, q3.n_chain_b, q3.n_groups, q3.bits, q3.n_contacts = nA, nB, 1, d_bits.data_ptr(), d_n.data_ptr()
        stages = (("counts", lambda: api.pose_contact_counts(q1, stream), t_counts, "counts and residue counts"),
                  ("numerators", lambda: api.pose_consensus_numerators(q2, stream), t_num, "a masked sum per pose"),
                  ("bits", lambda: api.pose_consensus_bits(q3, stream), t_bits, "one comparison"))
        reps = max(1, min(50, 4096 // M))
        total = 0.0
        for name, fn, t_cpu, note in stages:
            med, lo, hi = event_ms(fn, reps, args.repeats)
            total += med
            row.append("           %-11s %10.4f ms per call (%.4f - %.4f), %d calls per timing   numpy %10.1f ms (%s)   x %.0f"
                       % (name, med, lo, hi, reps, 1e3 * t_cpu, note, 1e3 * t_cpu / med))
        assert np.array_equal(d_counts.cpu().numpy(), counts) and np.array_equal(out_num.cpu().numpy(), num)
        row.append("           three calls %10.4f ms   numpy %10.1f ms" % (total, 1e3 * (t_counts + t_num + t_bits)))
        if by_common:
            med, lo, hi = event_ms(lambda: I._common_device(c).sum(dim=1, dtype=torch.int64), max(1, reps // 4), args.repeats)
            row.append("           row sums of common %10.4f ms per call (%.4f - %.4f): the numerators before this call existed   x %.1f"
                       % (med, lo, hi, med / max(event_ms(stages[1][1], reps, 3)[0] + event_ms(stages[0][1], reps, 3)[0], 1e-9)))
            row.append("           (the ratio is against counts + numerators together: what gives the numerators from the bits)")
        _, t_wall = wall(lambda: (I.consensus_scores(c), torch.cuda.synchronize()))
        row.append("           consensus_scores (PoseContacts -> scores on the host, wall clock)   %9.1f ms" % (1e3 * t_wall))
        lines += row
        print("\n".join(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
