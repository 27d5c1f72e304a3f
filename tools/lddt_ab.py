"""Time the lDDT kernel (drgnn_pose_lddt, csrc/drgnn_lddt.h) on the device next to the numpy rule of tests/lddt_ref.py on
the CPU, in one run, with the kernel's variants side by side.

usage: python tools/lddt_ab.py [--repeats 7] [--out profiles/lddt_ab.txt]
Poses: the 1ATN topology (tests/golden/atoms_1ATN.npz) against the reference structure of tests/golden/scores_1ATN.npz;
the four real poses, then the rigid perturbations of tools/score_ab.py, M = 1, 64 and 1 024.
Device rows: HIP events around `calls` back-to-back library calls on device-resident poses and tables (no copy, no
allocation inside the window), 2 warm-up rounds, median (min - max) over the repeats, divided by `calls`; with and without
residue_counts; poses_per_pass 1 (every pose its own pass over the entries) against 4 (four poses share the loads and
bounds of an entry), alternating in one run.  A call checks its index tables on the host before it launches (the entries
of both directions): `host side` is the wall clock until the call returns, which bounds the rate of small calls.
`upload`: the four entry tables to the device, once per complex and device.  `LddtReference`: the once-per-complex half on
the host.  The CPU row runs lddt_ref (matching, d2 and the thresholds over all pairs) on the first 2 poses, whose counts
the kernel's are checked against.  Needs the GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from deeprank_gnn_amd import _lib                                                # noqa: E402
from deeprank_gnn_amd import interface as I                                      # noqa: E402
import lddt_ref                                                                  # noqa: E402
from score_ab import load, perturbed                                             # noqa: E402


def alternating_ms(fns, calls, repeats, warm=2):
    """[(median, min, max) ms per call] of every fn: each repeat times a window of `calls` calls of each in turn"""
    for fn in fns:
        for _ in range(warm * calls):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) / calls)
    return [(float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in ts]


class DeviceCall(object):
    """one drgnn_pose_lddt request on device-resident inputs, buffers allocated once"""

    def __init__(self, api, lref, xyz_grouped, residue_counts, poses_per_pass):
        self.api = api
        self.xyz = torch.from_numpy(xyz_grouped).cuda()
        self.tables = lref.device_tables("cuda")
        self.host = [lref.entry_ptr, lref.self_atom, lref.other_atom]
        M, K, R = int(xyz_grouped.shape[0]), int(lref.thresholds.size), len(lref.entry_ptr) - 1
        self.counts = torch.empty((M, 2, K), dtype=torch.int32, device="cuda")
        self.per_residue = torch.empty((M, R, 2, K), dtype=torch.int32, device="cuda") if residue_counts else None
        q = _lib.LddtRequest()
        q.xyz = self.xyz.data_ptr()
        q.entry_ptr, q.self_atom, q.other_atom, q.d_ref = [t.data_ptr() for t in self.tables]
        q.host_entry_ptr, q.host_self_atom, q.host_other_atom = [h.ctypes.data for h in self.host]
        q.n_poses, q.n_atoms, q.n_residues, q.n_entries = M, int(xyz_grouped.shape[1]), R, len(lref.self_atom)
        q.n_chain_a_atoms, q.n_thresholds, q.poses_per_pass = lref.n_chain_a_atoms, K, poses_per_pass
        q.thresholds = type(q.thresholds)(*lref.thresholds.tolist())
        q.counts = self.counts.data_ptr()
        q.residue_counts = self.per_residue.data_ptr() if residue_counts else None
        self.q = q

    def run(self):
        self.api.pose_lddt(self.q, _lib.current_stream(self.xyz))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lddt_ab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lddt_ab.py measures on the GPU"
    api = _lib.get()
    (chain, seq, res, atom, xyz4), (rc, rs, rn, rx) = load()
    table = I.AtomTable(chain, seq, res, xyz4[0], atom_name=atom)
    t0 = time.perf_counter()
    lref = I.LddtReference(table, rc, rs, rn, rx)
    t_ref = time.perf_counter() - t0
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lref.device_tables("cuda")
    torch.cuda.synchronize()
    t_up = time.perf_counter() - t0
    table_bytes = sum(a.nbytes for a in (lref.entry_ptr, lref.self_atom, lref.other_atom, lref.d_ref))
    short = chain == table.chains[1]
    poses = perturbed(xyz4, short, max(max(args.sizes), 4))
    lines = ["# lDDT on %s, torch %s; 1ATN: %d atoms per pose, %d residues; the reference: %d heavy atoms (%d matched), %d pairs within %g A "
             "(%d inter-chain), %d matched = %d entries; thresholds %s"
             % (torch.cuda.get_device_name(0), torch.__version__, table.n_atoms, table.n_residues, lref.n_ref_atoms, lref.n_matched_atoms,
                lref.n_pairs, lref.inclusion_radius, lref.n_inter_pairs, lref.n_matched_pairs, len(lref.self_atom), lref.thresholds.tolist()),
             "# device: HIP events around back-to-back calls, 2 warm-up rounds, median (min - max) of %d; a workgroup per 64 residues and pass" % args.repeats,
             "LddtReference (host, numpy, once per complex)  %9.1f ms" % (1e3 * t_ref),
             "upload of the entry tables (%.1f MB, once per complex and device)  %9.2f ms" % (table_bytes / 1e6, 1e3 * t_up)]
    # the CPU side and the equality of the counts
    rule = lddt_ref.Reference(("A", "B"), rc, rs, rn, rx)
    t0 = time.perf_counter()
    want = [rule.score(chain, seq, atom, poses[m]) for m in range(2)]
    t_cpu = (time.perf_counter() - t0) / 2
    got = I.lddt_scores(I.AtomTable.poses(table, poses[:2]), lref)
    for m, w in enumerate(want):
        assert got["preserved"][m, 0].tolist() == w["all"].tolist() and got["preserved"][m, 1].tolist() == w["inter"].tolist(), m
        assert got["lddt"][m] == w["lddt"] and got["ilddt"][m] == w["ilddt"], m
    lines += ["cpu lddt_ref (float64 numpy, one process)  %9.1f ms per pose   %10.2f poses/s" % (1e3 * t_cpu, 1.0 / t_cpu),
              "counts and scores of the 2 poses timed on the CPU: equal to the kernel's", ""]
    print("\n".join(lines), flush=True)
    for M in args.sizes:
        xyz = np.ascontiguousarray(poses[:M][:, table.order])
        calls = max(1, min(32, 256 // M))
        variants = [("poses_per_pass 1", 1, False), ("poses_per_pass 1 + residue_counts", 1, True)]
        if M >= 4:
            variants += [("poses_per_pass 4", 4, False), ("poses_per_pass 4 + residue_counts", 4, True)]
        made = [(name, DeviceCall(api, lref, xyz, per_res, pp)) for name, pp, per_res in variants]
        rows = ["M = %5d  (%d calls per window)" % (M, calls)]
        base, meds = None, []
        timed = alternating_ms([call.run for _, call in made], calls, args.repeats)
        for (name, call), (med, lo, hi) in zip(made, timed):
            t0 = time.perf_counter()
            for _ in range(calls):
                call.run()
            t_host = (time.perf_counter() - t0) / calls
            torch.cuda.synchronize()
            meds.append(med)
            base = base if base is not None else call.counts.cpu()
            assert torch.equal(base, call.counts.cpu()), name              # the variants agree on every integer
            rows.append("           %-36s %9.3f ms per call (%.3f - %.3f)   %9.3f us per pose   %10.0f poses/s   host side %7.3f ms"
                        % (name, med, lo, hi, 1e3 * med / M, 1e3 * M / med, 1e3 * t_host))
        batch = I.AtomTable.poses(table, poses[:M])
        I.lddt_scores(batch, lref, per_residue=True)
        t0 = time.perf_counter()
        I.lddt_scores(batch, lref, per_residue=True)
        t_all = time.perf_counter() - t0
        rows.append("           lddt_scores(per_residue=True) (host arrays -> dict, wall clock, upload of the poses included)  %9.1f ms   %10.0f poses/s"
                    % (1e3 * t_all, M / t_all))
        rows.append("           fastest device call against lddt_ref  %9.0f x" % (t_cpu * 1e3 * M / min(meds)))
        lines += rows
        print("\n".join(rows), flush=True)
        del made
    lines += ["", "# the library's choice (poses_per_pass 0): 4 once such passes make 1 024 workgroups (here from 410 poses on), else 1; M = 1 and 64 are "
              "bound by the call's host-side check of the entries", "# tried first and replaced (this tool, the same device): a wave bound to one residue of 16 per workgroup, one entry per lane at a time, the "
              "loads of a pass's poses behind wave-uniform branches: 1 024 poses 8.54 ms (poses_per_pass 1), 9.88 ms (4)",
              "# not tried: staging a pose's coordinates in LDS (60 KB for 1ATN; a complex beyond the LDS would still need the gathers)"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
