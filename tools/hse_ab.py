"""Time the half-sphere-exposure kernel (drgnn_hse_residues, csrc/drgnn_hse.h) on the device next to the float64
statement of the rule in tests/hse_ref.py on the CPU, in one run, at several tile sizes (targets per workgroup), and
record how far the kernel's angle is from hse_ref.

usage: python tools/hse_ab.py [--repeats 7] [--sizes 1 64 1024] [--tiles 4 16 64 256] [--out profiles/hse_ab.txt]
Poses: the 1ATN topology (tests/golden/atoms_1ATN.npz, 6 003 atoms, 627 residues, names from scores_1ATN.npz); the four
real poses, then rigid perturbations of chain B of those four (tools/score_ab.py's).  Targets: once every residue, once
the node residues of every pose as interface_graphs finds them.  Deviation: the largest |angle - hse_ref| over all
2508 residues of the four real poses, hse_ref on the float32 coordinates the kernel sees (tests/hse_cases.py sets its
tolerance to 4 x this); the counts and the NaN rows must be equal.  Device rows: HIP events around back-to-back library
calls on device-resident inputs (no copy, no allocation inside the window), 2 warm-up rounds, median (min - max) over
the repeats; the tile sizes are timed one after another on the same inputs.  Needs the GPU: there is no fallback."""
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
import hse_cases                                                                 # noqa: E402
from score_ab import event_ms, perturbed                                         # noqa: E402


class DeviceCall(object):
    """one drgnn_hse_residues request on device-resident inputs, buffers allocated once"""

    def __init__(self, api, table, xyz_grouped, targets, tile):
        M = int(xyz_grouped.shape[0])
        xyz, atom_ptr, res_ptr = I._ragged([(table, x) for x in xyz_grouped])[:3]
        tgt_res = np.concatenate([np.asarray(t, dtype=np.int64) + int(res_ptr[k]) for k, t in enumerate(targets)])
        tgt_cx = np.repeat(np.arange(M), [len(t) for t in targets])
        first = np.concatenate(([0], np.cumsum([len(t) for t in targets])))
        tile_ptr = np.concatenate([np.arange(lo, hi, tile) for lo, hi in zip(first[:-1], first[1:])] + [first[-1:]])
        self.host = [np.ascontiguousarray(a, dtype=np.int32) for a in (atom_ptr, res_ptr, I.hse_table(table), tgt_res, tgt_cx, tile_ptr)]
        self.dev = [torch.from_numpy(h).cuda() for h in self.host]
        self.xyz = torch.from_numpy(xyz).cuda()
        self.n_targets, self.n_tiles = int(tgt_res.shape[0]), len(tile_ptr) - 1
        self.out = torch.empty((self.n_targets, 3), dtype=torch.float64, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        q = _lib.HseRequest()
        q.xyz = self.xyz.data_ptr()
        q.atom_ptr, q.res_ptr, q.bb, q.target_res, q.target_complex, q.tile_ptr = [t.data_ptr() for t in self.dev]
        (q.host_atom_ptr, q.host_res_ptr, q.host_bb, q.host_target_res, q.host_target_complex,
         q.host_tile_ptr) = [h.ctypes.data for h in self.host]
        q.n_atoms, q.n_residues, q.n_complexes = int(self.xyz.shape[0]), len(self.host[0]) - 1, M
        q.n_targets, q.n_tiles, q.n_rows = self.n_targets, self.n_tiles, table.n_residues
        q.radius, q.offset, q.connect_a, q.connect_b, q.connect_cutoff, q.direction = 12.0, 0, 1, 1, 4.3, 0
        q.out, q.status = self.out.data_ptr(), self.status.data_ptr()
        self.q, self.api, self.tile = q, api, tile

    def run(self):
        self.api.hse_residues(self.q, _lib.current_stream(self.xyz))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--tiles", type=int, nargs="+", default=[4, 16, 64, 256])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hse_ab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hse_ab.py measures on the GPU"
    api = _lib.get()
    a = hse_cases.atn()
    table, xyz4 = a["table"], a["xyz"]
    chain = a["per_atom"][0]
    lines = ["# half-sphere exposure on %s, torch %s; 1ATN: %d atoms, %d residues per pose; radius 12 A, offset 0, CA links, CA direction"
             % (torch.cuda.get_device_name(0), torch.__version__, table.n_atoms, table.n_residues),
             "# device: HIP events around back-to-back calls, 2 warm-up rounds, median (min - max) of %d; one workgroup per tile of"
             % args.repeats,
             "# targets of one complex (a wave per target, lanes across the residues); residue_hse takes the tile n_targets / %d"
             % I.HSE_WORKGROUPS,
             "# within %d .. %d (interface.hse_tile).  A lane-per-target layout was not built: only the tile size is compared" % I.HSE_TILE]
    t0 = time.perf_counter()
    want = [hse_cases.atn_ref(m) for m in range(4)]
    t_cpu = (time.perf_counter() - t0) / 4
    got = I.residue_hse(I.AtomTable.poses(table, xyz4))
    worst, wrong = 0.0, 0
    for m in range(4):
        w = want[m][0]
        has = ~np.isnan(w[:, 0])
        wrong += int((np.isnan(got[m]) != np.isnan(w)).any(axis=1).sum()) + int((got[m][has, :2] != w[has, :2]).any(axis=1).sum())
        worst = max(worst, float(np.abs(got[m][has, 2] - w[has, 2]).max()))
    margin = min(w[1].min() for w in want)
    rec = hse_cases.recorded()
    off = max(np.abs(np.nan_to_num(got[m][a["nodes"][m]])[:, 2] - rec[m][:, 2]).max() for m in range(4))
    lines += ["cpu hse_ref (float64 numpy, one process, all residues)  %9.1f ms per pose   %8.2f poses/s" % (1e3 * t_cpu, 1.0 / t_cpu),
              "rows of the %d residues of the four real poses whose counts or NaN pattern differ from hse_ref: %d (smallest margin %.3g A)"
              % (4 * table.n_residues, wrong, margin),
              "largest |angle - hse_ref| over them: %.3g rad" % worst,
              "  -> MEASURED %.3g rad; the tests' tolerance is 4 x that: %.3g rad (limit 1e-6)" % (worst, 4 * worst),
              "largest |angle - recorded node_data/hse| over the 496 nodes (Biopython keeps float32 coordinates, as the kernel does):  %.3g rad" % off,
              ""]
    print("\n".join(lines), flush=True)
    assert wrong == 0
    poses = perturbed(xyz4.astype(np.float32), chain == table.chains[1], max(max(args.sizes), 4))
    for M in args.sizes:
        batch = I.AtomTable.poses(table, poses[:M])
        names = ["p%05d" % m for m in range(M)]
        store = I.interface_graphs(batch, names)
        for what, targets in (("all residues", [np.arange(table.n_residues)] * M),
                              ("node residues", [store.get(n, "node_data/residue") for n in names])):
            calls = [DeviceCall(api, table, batch.xyz, targets, tile) for tile in args.tiles]
            reps = max(1, min(200, 20000 // max(1, calls[0].n_targets // 64)))      # back-to-back calls per timing
            row = ["M = %5d poses, %s: %d targets (%.1f per pose), %d calls per timing"
                   % (M, what, calls[0].n_targets, calls[0].n_targets / M, reps)]
            outs = []
            for call in calls:
                med, lo, hi = event_ms(call.run, reps, args.repeats)
                assert int(call.status.cpu()[0]) == 0
                outs.append(call.out.cpu().numpy())
                row.append("           tile %4d (%7d workgroups)   %10.4f ms per call (%.4f - %.4f)   %8.2f us per pose   %10.0f poses/s   hse_ref x %.0f"
                           % (call.tile, call.n_tiles, med, lo, hi, 1e3 * med / M, 1e3 * M / med,
                              (1e3 * M / med) * t_cpu * (call.n_targets / (M * table.n_residues))))
            assert all(o.tobytes() == outs[0].tobytes() for o in outs)              # the tile size changes no bit
            t0 = time.perf_counter()
            I.residue_hse(batch, residues=targets)
            row.append("           residue_hse (host arrays -> arrays, wall clock, upload included)   %9.1f ms" % (1e3 * (time.perf_counter() - t0)))
            lines += row
            print("\n".join(row), flush=True)
            del calls
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
