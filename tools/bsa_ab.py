"""Time the buried-surface-area kernel (drgnn_bsa_residues, csrc/drgnn_bsa.h) on the device next to the float64
statement of the rule in tests/bsa_ref.py on the CPU and next to interface_graphs for the same batch, in one run, and
record how far the kernel is from bsa_ref.

usage: python tools/bsa_ab.py [--repeats 5] [--sizes 256 8192] [--out profiles/bsa_ab.txt]
Poses: the 1ATN topology (tests/golden/atoms_1ATN.npz, 6 003 atoms, names from scores_1ATN.npz); the four real poses,
then rigid perturbations of chain B of those four (tools/score_ab.py's: a seeded rotation of up to 20 degrees about
the chain's centroid and a shift of up to 5 A).  Targets: the node residues of every pose, as interface_graphs finds
them.  Deviation: the largest |kernel - bsa_ref| over all fixture nodes of the four real poses, bsa_ref on the float32
coordinates the kernel sees (tests/bsa_cases.py sets its tolerance to 4 x this).  Device rows: HIP events around
back-to-back library calls on device-resident inputs (no copy, no allocation inside the window), 2 warm-up rounds,
median (min - max) over the repeats.  The interface_graphs rows are whole Python calls from host arrays to the
GraphStore (wall clock, uploads included), without and with bsa=True.  Needs the GPU: there is no fallback."""
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
import bsa_cases                                                                 # noqa: E402
from score_ab import event_ms, perturbed                                         # noqa: E402


class DeviceCall(object):
    """one drgnn_bsa_residues request on device-resident inputs, buffers allocated once"""

    def __init__(self, api, table, xyz_grouped, targets, radii):
        M = int(xyz_grouped.shape[0])
        part = [(table, x) for x in xyz_grouped]
        xyz, atom_ptr, res_ptr, split, _ = I._ragged(part)
        tgt_res = np.concatenate([np.asarray(t, dtype=np.int64) + int(res_ptr[k]) for k, t in enumerate(targets)])
        tgt_cx = np.repeat(np.arange(M), [len(t) for t in targets])
        self.host = [np.ascontiguousarray(a, dtype=np.int32) for a in (atom_ptr, res_ptr, split, tgt_res, tgt_cx)]
        self.dev = [torch.from_numpy(h).cuda() for h in self.host]
        self.rad = [torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32)).cuda() for r in radii]
        self.xyz = torch.from_numpy(xyz).cuda()
        self.n_targets = int(tgt_res.shape[0])
        self.out = torch.empty((self.n_targets, 3), dtype=torch.float64, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        q = _lib.BsaRequest()
        q.xyz = self.xyz.data_ptr()
        q.atom_ptr, q.res_ptr, q.res_split, q.target_res, q.target_complex = [t.data_ptr() for t in self.dev]
        q.rad_complex, q.rad_unbound = [t.data_ptr() for t in self.rad]
        (q.host_atom_ptr, q.host_res_ptr, q.host_res_split, q.host_target_res,
         q.host_target_complex) = [h.ctypes.data for h in self.host]
        q.n_atoms, q.n_residues, q.n_complexes = int(self.xyz.shape[0]), len(self.host[0]) - 1, M
        q.n_targets, q.n_radii, q.probe, q.n_slices = self.n_targets, int(self.rad[0].shape[0]), 1.4, 20
        q.out, q.status = self.out.data_ptr(), self.status.data_ptr()
        self.q, self.api = q, api

    def run(self):
        self.api.bsa_residues(self.q, _lib.current_stream(self.xyz))


def wall(fn):
    fn()
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 8192])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsa_ab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bsa_ab.py measures on the GPU"
    api = _lib.get()
    a = bsa_cases.atn()
    table, xyz4 = a["table"], a["xyz"]
    chain = a["per_atom"][0]
    radii = I.bsa_radii(table)
    lines = ["# buried surface area on %s, torch %s; 1ATN: %d atoms, %d residues per pose; probe 1.4 A, 20 slices, the reference's radii"
             % (torch.cuda.get_device_name(0), torch.__version__, table.n_atoms, table.n_residues),
             "# device: HIP events around back-to-back calls, 2 warm-up rounds, median (min - max) of %d; one workgroup per target residue"
             % args.repeats]
    # the CPU side and the deviation over all fixture nodes of the four real poses
    nodes = [np.sort(n) for n in a["nodes"]]
    t0 = time.perf_counter()
    want = [bsa_cases.atn_ref(m, nodes[m]) for m in range(4)]
    t_cpu = (time.perf_counter() - t0) / 4
    got = I.residue_bsa(I.AtomTable.poses(table, xyz4), residues=nodes, parts=True)
    dev = [max(np.abs(got[j][m][nodes[m]] - want[m][k]).max() for m in range(4)) for j, k in ((0, 2), (1, 0), (2, 1))]
    rec = max(np.abs(got[0][m][a["nodes"][m]] - a["recorded"][m]).max() for m in range(4))
    worst = max(dev)
    lines += ["cpu bsa_ref (float64 numpy, one process, node residues only)  %9.1f ms per pose   %8.2f poses/s" % (1e3 * t_cpu, 1.0 / t_cpu),
              "largest |kernel - bsa_ref| over the %d nodes of the four real poses (A^2):  bsa %.3g  sasa_unbound %.3g  sasa_complex %.3g"
              % (sum(len(n) for n in nodes), dev[0], dev[1], dev[2]),
              "  -> measured deviation %.3g A^2; the tests' tolerance is 4 x that: %.3g A^2 (limit 1e-2)" % (worst, 4 * worst),
              "largest |kernel - recorded node_data/bsa| (the record was made from the file's coordinates, not their float32):  %.3g A^2" % rec,
              ""]
    print("\n".join(lines), flush=True)
    poses = perturbed(xyz4.astype(np.float32), chain == table.chains[1], max(args.sizes))
    for M in args.sizes:
        batch = I.AtomTable.poses(table, poses[:M])
        names = ["p%05d" % m for m in range(M)]
        store = I.interface_graphs(batch, names)
        targets = [store.get(n, "node_data/residue") for n in names]
        t_plain = wall(lambda: I.interface_graphs(batch, names))
        t_bsa = wall(lambda: I.interface_graphs(batch, names, bsa=True))
        t_call = wall(lambda: I.residue_bsa(batch, residues=targets))
        call = DeviceCall(api, table, batch.xyz, targets, radii)
        med, lo, hi = event_ms(call.run, 1, args.repeats)
        assert int(call.status.cpu()[0]) == 0 and bool(torch.isfinite(call.out).all())
        n_atoms = int(sum(np.diff(table.atom_ptr)[t].sum() for t in targets))
        row = ["M = %5d poses, %d node residues (%.1f per pose, %d of their atoms evaluated per pose)"
               % (M, call.n_targets, call.n_targets / M, n_atoms // M),
               "           drgnn_bsa_residues   %10.3f ms per call (%.3f - %.3f)   %8.2f us per pose   %10.0f poses/s"
               % (med, lo, hi, 1e3 * med / M, 1e3 * M / med),
               "           residue_bsa (host arrays -> arrays, wall clock, upload included)      %9.1f ms" % (1e3 * t_call),
               "           interface_graphs (host arrays -> GraphStore, wall clock)              %9.1f ms" % (1e3 * t_plain),
               "           interface_graphs(bsa=True)                                            %9.1f ms" % (1e3 * t_bsa),
               "           device call against bsa_ref  %9.0f x" % ((1e3 * M / med) * t_cpu)]
        lines += row
        print("\n".join(row), flush=True)
        del call
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
