"""Time the residue-depth kernels (drgnn_depth_residues, csrc/drgnn_depth.h) on the device, launch by launch and as a
whole, next to the float64 statement of the rule in tests/depth_ref.py on the CPU, in one run, and record how far the
kernel is from depth_ref and from the values the reference recorded.

usage: python tools/depth_ab.py [--repeats 7] [--sizes 1 64 1024] [--out profiles/depth_ab.txt]
Poses: the 1ATN topology (tests/golden/atoms_1ATN.npz, 6 003 atoms, 627 residues, names from scores_1ATN.npz); the four
real poses, then rigid perturbations of chain B of those four (tools/score_ab.py's).  Targets: once the node residues of
every pose as interface_graphs finds them, once every residue.  A call serves as many poses as fit the workspace budget of
residue_depth (DEPTH_WORKSPACE_BUDGET on the device), so a batch is a sequence of calls, each on buffers of its own allocated before the
window.  Device rows: HIP events around the calls of the whole batch (no copy, no allocation inside the window), 2 warm-up
rounds, median (min - max) over the repeats; the three launches are timed one by one through the request's `phases`
(a launch repeated on the workspace the whole call left changes no bit: asserted).  Needs the GPU: there is no fallback."""
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
import depth_cases                                                               # noqa: E402
import depth_ref                                                                 # noqa: E402
from score_ab import event_ms, perturbed                                         # noqa: E402

N_DOTS, PROBE = 192, 1.5


class DeviceCall(object):
    """one drgnn_depth_residues request on device-resident inputs, buffers allocated once"""

    def __init__(self, api, table, xyz_grouped, targets, rad, dots):
        M = int(xyz_grouped.shape[0])
        xyz, atom_ptr, res_ptr = I._ragged([(table, x) for x in xyz_grouped])[:3]
        tgt_res = np.concatenate([np.asarray(t, dtype=np.int64) + int(res_ptr[k]) for k, t in enumerate(targets)])
        tgt_cx = np.repeat(np.arange(M), [len(t) for t in targets])
        self.host = [np.ascontiguousarray(a, dtype=np.int32) for a in (atom_ptr, res_ptr, tgt_res, tgt_cx)]
        self.dev = [torch.from_numpy(h).cuda() for h in self.host]
        self.xyz = torch.from_numpy(xyz).cuda()
        self.rad, self.dots = rad, dots
        self.n_targets = int(tgt_res.shape[0])
        n_bytes, _ = api.depth_workspace(self.xyz.shape[0], M, N_DOTS)
        self.work = torch.empty(n_bytes // 8, dtype=torch.int64, device="cuda")
        self.out = torch.empty(self.n_targets, dtype=torch.float64, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        q = _lib.DepthRequest()
        q.xyz, q.radii, q.dots = self.xyz.data_ptr(), rad.data_ptr(), dots.data_ptr()
        q.atom_ptr, q.res_ptr, q.target_res, q.target_complex = [t.data_ptr() for t in self.dev]
        q.host_atom_ptr, q.host_res_ptr, q.host_target_res, q.host_target_complex = [h.ctypes.data for h in self.host]
        q.n_atoms, q.n_residues, q.n_complexes = int(self.xyz.shape[0]), len(self.host[0]) - 1, M
        q.n_targets, q.n_radii = self.n_targets, int(rad.shape[0])
        q.probe, q.link, q.n_dots, q.components = PROBE, I.depth_link(N_DOTS, PROBE), N_DOTS, 0
        q.workspace, q.workspace_bytes = self.work.data_ptr(), n_bytes
        q.out, q.status = self.out.data_ptr(), self.status.data_ptr()
        self.q, self.api = q, api

    def run(self, phases=0):
        self.q.phases = phases
        self.api.depth_residues(self.q, _lib.current_stream(self.xyz))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_ab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "depth_ab.py measures on the GPU"
    api = _lib.get()
    a = depth_cases.atn()
    table, xyz4 = a["table"], a["xyz"]
    chain = a["per_atom"][0]
    per_call = max(1, I.DEPTH_WORKSPACE_BUDGET["cuda"] // (44 * table.n_atoms * N_DOTS))
    lines = ["# residue depth on %s, torch %s; 1ATN: %d atoms, %d residues per pose; %d dots per atom, probe %.1f A, link %.4f A, outer component"
             % (torch.cuda.get_device_name(0), torch.__version__, table.n_atoms, table.n_residues, N_DOTS, PROBE,
                I.depth_link(N_DOTS, PROBE)),
             "# device: HIP events around the calls of a batch, 2 warm-up rounds, median (min - max) of %d; %d poses per call"
             % (args.repeats, per_call),
             "# (the workspace is sized for every dot of every atom: %.1f MB per pose), three launches per call:"
             % (api.depth_workspace(table.n_atoms, 1, N_DOTS)[0] / 1e6),
             "# k_depth_dots a wave per atom, k_depth_components a workgroup per complex, k_depth_residues a workgroup per target"]
    rad_h = depth_ref.radii_of(table.atom_name)
    t0 = time.perf_counter()
    surfs = [depth_cases.atn_surface(m) for m in range(4)]
    want = [depth_ref.residue_depth(depth_cases.atn_x(m), table.atom_ptr, rad_h, surf=surfs[m])[0] for m in range(4)]
    t_cpu = (time.perf_counter() - t0) / 4
    got = I.residue_depth(I.AtomTable.poses(table, xyz4))
    worst = max(float(np.abs(got[m] - want[m]).max()) for m in range(4))
    rec = depth_cases.recorded()
    f = depth_cases.figures(np.concatenate([got[m][a["nodes"][m]] for m in range(4)]), np.concatenate(rec))
    lines += ["cpu depth_ref (float64 numpy, one process, surface and all residues)  %9.1f ms per pose   %8.3f poses/s" % (1e3 * t_cpu, 1.0 / t_cpu),
              "accessible dots per pose: %s; components: %s" % ([len(s["ids"]) for s in surfs], [len(np.unique(s["label"])) for s in surfs]),
              "largest |depth - depth_ref| over the %d residues of the four real poses: %.3g A (the tests allow 1e-12)" % (4 * table.n_residues, worst),
              "against the recorded node_data/depth over the 496 nodes: rms %(rms).3f A, mean %(mean).3f A, r %(r).4f, within 0.5 A %(share).4f, worst %(worst).2f A" % f,
              ""]
    print("\n".join(lines), flush=True)
    assert worst <= 1e-12
    poses = perturbed(xyz4.astype(np.float32), chain == table.chains[1], max(max(args.sizes), 4))
    rad = torch.from_numpy(I.depth_radii(table)).cuda()
    dots = torch.from_numpy(I.depth_dots(N_DOTS)).cuda()
    for M in args.sizes:
        batch = I.AtomTable.poses(table, poses[:M])
        names = ["p%05d" % m for m in range(M)]
        store = I.interface_graphs(batch, names)
        for what, targets in (("node residues", [store.get(n, "node_data/residue") for n in names]),
                              ("all residues", [np.arange(table.n_residues)] * M)):
            resident = per_call                                          # the buffers of one call at a time
            n_targets = sum(len(t) for t in targets)
            row = ["M = %5d poses, %s: %d targets (%.1f per pose), %d call(s) of at most %d poses"
                   % (M, what, n_targets, n_targets / M, -(-M // per_call), per_call)]
            total = {0: [0.0, 0.0, 0.0], 1: [0.0, 0.0, 0.0], 2: [0.0, 0.0, 0.0], 4: [0.0, 0.0, 0.0]}
            for lo in range(0, M, resident):
                calls = [DeviceCall(api, table, batch.xyz[c:c + per_call], targets[c:c + per_call], rad, dots)
                         for c in range(lo, min(M, lo + resident), per_call)]
                for phases in (0, 1, 2, 4):
                    med, tlo, thi = event_ms(lambda: [c.run(phases) for c in calls], 1 if M > 1 else 20, args.repeats)
                    for j, v in enumerate((med, tlo, thi)):
                        total[phases][j] += v
                outs = [c.out.cpu().numpy().copy() for c in calls]
                for c in calls:
                    c.run(0)
                assert all(int(c.status.cpu()[0]) == 0 for c in calls)
                assert all(o.tobytes() == c.out.cpu().numpy().tobytes() for o, c in zip(outs, calls))      # launch by launch: the same bits
                del calls
            for phases, name in ((0, "the whole call    "), (1, "k_depth_dots      "), (2, "k_depth_components"), (4, "k_depth_residues  ")):
                med, tlo, thi = total[phases]
                row.append("           %s   %10.4f ms per batch (%.4f - %.4f)   %9.2f us per pose   %10.0f poses/s%s"
                           % (name, med, tlo, thi, 1e3 * med / M, 1e3 * M / med,
                              "   depth_ref x %.0f" % ((1e3 * M / med) * t_cpu) if phases == 0 and what == "all residues" else ""))
            t0 = time.perf_counter()
            I.residue_depth(batch, residues=targets)
            row.append("           residue_depth (host arrays -> arrays, wall clock, upload and allocation included)   %9.1f ms"
                       % (1e3 * (time.perf_counter() - t0)))
            lines += row
            print("\n".join(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
