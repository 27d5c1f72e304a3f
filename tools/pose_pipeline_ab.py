"""Time the two ways from pose coordinates to scores on the device, in one run:

  A  interface_graphs(bsa=True, hse=True) -> GraphDataSet -> PreCluster -> ResidentGraphSet -> Ensemble.predict
  B  interface_resident_set -> the same Ensemble.predict

usage: python tools/pose_pipeline_ab.py [--repeats 5] [--sizes 64 256 1024] [--out profiles/pose_pipeline_ab.txt]
Poses: the 1ATN topology (tests/golden/atoms_1ATN.npz, names from scores_1ATN.npz), the four reference poses cycled with
the rigid chain-B shifts of tests/iface_cases.check_pose_batch (the pattern repeats every 64 poses).  Node features type,
polarity, bsa, hse (28 columns), edge feature dist, Markov clustering; two seeded GINet members.
Timed, wall clock, every window closed by a device synchronise: poses -> resident set, and poses -> scores.  Two warm-up
rounds of both paths, then the paths alternate; median (min - max) over the repeats.  The pack launch alone: HIP events
around 20 back-to-back drgnn_iface_pack calls on the device-resident output of one build, next to the bytes the launch
must move, computed from the shapes.  Needs the GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from deeprank_gnn_amd import Ensemble, GINet, _lib                               # noqa: E402
from deeprank_gnn_amd import interface as I                                      # noqa: E402
from deeprank_gnn_amd.clustering import PreCluster                               # noqa: E402
from deeprank_gnn_amd.dataset import GraphDataSet                                # noqa: E402
from deeprank_gnn_amd.resident import ResidentGraphSet                           # noqa: E402
import pack_cases                                                                # noqa: E402
import score_cases                                                               # noqa: E402

FEATURES = ["type", "polarity", "bsa", "hse"]


def path_a(poses, names, ens):
    store = I.interface_graphs(poses, names, bsa=True, hse=True)
    ds = GraphDataSet(store, node_feature=FEATURES, edge_feature=["dist"])
    PreCluster(ds, method="mcl")
    rs = ResidentGraphSet(ds, "cuda")
    torch.cuda.synchronize()
    t = time.perf_counter()
    pred = ens.predict(rs)
    torch.cuda.synchronize()
    return t, pred


def path_b(poses, names, ens):
    rs = I.interface_resident_set(poses, names, node_feature=FEATURES)
    torch.cuda.synchronize()
    t = time.perf_counter()
    pred = ens.predict(rs)
    torch.cuda.synchronize()
    return t, pred


def timed(path, poses, names, ens):
    """(ms poses -> resident set, ms poses -> scores, predictions)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t1, pred = path(poses, names, ens)
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t0), pred


def stat(v):
    return "%9.2f ms (%.2f - %.2f)" % (float(np.median(v)), min(v), max(v))


def pack_alone(api, table, xyz_grouped, calls=20):
    """(us per drgnn_iface_pack launch, bytes it must move, (N, E, Ei)) on the output of one build of these poses"""
    part = [(table, x) for x in xyz_grouped]
    xyz, atom_ptr, res_ptr, split, res_type = I._ragged(part)
    built, ptrs = I.build_ragged_device(api, xyz, atom_ptr, res_ptr, split, res_type, device="cuda")
    N, E, Ei = (int(v) for v in ptrs[:, -1].cpu())
    M = len(part)
    dev = ptrs.device
    type_table = torch.from_numpy(I.pack_type_table()).to(dev)
    rows = torch.zeros((N, 3), dtype=torch.float64, device=dev)          # (the values do not matter to the launch's time)
    cols = I._pack_columns(FEATURES, {})
    F = int(cols.shape[0])
    q, out, keep = I.pack_request(built, ptrs, cols, len(atom_ptr) - 1, type_table, rows, rows, None, 1)
    stream = _lib.current_stream(ptrs)
    for _ in range(3):
        api.iface_pack(q, stream)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        api.iface_pack(q, stream)
    b.record()
    torch.cuda.synchronize()
    read = 12 * (M + 1) + 4 * N + 8 * N + 24 * N + 20 * E + 16 * Ei + 8 * F + 4 * type_table.numel()
    write = 4 * N * F + 8 * N + 32 * E + 8 * E + 32 * Ei
    return 1e3 * a.elapsed_time(b) / calls, read + write, (N, E, Ei)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_pipeline_ab.txt"))
    args = ap.parse_args()
    api = _lib.get()
    case, _ = score_cases.atn()
    table = case.table
    torch.manual_seed(3)
    states = [{k: v.clone() for k, v in GINet(28, 1, 1).state_dict().items()} for _ in range(2)]
    ens = Ensemble(GINet, states, device="cuda")
    lines = ["# poses -> resident set -> scores on %s, torch %s; 1ATN: %d residues, %d atoms per pose"
             % (torch.cuda.get_device_name(0), torch.__version__, table.n_residues, table.n_atoms),
             "# A: interface_graphs(bsa, hse) -> GraphDataSet -> PreCluster -> ResidentGraphSet; B: interface_resident_set",
             "# node features %s (28 columns), dist, mcl; Ensemble.predict of 2 GINet members" % ", ".join(FEATURES),
             "# wall clock, every window ends in a device synchronise; 2 warm-up rounds, the paths alternate, median "
             "(min - max) of %d" % args.repeats, ""]
    for n in args.sizes:
        _, xyz, names = pack_cases.pose_batch(n)
        poses = I.AtomTable.poses(table, xyz)
        for _ in range(2):
            timed(path_a, poses, names, ens)
            timed(path_b, poses, names, ens)
        got = {"A": ([], []), "B": ([], [])}
        for _ in range(max(args.repeats, 5)):
            for key, path in (("A", path_a), ("B", path_b)):
                s, p, pred = timed(path, poses, names, ens)
                got[key][0].append(s)
                got[key][1].append(p)
                got[key] = got[key][:2] + (pred,)
        same = bool(torch.equal(got["A"][2], got["B"][2]))
        us, moved, (N, E, Ei) = pack_alone(api, table, poses.xyz)
        lines.append("%d poses: %d nodes, %d interface edges, %d internal edges" % (n, N, E, Ei))
        for key in ("A", "B"):
            lines.append("  %s  poses -> resident set %s   poses -> scores %s" % (key, stat(got[key][0]), stat(got[key][1])))
        ra = float(np.median(got["A"][0])) / float(np.median(got["B"][0]))
        rb = float(np.median(got["A"][1])) / float(np.median(got["B"][1]))
        lines.append("  A / B  resident set %.1f x   scores %.1f x   predictions bit-equal: %s" % (ra, rb, same))
        lines.append("  drgnn_iface_pack alone  %.1f us per launch, %.2f MB to move: %.0f GB/s" % (us, moved / 1e6, moved / us / 1e3))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
