"""Time the device build of interface graphs (drgnn_iface_count + drgnn_iface_fill) next to the same rule in numpy on
the CPU, in one run, on the four reference poses of 1ATN (tests/golden/atoms_1ATN.npz: 627 residues, 6 003 atoms).

usage: python tools/iface_ab.py [--repeats 10] [--out profiles/iface_graphs.txt]
  case 1  the four poses as tables of their own, replicated to 256 complexes (the general, ragged input)
  case 2  one AtomTable.poses batch of 64 poses
Device rows: HIP events around the two library calls on device-resident inputs and a preallocated workspace (the read
of the three totals between them included), 2 warm-up builds, median over the repeats; `interface_graphs` is the
whole Python call from host arrays to a GraphStore (wall clock).  Kernel rows: the duration of each launch of one
build, from torch.profiler, when it yields device events.  The CPU row runs `numpy_rule` below, the rule of
tests/iface_ref.py vectorised over the atoms of one complex, on the four poses.  Needs the GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deeprank_gnn_amd import _lib                                                # noqa: E402
from deeprank_gnn_amd import interface as I                                      # noqa: E402


def numpy_rule(xyz, atom_ptr, split, res_type, cut=8.5, icut=3.0):
    """(nodes, interface pairs with their dist, internal pairs with their dist) of one complex, float64"""
    xyz = np.asarray(xyz, dtype=np.float64)
    atom_ptr = np.asarray(atom_ptr, dtype=np.int64)

    def min_d2(xa, pa, xb, pb):
        d2 = np.zeros((xa.shape[0], xb.shape[0]))
        for k in range(3):
            d = xa[:, None, k] - xb[None, :, k]
            d2 += d * d
        return np.minimum.reduceat(np.minimum.reduceat(d2, pa[:-1], axis=0), pb[:-1], axis=1)
    c = atom_ptr[split]
    m = min_d2(xyz[:c], atom_ptr[:split + 1], xyz[c:], atom_ptr[split:] - c)
    ok = (m < cut * cut) & (res_type[:split, None] >= 0) & (res_type[None, split:] >= 0)
    is_node = np.concatenate((ok.any(axis=1), ok.any(axis=0)))
    nodes = np.flatnonzero(is_node)
    local = np.cumsum(is_node) - 1
    ia, ib = np.nonzero(ok)
    edges, dist = np.stack((local[ia], local[split + ib]), axis=1), np.sqrt(m[ia, ib])
    pos = np.add.reduceat(xyz, atom_ptr[:-1], axis=0)[nodes] / np.diff(atom_ptr)[nodes, None]
    internal, idist = [], []
    for lo, hi in ((0, split), (split, len(atom_ptr) - 1)):
        sel = nodes[(nodes >= lo) & (nodes < hi)]
        if sel.size < 2:
            continue
        idx = np.concatenate([np.arange(atom_ptr[r], atom_ptr[r + 1]) for r in sel])
        ptr = np.concatenate(([0], np.cumsum(atom_ptr[sel + 1] - atom_ptr[sel])))
        mi = min_d2(xyz[idx], ptr, xyz[idx], ptr)
        i, j = np.nonzero(np.triu(mi < icut * icut, k=1))
        internal.append(np.stack((local[sel[i]], local[sel[j]]), axis=1))
        idist.append(np.sqrt(mi[i, j]))
    return nodes, pos, edges, dist, internal, idist


class DeviceBuild(object):
    """the two library calls on device-resident inputs, buffers allocated once"""

    def __init__(self, api, ragged):
        xyz, atom_ptr, res_ptr, split, res_type = ragged
        self.api = api
        self.M, R = len(res_ptr) - 1, len(atom_ptr) - 1
        self.host = [np.ascontiguousarray(a, dtype=np.int32) for a in (atom_ptr, res_ptr, split)]
        self.dev = [torch.from_numpy(a).cuda() for a in (xyz, *self.host, res_type)]
        rp, rs = self.host[1].astype(np.int64), self.host[2].astype(np.int64)
        nbytes = api.iface_workspace_bytes(self.M, int((rs - rp[:-1]).max()), int((rp[1:] - rs).max()), R)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.ptrs = torch.zeros((3, self.M + 1), dtype=torch.int32, device="cuda")
        q = _lib.IfaceRequest()
        q.xyz, q.atom_ptr, q.res_ptr, q.res_split, q.res_type = [t.data_ptr() for t in self.dev]
        q.host_atom_ptr, q.host_res_ptr, q.host_res_split = [h.ctypes.data for h in self.host]
        q.n_atoms, q.n_residues, q.n_complexes = int(xyz.shape[0]), R, self.M
        q.contact_distance, q.internal_contact_distance = 8.5, 3.0
        q.workspace, q.workspace_bytes = self.ws.data_ptr(), nbytes
        q.node_ptr, q.edge_ptr, q.iedge_ptr = [self.ptrs[k].data_ptr() for k in range(3)]
        self.q, self.out, self.workspace_bytes = q, None, nbytes

    def run(self):
        stream = _lib.current_stream(self.ws)
        self.api.iface_count(self.q, stream)
        N, E, Ei = (int(v) for v in self.ptrs[:, -1].cpu())
        if self.out is None:
            i32, f32, i64 = torch.int32, torch.float32, torch.int64
            self.out = [torch.empty(N, dtype=i32, device="cuda"), torch.empty((N, 3), dtype=f32, device="cuda"),
                        torch.empty(N, dtype=i32, device="cuda"), torch.empty(N, dtype=i32, device="cuda"),
                        torch.empty((E, 2), dtype=i64, device="cuda"), torch.empty(E, dtype=f32, device="cuda"),
                        torch.empty((Ei, 2), dtype=i64, device="cuda"), torch.empty(Ei, dtype=f32, device="cuda")]
        self.api.iface_fill(self.q, N, E, Ei, *self.out, stream)
        return N, E, Ei


def event_ms(fn, repeats, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def kernel_rows(fn):
    """[(kernel name, microseconds)] of the launches of one call, in launch order; [] when the profiler yields none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if "k_iface" in e.name]
        ev.sort(key=lambda e: e.time_range.start)
        return [(e.name.split("(")[0], float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0))) for e in ev]
    except Exception as exc:                       # the rows are an extra: the figures above do not depend on them
        return [("profiler unavailable: %s" % (exc,), 0.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iface_graphs.txt"))
    args = ap.parse_args()
    api = _lib.get()
    with np.load(os.path.join(ROOT, "tests", "golden", "atoms_1ATN.npz")) as z:
        n = np.diff(z["atom_ptr"])
        chain = np.repeat(np.array(["A", "B"])[z["res_chain"]], n)
        seq, name = np.repeat(z["res_seq"], n), np.repeat(z["res_names"][z["res_name_index"]], n)
        xyz = z["xyz_milli"] / 1000.0
    tables = [I.AtomTable(chain, seq, name, xyz[m]) for m in range(4)]
    t = tables[0]
    lines = ["# interface graphs from atoms on %s, torch %s; 1ATN: %d residues (%d + %d), %d atoms per complex"
             % (torch.cuda.get_device_name(0), torch.__version__, t.n_residues, t.split, t.n_residues - t.split, t.n_atoms),
             "# device: HIP events, 2 warm-up builds, median of %d; cut-offs 8.5 / 3.0 A" % args.repeats]
    # the CPU side: the four poses, one after another
    t0 = time.perf_counter()
    cpu = [numpy_rule(tb.xyz, tb.atom_ptr, tb.split, tb.res_type) for tb in tables]
    t_cpu = (time.perf_counter() - t0) / 4
    lines.append("cpu numpy rule (float64, one core)      %9.1f ms per graph   %10.1f graphs/s" % (1e3 * t_cpu, 1.0 / t_cpu))
    cases = [("case 1: 4 poses x 64 = 256 tables", [(tables[k % 4], tables[k % 4].xyz) for k in range(256)]),
             ("case 2: AtomTable.poses, 64 poses", I._complexes(I.AtomTable.poses(t, xyz[np.arange(64) % 4])))]
    for title, cx in cases:
        M = len(cx)
        build = DeviceBuild(api, I._ragged(cx))
        N, E, Ei = build.run()
        want = [sum(len(cpu[k % 4][0]) for k in range(M)), sum(len(cpu[k % 4][2]) for k in range(M)),
                sum(sum(len(p) for p in cpu[k % 4][4]) for k in range(M))]
        assert [N, E, Ei] == want, ("the device and the CPU rule disagree", [N, E, Ei], want)
        ms = event_ms(build.run, args.repeats)
        ms_count = event_ms(lambda: api.iface_count(build.q, _lib.current_stream(build.ws)), args.repeats)
        names = ["g%d" % k for k in range(M)]
        items = [tb for tb, _ in cx] if "256" in title else I.AtomTable.poses(t, xyz[np.arange(64) % 4])
        I.interface_graphs(items, names)
        t0 = time.perf_counter()
        I.interface_graphs(items, names)
        t_all = time.perf_counter() - t0
        lines += ["", "%s: %d nodes, %d interface edges, %d internal edges; workspace %.1f MiB" % (title, N, E, Ei, build.workspace_bytes / 2 ** 20),
                  "  count + read of the totals + fill     %9.3f ms per build   %10.0f graphs/s" % (ms, 1e3 * M / ms),
                  "  count alone (5 launches)              %9.3f ms" % ms_count,
                  "  interface_graphs (host arrays -> GraphStore, wall clock)  %9.1f ms   %10.0f graphs/s" % (1e3 * t_all, M / t_all),
                  "  device build against the CPU rule     %9.0f x" % ((1e3 * M / ms) * t_cpu)]
        for kname, us in kernel_rows(build.run):
            lines.append("    %-28s %10.1f us" % (kname, us))
        print("\n".join(lines[-12:]), flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
