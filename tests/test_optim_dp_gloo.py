"""The optimiser options on the data-parallel route, world_size 2 over gloo on the CPU (kernels: host-emulation build):
gradient launches -> ONE all-reduce -> the flat Adam launch with decoupled weight decay, a learning-rate table and clipping
by the norm of the ALL-REDUCED gradient.  Checked against a single process on the union of the shards, test_dp_gloo.py's
harness and tolerance."""
import os
import tempfile

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_dp_gloo import _graphs, _make_net

SIZES = [7, 4]
TABLE = [0.02, 0.005]


def _options(max_norm):
    return dict(weight_decay=0.05, decoupled_weight_decay=True, max_grad_norm=max_norm, lr_schedule=TABLE)


def _worker(rank, world, init_file, max_norm, out_dir):
    from emu_api import emu
    from deeprank_gnn_amd.data import Batch
    from deeprank_gnn_amd.trainer import FusedTrainer
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + init_file, rank=rank, world_size=world)
    graphs = _graphs(sum(SIZES))
    lo = sum(SIZES[:rank])
    batch = Batch.from_data_list(graphs[lo:lo + SIZES[rank]])
    tr = FusedTrainer(_make_net("GINet"), lr=0.01, api=emu(), **_options(max_norm))
    norms = []
    for _ in range(2):
        tr.train_step(batch, n_global=sum(SIZES))
        norms.append(float(tr.grad_norm))
    np.save(os.path.join(out_dir, "p%d.npy" % rank), tr.flat_p.numpy())
    np.save(os.path.join(out_dir, "g%d.npy" % rank), tr.flat_g.numpy())
    np.save(os.path.join(out_dir, "n%d.npy" % rank), np.asarray(norms))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_by_the_all_reduced_norm():
    from emu_api import emu
    from deeprank_gnn_amd.data import Batch
    from deeprank_gnn_amd.trainer import FusedTrainer
    emu()
    union = Batch.from_data_list(_graphs(sum(SIZES)))
    probe = FusedTrainer(_make_net("GINet"), lr=0.01, api=emu())
    probe.compute_gradients(union)
    max_norm = 0.5 * float(np.sqrt(np.sum(probe.flat_g.numpy().astype(np.float64) ** 2)))      # active at the first step
    with tempfile.TemporaryDirectory() as tmp:
        init_file = os.path.join(tmp, "rendezvous")
        mp.spawn(_worker, args=(2, init_file, max_norm, tmp), nprocs=2, join=True)
        p, g, n = ([np.load(os.path.join(tmp, "%s%d.npy" % (k, r))) for r in range(2)] for k in "pgn")
    np.testing.assert_array_equal(p[0], p[1])           # replicas stay bit-identical
    np.testing.assert_array_equal(g[0], g[1])
    np.testing.assert_array_equal(n[0], n[1])
    tr = FusedTrainer(_make_net("GINet"), lr=0.01, api=emu(), **_options(max_norm))
    norms = []
    for _ in range(2):
        tr.train_step(union)
        norms.append(float(tr.grad_norm))
    assert norms[0] > max_norm
    # the norm every rank clipped by is the union's, not its shard's
    np.testing.assert_allclose(n[0], norms, rtol=1e-4)
    scale = max(1.0, float(np.abs(tr.flat_g.numpy()).max()))
    np.testing.assert_allclose(g[0], tr.flat_g.numpy(), rtol=1e-4, atol=1e-5 * scale)
    np.testing.assert_allclose(p[0], tr.flat_p.numpy(), rtol=1e-4, atol=1e-5)


def _worker_epoch(rank, world, init_file, max_norm, out_dir):
    from emu_api import emu
    from deeprank_gnn_amd.resident import ResidentGraphSet
    from deeprank_gnn_amd.trainer import FusedTrainer
    torch.set_num_threads(1)
    dist.init_process_group("gloo", init_method="file://" + init_file, rank=rank, world_size=world)
    rs = ResidentGraphSet(_graphs(19), "cpu", api=emu())
    tr = FusedTrainer(_make_net("GINet"), lr=0.01, api=emu(), seed=5, **_options(max_norm))
    tr.EPOCH_CHUNK = 2
    mine = [g for lo in range(0, 19, 4) for g in range(lo, min(lo + 4, 19))[2 * rank:2 * rank + 2]]
    done = tr.train_epoch(rs, mine, 2, dp_global_sizes=[4, 4, 4, 4, 3])
    assert done is not None and int(tr.step) == 5
    np.save(os.path.join(out_dir, "p%d.npy" % rank), tr.flat_p.numpy())
    np.save(os.path.join(out_dir, "g%d.npy" % rank), tr.flat_g.numpy())
    np.save(os.path.join(out_dir, "n%d.npy" % rank), tr.grad_norm.numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_native_epoch_loop_under_data_parallel_with_the_options():
    """the loop's data-parallel branch: gradient launches -> the exchange -> drgnn_adam_step_opt, 5 global mini-batches
    (4, 4, 4, 4, 3 graphs) in pieces of 2, against one process stepping the same mini-batches"""
    from emu_api import emu
    from deeprank_gnn_amd.data import Batch
    from deeprank_gnn_amd.trainer import FusedTrainer
    emu()
    graphs = _graphs(19)
    probe = FusedTrainer(_make_net("GINet"), lr=0.01, api=emu(), seed=5)
    probe.compute_gradients(Batch.from_data_list(graphs[:4]))
    max_norm = 0.5 * float(np.sqrt(np.sum(probe.flat_g.numpy().astype(np.float64) ** 2)))
    with tempfile.TemporaryDirectory() as tmp:
        init_file = os.path.join(tmp, "rendezvous")
        mp.spawn(_worker_epoch, args=(2, init_file, max_norm, tmp), nprocs=2, join=True)
        p, g, n = ([np.load(os.path.join(tmp, "%s%d.npy" % (k, r))) for r in range(2)] for k in "pgn")
    np.testing.assert_array_equal(p[0], p[1])
    np.testing.assert_array_equal(n[0], n[1])
    tr = FusedTrainer(_make_net("GINet"), lr=0.01, api=emu(), seed=5, **_options(max_norm))
    clipped = 0
    for lo in range(0, 19, 4):
        tr.train_step(Batch.from_data_list(graphs[lo:lo + 4]))
        clipped += float(tr.grad_norm) > max_norm
    assert clipped >= 1
    np.testing.assert_allclose(n[0], tr.grad_norm.numpy(), rtol=1e-4)       # the last mini-batch's all-reduced norm
    scale = max(1.0, float(np.abs(tr.flat_g.numpy()).max()))
    np.testing.assert_allclose(g[0], tr.flat_g.numpy(), rtol=1e-4, atol=1e-5 * scale)
    np.testing.assert_allclose(p[0], tr.flat_p.numpy(), rtol=1e-4, atol=1e-5)
