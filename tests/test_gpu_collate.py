"""Resident graph set + drgnn_collate on the MI355X against the restated PyG collate (Batch.from_data_list)."""
import numpy as np
import pytest
import torch

from collate_check import check_collate, check_set_topology, ragged_graphs
from helpers import fixture_graphs, syn4_graphs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_feat", [1, 7, 32])
def test_collate_ragged(n_feat):
    check_collate(ragged_graphs(3 + n_feat, n_feat), "cuda")


def test_collate_fixture_and_synthetic():
    check_collate(fixture_graphs(), "cuda")
    check_collate(syn4_graphs(), "cuda")


def test_collate_full_size_batches_train_identically():
    """SYN graphs at BASELINE size: batches of 64 out of a resident set of 160 graphs are bit-identical to the
    host collate, and one epoch of fused training steps over them gives the same losses."""
    import copy
    import deeprank_gnn_amd.synthetic as synth
    from deeprank_gnn_amd.data import Batch
    from deeprank_gnn_amd.ginet import GINet
    from deeprank_gnn_amd.resident import ResidentGraphSet
    from deeprank_gnn_amd.trainer import FusedTrainer
    from collate_check import assert_same_batch
    graphs = [synth.make_graph(i) for i in range(160)]
    rs = ResidentGraphSet(graphs, "cuda")
    order = np.random.default_rng(0).permutation(160).tolist()
    ids_dev = rs.upload_ids(order)
    torch.manual_seed(0)
    net = GINet(32, 1, 1).cuda()
    net.dropout = 0.0
    tr_a = FusedTrainer(net, lr=1e-3, task="reg")
    tr_b = FusedTrainer(copy.deepcopy(net), lr=1e-3, task="reg")
    for lo in range(0, 160, 64):
        ids = order[lo:lo + 64]
        dev_batch = rs.batch(ids, ids_dev[lo:lo + 64])
        host_batch = Batch.from_data_list([graphs[i] for i in ids]).to("cuda")
        assert_same_batch(dev_batch, host_batch)
        la = float(tr_a.train_step(dev_batch))
        lb = float(tr_b.train_step(host_batch))
        assert la == lb


@pytest.mark.parametrize("need_weights", [False, True])
def test_topology_from_the_resident_set(need_weights):
    import deeprank_gnn_amd.synthetic as synth
    check_set_topology(ragged_graphs(4, 6), "cuda", need_weights=need_weights, batch_size=4)
    check_set_topology(fixture_graphs(), "cuda", need_weights=need_weights, batch_size=3)
    check_set_topology([synth.make_graph(i) for i in range(96)], "cuda", need_weights=need_weights, batch_size=64)


# ---- beyond nine graphs: the cases of collate_cases.py, shared with tests/test_emu_collate.py ---------------------------
import collate_cases as CC


@pytest.mark.parametrize("B", CC.SLOT_COUNTS)
def test_collate_at_slot_count_edges(B):
    CC.check_slot_counts(B, None, "cuda")


@pytest.mark.parametrize("n_feat", CC.ROW_FEATS)
def test_collate_row_copy_paths(n_feat):
    CC.check_row_copies(n_feat, None, "cuda")


@pytest.mark.parametrize("field", ["edge_attr", "y", "cluster1", "cluster0"])
def test_collate_without_one_field(field):
    CC.check_without(field, None, "cuda")


def test_collate_int64_targets_and_replaced_targets():
    CC.check_int64_targets(None, "cuda")


@pytest.mark.parametrize("batch_size", CC.OFFSET_BATCH_SIZES)
def test_batch_offsets(batch_size):
    CC.check_batch_offsets(batch_size, None, "cuda")


def test_batch_offsets_without_ids():
    CC.check_batch_offsets_no_ids(None, "cuda")


def test_batch_offsets_capacity():
    CC.check_batch_offsets_capacity(None, "cuda")


@pytest.mark.parametrize("need_weights", [False, True])
@pytest.mark.parametrize("which,batch_size", [("tiny", 65), ("tiny", 1025), ("mixed", 65)])
def test_topology_from_the_resident_set_at_slot_count_edges(which, batch_size, need_weights):
    CC.check_topology(which, batch_size, need_weights, None, "cuda")


@pytest.mark.parametrize("which", range(CC.N_OUTSIDE_LISTS))
def test_collate_ids_outside_the_set(which):
    CC.check_collate_outside_ids(which, None, "cuda")


def test_batch_offsets_ids_outside_the_set():
    CC.check_offsets_outside_ids(None, "cuda")


def test_batch_offsets_ids_outside_the_declared_set():
    CC.check_offsets_outside_declared_set(None, "cuda")


def test_collate_refusals():
    CC.check_collate_refusals(None, "cuda")


def test_batch_offsets_refusals():
    CC.check_offsets_refusals(None, "cuda")


def test_upload_ids_out_of_range():
    CC.check_upload_ids_range(None, "cuda")


def test_upload_ids_staging_ring():
    CC.check_upload_ids_ring("cuda")


def test_resident_set_image_round_trip(tmp_path):
    CC.check_image_round_trip(str(tmp_path / "set.npz"), None, "cuda")
