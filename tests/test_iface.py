"""Interface graphs from atom coordinates (drgnn_iface.h, deeprank_gnn_amd.interface) on the host-emulation build:
hand-made complexes against the float64 reference of tests/iface_ref.py bit for bit, the four reference poses of
1ATN against the graphs the reference generated from them, batch / chunk / poses independence, the node feature
tables, argument errors.  CPU only; tests/test_gpu_iface.py runs the same checks on the device."""
import os

import numpy as np
import pytest

import iface_cases as C
from helpers import GOLDEN


@pytest.fixture(scope="module")
def api():
    from emu_api import emu
    return emu()


@pytest.fixture(scope="module")
def batch(api):
    return C.atn_batch(api, "cpu")


@pytest.mark.parametrize("case", C.hand_cases(), ids=[n for n, _ in C.hand_cases()])
def test_hand_made_case_equals_reference_exactly(case, api):
    C.check_hand_case(case, api, "cpu")


@pytest.mark.parametrize("k", range(4))
def test_1ATN_pose_matches_the_reference_graph(k, batch):
    from deeprank_gnn_amd.dataset import GraphStore
    store, names, _ = batch
    C.assert_matches_fixture(store, names[k], GraphStore(os.path.join(GOLDEN, "fixture_1ATN.npz")))


def test_1ATN_counts(batch):
    store, names, _ = batch
    got = [(store.get(m, "node_data/pos").shape[0], store.get(m, "edge_index").shape[0],
            store.get(m, "internal_edge_index").shape[0]) for m in names[:4]]
    assert got == [(132, 374, 230), (132, 330, 232), (137, 386, 245), (95, 201, 161)]


def test_1ATN_equals_float64_reference_in_structure(batch):
    """nodes and both edge lists equal the numpy reference's exactly, canonical order included; distances within fp32"""
    store, names, items = batch
    t, xyz, _ = C.atn()
    for k in range(4):
        ref = C.reference_tree(t, items[0].xyz[k].astype(np.float64))
        for key in ("edge_index", "internal_edge_index", "node_data/residue", "node_data/chain"):
            np.testing.assert_array_equal(store.get(names[k], key), ref[key])
        for key in ("edge_data/dist", "internal_edge_data/dist", "node_data/pos"):
            assert np.abs(store.get(names[k], key).astype(np.float64) - ref[key]).max() <= 4e-6


def test_batch_chunks_and_poses_change_no_bit(batch, api):
    C.check_batch_independence(batch, api, "cpu")


def test_empty_complexes_do_not_advance_the_offsets(api):
    C.check_empty_complexes(api, "cpu")


def test_node_feature_tables(api):
    C.check_tables(api, "cpu")


def test_bad_input_is_refused_on_the_host(api):
    C.check_bad_input(api, "cpu")


def test_atom_table_groups_an_interleaved_input():
    """atoms of a residue scattered over the input, chain B first: residues by (chain, first appearance), atoms of a
    residue in input order; other chains and their atoms dropped"""
    from deeprank_gnn_amd.interface import AtomTable
    chain = np.array(list("BABAXBA"))
    seq = np.array([7, 3, 7, 1, 1, 2, 3])
    name = np.array(["SER", "GLY", "SER", "ALA", "HOH", "UNK", "GLY"])
    xyz = np.arange(21, dtype=np.float64).reshape(7, 3)
    t = AtomTable(chain, seq, name, xyz)
    assert t.order.tolist() == [1, 6, 3, 0, 2, 5] and t.atom_ptr.tolist() == [0, 2, 3, 5, 6] and t.split == 2
    assert t.res_seq.tolist() == [3, 1, 7, 2] and t.res_chain.tolist() == [0, 0, 1, 1]
    assert t.res_type.tolist() == [10, 8, 4, -1]
    p = AtomTable.poses(t, np.stack((xyz, xyz + 1.0)))
    assert p.xyz.shape == (2, 6, 3) and np.array_equal(p.xyz[1], (xyz + 1.0)[t.order].astype(np.float32))


def test_store_feeds_dataset_and_precluster(batch, api):
    """the result is a GraphStore that GraphDataSet and PreCluster take as it is; attach_residue_features gathers"""
    from deeprank_gnn_amd.clustering import PreCluster
    from deeprank_gnn_amd.dataset import GraphDataSet
    from deeprank_gnn_amd.interface import attach_residue_features
    store, names, _ = batch
    t, _, mols = C.atn()
    per_residue = np.arange(t.n_residues * 2, dtype=np.float64).reshape(-1, 2)
    attach_residue_features(store, "pssm2", per_residue)
    ds = GraphDataSet(store, node_feature=["type", "polarity", "charge", "pssm2"], edge_feature=["dist"], index=[0, 1, 2, 3])
    g = ds[2]
    assert g.x.shape == (137, 27) and g.edge_index.shape[1] in (386, 2 * 386)
    np.testing.assert_array_equal(store.get(mols[2], "node_data/pssm2"), per_residue[store.get(mols[2], "node_data/residue")])
    PreCluster(ds, method='louvain', api=api, device='cpu')
    assert store.get(mols[0], "clustering/louvain/depth_0").shape == (132,)


def test_atoms_to_scores_end_to_end(api, tmp_path):
    C.check_end_to_end(api, "cpu", tmp_path, {"_api": api, "device": "cpu"})


def test_pose_batch_of_64_with_moved_chains(api):
    C.check_pose_batch(api, "cpu")
