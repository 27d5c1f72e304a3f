"""Interface graphs from atom coordinates on the device (drgnn_iface.h through libdrgnn.so): the checks of
tests/test_iface.py on the MI355X, the device against the host emulation bit for bit, the graphs built from atoms
through PreCluster and a shipped checkpoint next to the reference's own, and a 64-pose batch."""
import os

import numpy as np
import pytest

import iface_cases as C
from helpers import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


@pytest.fixture(scope="module")
def batch(api):
    return C.atn_batch(api, "cuda")


@pytest.mark.parametrize("case", C.hand_cases(), ids=[n for n, _ in C.hand_cases()])
def test_hand_made_case_equals_reference_exactly(case, api):
    C.check_hand_case(case, api, "cuda")


@pytest.mark.parametrize("k", range(4))
def test_1ATN_pose_matches_the_reference_graph(k, batch):
    from deeprank_gnn_amd.dataset import GraphStore
    store, names, _ = batch
    C.assert_matches_fixture(store, names[k], GraphStore(os.path.join(GOLDEN, "fixture_1ATN.npz")))


def test_batch_chunks_and_poses_change_no_bit(batch, api):
    C.check_batch_independence(batch, api, "cuda")


def test_empty_complexes_do_not_advance_the_offsets(api):
    C.check_empty_complexes(api, "cuda")


def test_node_feature_tables(api):
    C.check_tables(api, "cuda")


def test_bad_input_is_refused_on_the_host(api):
    C.check_bad_input(api, "cuda")


def test_device_equals_emulation_bit_for_bit(batch):
    from emu_api import emu
    store, names, _ = batch
    host, _, _ = C.atn_batch(emu(), "cpu")
    C.assert_stores_identical(store, names, host, names)


def test_repeat_builds_are_bit_identical(batch, api):
    store, names, _ = batch
    again, _, _ = C.atn_batch(api, "cuda")
    C.assert_stores_identical(store, names, again, names)


def test_atoms_to_scores_end_to_end(api, tmp_path):
    C.check_end_to_end(api, "cuda", tmp_path)


def test_pose_batch_of_64_with_moved_chains(api):
    C.check_pose_batch(api, "cuda")
