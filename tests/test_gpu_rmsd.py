"""Pairwise pose RMSD and RMSD clustering of docking poses on the device (drgnn_rmsd.h through libdrgnn.so): the checks
of tests/test_rmsd.py on the MI355X.  The device need not equal the emulation bit for bit (FMA contraction differs); each
holds the bound against the explicit Kabsch form of tests/rmsd_ref.py, and each is bit for bit its own from run to run."""
import pytest

import rmsd_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


def test_1ATN_poses_under_every_kind(api):
    C.check_atn(api, "cuda")


def test_hand_made_atoms_have_their_known_answers(api):
    C.check_hand(api, "cuda")


def test_selection_sizes_around_the_staging_chunk(api):
    C.check_stage_sizes(api, "cuda")


@pytest.mark.parametrize("M", C.BATCH_SIZES)
def test_pose_batches_across_the_tile_edge(M, api):
    C.check_batch(api, "cuda", M)


def test_results_do_not_depend_on_batch_chunk_side_place_or_run(api):
    C.check_independence(api, "cuda")


def test_pose_rmsd_splits_at_the_capacity(api, monkeypatch):
    C.check_split_at_capacity(api, "cuda", monkeypatch)


def test_ligand_rmsd_agrees_with_docking_scores(api):
    C.check_against_scores(api, "cuda")


def test_hand_written_matrices_cluster_as_the_rule_says(api):
    C.check_hand_matrices(api, "cuda")


def test_the_family_clusters_as_the_reference_does(api):
    C.check_family_clusters(api, "cuda")


def test_interface_residues(api):
    C.check_interface_residues(api, "cuda")


def test_capacity_is_refused_not_wrong(api):
    C.check_capacity(api, "cuda")


def test_empty_batch(api):
    C.check_empty_batch(api, "cuda")


@pytest.mark.parametrize("name", C.refusal_names())
def test_bad_requests_are_refused_before_a_launch(name, api):
    C.check_refusal(api, "cuda", name)
