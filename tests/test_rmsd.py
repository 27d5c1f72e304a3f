"""Pairwise pose RMSD and RMSD clustering of docking poses (drgnn_rmsd.h; deeprank_gnn_amd.interface.select_atoms,
pose_rmsd, interface_residues, cluster_poses_rmsd) on the host-emulation build: the two statements of the rule in
tests/rmsd_ref.py against each other (that gap sets the tolerance), then the kernels against the explicit Kabsch form on
squared RMSD: 1ATN under every kind, hand-made atoms on the 1/8 A grid, selections around the staging chunk, batches
across the tile edge, rectangular blocks, independence of batch / chunk / place / run, the cross-check against
docking_scores; the clustering by exact equality on the same matrix; capacities, refusals, the empty batch and the
ranking.  CPU only; tests/test_gpu_rmsd.py runs the same checks on the device."""
import pytest

import rmsd_cases as C


@pytest.fixture(scope="module")
def api():
    from emu_api import emu
    return emu()


def test_the_two_forms_of_the_rule_agree():
    """on the reference alone: explicit Kabsch against the moment form, the k the tolerance is 16 times of"""
    C.check_forms_agree()


def test_the_family_has_clusters_leftovers_and_no_pair_at_the_cutoff():
    C.check_family_ref()


def test_1ATN_poses_under_every_kind(api):
    C.check_atn(api, "cpu")


def test_hand_made_atoms_have_their_known_answers(api):
    C.check_hand(api, "cpu")


def test_selection_sizes_around_the_staging_chunk(api):
    C.check_stage_sizes(api, "cpu")


@pytest.mark.parametrize("M", C.BATCH_SIZES)
def test_pose_batches_across_the_tile_edge(M, api):
    C.check_batch(api, "cpu", M)


def test_results_do_not_depend_on_batch_chunk_side_place_or_run(api):
    C.check_independence(api, "cpu")


def test_pose_rmsd_splits_at_the_capacity(api, monkeypatch):
    C.check_split_at_capacity(api, "cpu", monkeypatch)


def test_ligand_rmsd_agrees_with_docking_scores(api):
    C.check_against_scores(api, "cpu")


def test_hand_written_matrices_cluster_as_the_rule_says(api):
    C.check_hand_matrices(api, "cpu")


def test_the_family_clusters_as_the_reference_does(api):
    C.check_family_clusters(api, "cpu")


def test_interface_residues(api):
    C.check_interface_residues(api, "cpu")


def test_capacity_is_refused_not_wrong(api):
    C.check_capacity(api, "cpu")


def test_empty_batch(api):
    C.check_empty_batch(api, "cpu")


def test_value_errors():
    C.check_value_errors()


@pytest.mark.parametrize("name", C.refusal_names())
def test_bad_requests_are_refused_before_a_launch(name, api):
    C.check_refusal(api, "cpu", name)
