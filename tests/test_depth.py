"""Residue depth (drgnn_depth.h, deeprank_gnn_amd.interface.residue_depth) on the host-emulation build: the float64
statement of the rule in tests/depth_ref.py against the values the reference recorded for the four 1ATN poses, then the
kernels against depth_ref (accessible dots, component labels, the component kept, depths) on 1ATN, on hand-made atoms and
at several dot counts, batch / chunk / target-list independence, the capacity, refusals, and the way through
interface_graphs, GraphDataSet, interface_resident_set and a shipped checkpoint.  CPU only; whole poses run at 32 dots
per atom here and at 192 on the device (tests/test_gpu_depth.py)."""
import pytest

import depth_cases as C


@pytest.fixture(scope="module")
def api():
    from emu_api import emu
    return emu()


def test_depth_ref_against_the_recorded_depth():
    """all 496 nodes of the four poses at the defaults; no kernel: this pins the rule.  Measured: rms 0.152 A, mean
    -0.027 A, r 0.990, 99.4 % within 0.5 A, worst 1.72 A; with every component kept r drops to 0.938"""
    C.check_ref_against_recorded()


def test_1ATN_nodes_equal_depth_ref(api):
    C.check_atn(api, "cpu", 0, n_dots=32, subset=C.emu_subset())


@pytest.mark.parametrize("name", C.HAND_CASES)
def test_hand_made_atoms_equal_depth_ref(name, api):
    C.check_hand_case(name, api, "cpu")


@pytest.mark.parametrize("n_dots", C.DOT_COUNTS)
def test_dot_counts(n_dots, api):
    C.check_dot_count(api, "cpu", n_dots)


def test_results_do_not_depend_on_batch_chunk_targets_or_run(api):
    C.check_independence(api, "cpu")


def test_value_errors():
    C.check_value_errors()


def test_capacity_is_refused_not_wrong(api):
    C.check_capacity(api, "cpu")


def test_empty_target_list(api):
    C.check_empty_targets(api, "cpu")


@pytest.mark.parametrize("name", C.refusal_names())
def test_bad_requests_are_refused_before_a_launch(name, api):
    C.check_refusal(api, "cpu", name)


def test_interface_graphs_with_depth(api, tmp_path):
    C.check_graphs(api, "cpu", tmp_path, nn_kw={"_api": api, "device": "cpu"}, n_dots=32)


def test_resident_set_with_depth_equals_the_store_path(api):
    C.check_resident_set(api, "cpu", poses=(0,), n_dots=32)
