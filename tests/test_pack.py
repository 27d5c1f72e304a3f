"""interface_resident_set and drgnn_iface_pack (drgnn_pack.h) on the host-emulation build: the checks of
tests/pack_cases.py against the existing path through host trees.  The emulated bsa slices are slow, so bsa is asked
for on one pose only, as tests/test_bsa.py does; tests/test_gpu_pack.py uses all four on the device."""
import pytest

import pack_cases as C


@pytest.fixture(scope="module")
def api():
    from emu_api import emu
    return emu()


def test_hand_made_complexes_equal_the_store_path(api):
    C.check_hand(api, "cpu")


def test_raw_pack_outputs(api):
    C.check_raw_outputs(api, "cpu")


def test_float64_sources_are_rounded_once_and_depth_may_be_listed_twice(api):
    C.check_f64_sources(api, "cpu")


def test_wrongly_shaped_depth_rows_are_refused(api):
    C.check_depth_argument(api, "cpu")


@pytest.mark.parametrize("method", ["mcl", "louvain"])
def test_1ATN_every_source_one_pose_with_bsa(api, method):
    C.check_atn(api, "cpu", (0,), C.ALL_FEATURES, method)


@pytest.mark.parametrize("method", ["mcl", "louvain"])
def test_1ATN_four_poses_without_bsa(api, method):
    C.check_atn(api, "cpu", (0, 1, 2, 3), C.NO_BSA, method)


def test_result_does_not_depend_on_chunk_budget_run_or_batch(api):
    C.check_independence(api, "cpu")


def test_edge_attr(api):
    C.check_edge_attr(api, "cpu")


def test_scores_and_consumers(api, tmp_path):
    C.check_scores(api, "cpu", (0, 1, 2, 3), C.NO_BSA, tmp_path, {"_api": api, "device": "cpu"})


@pytest.mark.parametrize("name", ["good"] + sorted(C.refusal_cases()))
def test_bad_requests_are_refused_before_a_launch(name, api):
    C.check_refusal(api, "cpu", name)


def test_value_errors(api):
    C.check_value_errors(api, "cpu")


def test_capacities(api):
    C.check_capacity_values(api)
