"""interface_resident_set and drgnn_iface_pack (drgnn_pack.h through libdrgnn.so) on the MI355X: the checks of
tests/test_pack.py with bsa on all four poses, and the device against the host emulation."""
import numpy as np
import pytest

import pack_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


def test_hand_made_complexes_equal_the_store_path(api):
    C.check_hand(api, "cuda")


def test_raw_pack_outputs(api):
    C.check_raw_outputs(api, "cuda")


def test_float64_sources_are_rounded_once_and_depth_may_be_listed_twice(api):
    C.check_f64_sources(api, "cuda")


def test_wrongly_shaped_depth_rows_are_refused(api):
    C.check_depth_argument(api, "cuda")


@pytest.mark.parametrize("method", ["mcl", "louvain"])
def test_1ATN_four_poses_every_source(api, method):
    C.check_atn(api, "cuda", (0, 1, 2, 3), C.ALL_FEATURES, method)


def test_result_does_not_depend_on_chunk_budget_run_or_batch(api):
    C.check_independence(api, "cuda")


def test_edge_attr_and_device_equals_emulation(api):
    from emu_api import emu
    raw, default = C.check_edge_attr(api, "cuda")
    host_raw, host_default = C.check_edge_attr(emu(), "cpu")
    C.assert_sets_equal(raw, host_raw, "device against emulation, raw distances", attr="bits")
    C.assert_sets_equal(default, host_default, "device against emulation", attr=None)
    u = C.ulps32(default.edge_attr.cpu().numpy(), host_default.edge_attr.numpy())
    print("edge_attr, device against emulation: at most %d ulp" % int(u.max()))
    assert u.max() <= 1                                                 # two fp64 tanh implementations


def test_scores_and_consumers(api, tmp_path):
    C.check_scores(api, "cuda", (0, 1, 2, 3), C.ALL_FEATURES, tmp_path, {})


@pytest.mark.parametrize("name", ["good"] + sorted(C.refusal_cases()))
def test_bad_requests_are_refused_before_a_launch(name, api):
    C.check_refusal(api, "cuda", name)


def test_value_errors(api):
    C.check_value_errors(api, "cuda")


def test_capacities(api):
    C.check_capacity_values(api)
