"""The function-level pooling API beyond the fixture graphs (tests/pool_check.py), kernels emulated on the CPU."""
import pytest

import pool_check as P
from emu_api import emu
from deeprank_gnn_amd import _lib


@pytest.fixture(autouse=True)
def use_emulation(monkeypatch):
    monkeypatch.setattr(_lib, "get", lambda: emu())


def test_numpy_references_equal_the_pinned_oracle_on_the_fixture():
    P.check_references_on_fixture()


@pytest.mark.parametrize("width", P.WIDTHS)
@pytest.mark.parametrize("variant", P.VARIANTS)
def test_cluster_max_and_gradient_on_ragged_batch(variant, width):
    P.check_cluster_max("cpu", variant, width, api=emu())


@pytest.mark.parametrize("width", P.WIDTHS)
def test_scatter_ops_on_ragged_labels(width):
    P.check_scatter_on_ragged("cpu", width, api=emu())


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_pooled_edges_and_mean_positions_on_ragged_batch(variant):
    P.check_pooled_edges("cpu", variant, api=emu())


def test_plain_data_pools_to_data_with_pos2D():
    P.check_plain_data("cpu", api=emu())


@pytest.mark.parametrize("where,shift", P.PRELOADED_CASES)
def test_get_preloaded_cluster_maximum_positions(where, shift):
    P.check_preloaded_cluster("cpu", where, shift, api=emu())


@pytest.mark.parametrize("name", sorted(P.SCATTER_CASES))
def test_scatter_ops_at_size(name):
    P.check_scatter_at_size("cpu", name, api=emu())
