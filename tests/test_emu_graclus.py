"""graclus / normalized_cut / max_pool, kernels emulated on the CPU."""
import pytest

from emu_api import emu
from graclus_check import check_custom_net_recipe, check_graclus, check_graclus_carve_limit, check_graclus_large
from deeprank_gnn_amd import _lib


@pytest.fixture(autouse=True)
def use_emulation(monkeypatch):
    monkeypatch.setattr(_lib, "get", lambda: emu())          # (the conv layers of the recipe ask the library themselves)


@pytest.mark.parametrize("seed", [0, 1])
def test_graclus_matches_oracle(seed):
    check_graclus("cpu", api=emu(), seed=seed)


def test_graclus_large_graph_with_ties_matches_oracle():
    check_graclus_large("cpu", api=emu())


def test_graclus_carve_limit_and_capacity_error():
    check_graclus_carve_limit("cpu", api=emu())


def test_readme_custom_net_recipe():
    check_custom_net_recipe("cpu", api=emu())
