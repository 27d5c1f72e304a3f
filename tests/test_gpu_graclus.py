"""graclus / normalized_cut / max_pool on the MI355X."""
import pytest

from graclus_check import check_custom_net_recipe, check_graclus, check_graclus_carve_limit, check_graclus_large

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [0, 1])
def test_graclus_matches_oracle(seed):
    check_graclus("cuda", seed=seed)


def test_graclus_large_graph_with_ties_matches_oracle():
    """(a carve beyond 64 KiB: the dynamic-LDS attribute of the kernel is raised; two runs give the same labels)"""
    check_graclus_large("cuda")


def test_graclus_carve_limit_and_capacity_error():
    check_graclus_carve_limit("cuda")


def test_readme_custom_net_recipe():
    check_custom_net_recipe("cuda")
