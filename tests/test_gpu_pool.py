"""The function-level pooling API beyond the fixture graphs (tests/pool_check.py) on the MI355X."""
import pytest

import pool_check as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("width", P.WIDTHS)
@pytest.mark.parametrize("variant", P.VARIANTS)
def test_cluster_max_and_gradient_on_ragged_batch(variant, width):
    P.check_cluster_max(DEV, variant, width)


@pytest.mark.parametrize("width", P.WIDTHS)
def test_scatter_ops_on_ragged_labels(width):
    P.check_scatter_on_ragged(DEV, width)


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_pooled_edges_and_mean_positions_on_ragged_batch(variant):
    P.check_pooled_edges(DEV, variant)


def test_plain_data_pools_to_data_with_pos2D():
    P.check_plain_data(DEV)


@pytest.mark.parametrize("where,shift", P.PRELOADED_CASES)
def test_get_preloaded_cluster_maximum_positions(where, shift):
    P.check_preloaded_cluster(DEV, where, shift)


@pytest.mark.parametrize("name", sorted(P.SCATTER_CASES))
def test_scatter_ops_at_size(name):
    P.check_scatter_at_size(DEV, name)
