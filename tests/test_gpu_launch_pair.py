"""The launch pair on the MI355X at the shapes only it serves: more than 64 node features (k_net's LDS / global-scratch
instances, the MFMA wg_gemm with K = F and M = F beyond 64 and its tails, the K-split of dW1, dX through the xs tile), heads
other than the reference's (head_graph's passes, the staged and the unstaged head, k_head's passes), d loss / d x, and a
resident set of 72 features with and without aggregation tiles.  Before each launch the checker asserts that the plan is outside the fused kernels
(family NONE) and which scratch regime of k_net it is.  See pair_check.py; the emulated counterpart is
test_emu_launch_pair.py."""
import pytest
import torch

import pair_check as pc

pytestmark = pytest.mark.gpu
NETS = ["GINet", "sGAT", "FoutNet"]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("net_name,n_feat,n_nodes,want", pc.WIDTH_CASES)
def test_wide_features_match_oracle(net_name, n_feat, n_nodes, want):
    pc.check_width(net_name, n_feat, n_nodes, want, _dev())


def test_wide_features_with_the_next_topology_co_built():
    pc.check_width(*pc.CO_BUILD_CASE, _dev(), co_build=True)


@pytest.mark.parametrize("net_name", NETS)
@pytest.mark.parametrize("n_feat", [100, 129])
def test_wide_features_ragged_batch(net_name, n_feat):
    pc.check_ragged(net_name, n_feat, _dev())


@pytest.mark.parametrize("net_name", NETS)
def test_three_adam_steps_at_100_features(net_name):
    pc.check_three_adam_steps(net_name, _dev())


@pytest.mark.parametrize("n_feat", [32, 100])
@pytest.mark.parametrize("O", [1, 3])
@pytest.mark.parametrize("net_name,H", pc.HEADS)
def test_other_heads_match_oracle(net_name, H, O, n_feat):
    pc.check_head(net_name, H, O, n_feat, _dev())


def test_head_with_dropout_mask():
    pc.check_head("GINet", 200, 1, 100, _dev(), dropout=0.4)


def test_head_of_513_units_is_refused():
    pc.check_head_too_wide(_dev())


@pytest.mark.parametrize("B,R,H,O,passes", pc.HEAD_STEP_CASES)
def test_head_step_wide_heads_many_outputs_large_batches(B, R, H, O, passes):
    pc.check_head_step(_dev(), None, B, R, H, O, passes)


@pytest.mark.parametrize("net_name", NETS)
def test_model_call_at_100_features(net_name):
    pc.check_dropin_wide(net_name, _dev())


@pytest.mark.parametrize("net_name", NETS)
@pytest.mark.parametrize("n_feat", [32, 100])
def test_grad_x_matches_oracle(net_name, n_feat):
    pc.check_grad_x(net_name, n_feat, _dev())


@pytest.mark.parametrize("net_name", NETS)
def test_resident_set_with_72_features(net_name):
    pc.check_resident_set(net_name, _dev())


@pytest.mark.parametrize("net_name", NETS)
def test_resident_set_with_72_features_and_no_tiles(net_name):
    pc.check_resident_set(net_name, _dev(), big=250)


@pytest.mark.parametrize("net_name", NETS)
def test_neuralnet_trains_on_72_features(net_name, tmp_path):
    pc.check_neuralnet_wide(net_name, tmp_path)
