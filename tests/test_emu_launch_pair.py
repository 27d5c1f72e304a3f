"""The launch pair beyond the fused kernels' shapes -- more than 64 features, other heads, d loss / d x -- in the
host-emulation build: k_net's per-graph routines, head_graph, train_update and k_head are the device's own source (the
emulation's wg_gemm is a plain loop: the MFMA tiles are the device test's, test_gpu_launch_pair.py).  CPU only.  See
pair_check.py."""
import pytest

import pair_check as pc
from emu_api import emu

NETS = ["GINet", "sGAT", "FoutNet"]


@pytest.mark.parametrize("net_name,n_feat,n_nodes,want", pc.WIDTH_CASES)
def test_wide_features_match_oracle(net_name, n_feat, n_nodes, want):
    pc.check_width(net_name, n_feat, n_nodes, want, "cpu", api=emu())


def test_wide_features_with_the_next_topology_co_built():
    pc.check_width(*pc.CO_BUILD_CASE, "cpu", api=emu(), co_build=True)


@pytest.mark.parametrize("net_name", NETS)
@pytest.mark.parametrize("n_feat", [100, 129])
def test_wide_features_ragged_batch(net_name, n_feat):
    pc.check_ragged(net_name, n_feat, "cpu", api=emu())


@pytest.mark.parametrize("net_name", NETS)
def test_three_adam_steps_at_100_features(net_name):
    pc.check_three_adam_steps(net_name, "cpu", api=emu())


@pytest.mark.parametrize("n_feat", [32, 100])
@pytest.mark.parametrize("O", [1, 3])
@pytest.mark.parametrize("net_name,H", pc.HEADS)
def test_other_heads_match_oracle(net_name, H, O, n_feat):
    """(H > 128: head_graph's fc1 in passes of 128 units; before, its split sums ran over the hidden row and the staged
    readout row)"""
    pc.check_head(net_name, H, O, n_feat, "cpu", api=emu())


def test_head_with_dropout_mask():
    pc.check_head("GINet", 200, 1, 100, "cpu", api=emu(), dropout=0.4)


def test_head_of_513_units_is_refused():
    pc.check_head_too_wide("cpu", api=emu())


@pytest.mark.parametrize("B,R,H,O,passes", pc.HEAD_STEP_CASES)
def test_head_step_wide_heads_many_outputs_large_batches(B, R, H, O, passes):
    pc.check_head_step("cpu", emu(), B, R, H, O, passes)


@pytest.mark.parametrize("net_name", NETS)
def test_model_call_at_100_features(net_name):
    pc.check_dropin_wide(net_name, "cpu", api=emu())


@pytest.mark.parametrize("net_name", NETS)
@pytest.mark.parametrize("n_feat", [32, 100])
def test_grad_x_matches_oracle(net_name, n_feat):
    pc.check_grad_x(net_name, n_feat, "cpu", api=emu())


@pytest.mark.parametrize("net_name", NETS)
def test_resident_set_with_72_features(net_name):
    pc.check_resident_set(net_name, "cpu", api=emu())


@pytest.mark.parametrize("net_name", NETS)
def test_resident_set_with_72_features_and_no_tiles(net_name):
    pc.check_resident_set(net_name, "cpu", api=emu(), big=250)


@pytest.mark.parametrize("net_name", NETS)
def test_neuralnet_trains_on_72_features(net_name, tmp_path):
    pc.check_neuralnet_wide(net_name, tmp_path, api=emu())
