"""AdamW, gradient-norm clipping and learning-rate tables on every native path (optim_check.py), product library on the
MI355X."""
import pytest
import torch

from adam_check import NETS, PATH_NETS, PATHS, SIZES
from deeprank_gnn_amd import _lib
from optim_check import (OPTIONS, check_cohort, check_epoch_of_many, check_flat_coupled, check_path_coupled, check_five_steps_against_torch, check_flat_clip, check_flat_decay,
                         check_flat_schedule, check_path_option, check_recorded_step, check_resume)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("t0", [0, 9])
@pytest.mark.parametrize("n", SIZES)
def test_flat_kernel_adamw(n, t0):
    check_flat_decay(DEV, _lib.get(), n, t0)


@pytest.mark.parametrize("active", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_flat_kernel_clipping(n, active):
    check_flat_clip(DEV, _lib.get(), n, active)


@pytest.mark.parametrize("t0", [0, 999])
@pytest.mark.parametrize("n", SIZES)
def test_flat_kernel_schedule(n, t0):
    check_flat_schedule(DEV, _lib.get(), n, t0)


@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("net,task,n_out", PATH_NETS)
def test_trainer_paths(net, task, n_out, path, option):
    check_path_option(net, DEV, _lib.get(), path, option, task=task, n_out=n_out)


@pytest.mark.parametrize("net", sorted(NETS))
def test_epoch_of_many(net):
    check_epoch_of_many(net, DEV, _lib.get())


@pytest.mark.parametrize("net", sorted(NETS))
def test_resume(net):
    check_resume(net, DEV, _lib.get())


@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("net", sorted(NETS))
def test_recorded_step_walks_the_schedule(net, cached):
    check_recorded_step(net, DEV, _lib.get(), cached)


@pytest.mark.parametrize("net_name", sorted(NETS))
def test_five_steps_match_torch_adamw_clip_steplr(net_name):
    from test_gpu_parity import build
    check_five_steps_against_torch(net_name, torch.device(DEV), _lib.get(), lambda name, params: build(name, params, 1))


@pytest.mark.parametrize("net", sorted(NETS))
def test_cohort_members_equal_their_own_trainers(net):
    check_cohort(net, DEV, _lib.get(), "fused")


@pytest.mark.parametrize("n", SIZES)
def test_flat_kernel_coupled_decay_with_clipping_and_schedule(n):
    check_flat_coupled(DEV, _lib.get(), n)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("net", sorted(NETS))
def test_trainer_paths_coupled_decay_with_clipping_and_schedule(net, path):
    check_path_coupled(net, DEV, _lib.get(), path)
