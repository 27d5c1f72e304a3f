"""AdamW, gradient-norm clipping and learning-rate tables on every native path (optim_check.py), kernels emulated on the CPU."""
import pytest
import torch

from adam_check import NETS, PATH_NETS, PATHS
from emu_api import emu
from optim_check import (OPTIONS, check_cohort, check_epoch_of_many, check_flat_coupled, check_path_coupled, check_five_steps_against_torch, check_flat_clip, check_flat_decay,
                         check_flat_schedule, check_path_option, check_resume, check_schedule_from_torch)

FLAT = [1, 257, 4273]


@pytest.mark.parametrize("t0", [0, 9])
@pytest.mark.parametrize("n", FLAT)
def test_flat_kernel_adamw(n, t0):
    check_flat_decay("cpu", emu(), n, t0)


@pytest.mark.parametrize("active", [True, False])
@pytest.mark.parametrize("n", FLAT)
def test_flat_kernel_clipping(n, active):
    check_flat_clip("cpu", emu(), n, active)


@pytest.mark.parametrize("t0", [0, 999])
@pytest.mark.parametrize("n", FLAT)
def test_flat_kernel_schedule(n, t0):
    check_flat_schedule("cpu", emu(), n, t0)


@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("net,task,n_out", PATH_NETS)
def test_trainer_paths(net, task, n_out, path, option):
    check_path_option(net, "cpu", emu(), path, option, task=task, n_out=n_out)


@pytest.mark.parametrize("net", sorted(NETS))
def test_epoch_of_many(net):
    check_epoch_of_many(net, "cpu", emu())


@pytest.mark.parametrize("net", sorted(NETS))
def test_resume(net):
    check_resume(net, "cpu", emu())


def test_schedule_from_torch():
    check_schedule_from_torch()


def _build(net_name, params):
    net = NETS[net_name](32, 1, 1)
    net.load_state_dict(params, strict=True)
    if hasattr(net, "dropout"):
        net.dropout = 0.0
    return net


@pytest.mark.parametrize("net_name", sorted(NETS))
def test_five_steps_match_torch_adamw_clip_steplr(net_name):
    check_five_steps_against_torch(net_name, torch.device("cpu"), emu(), _build)


@pytest.mark.parametrize("net", sorted(NETS))
def test_cohort_members_equal_their_own_trainers(net):
    check_cohort(net, "cpu", emu(), "separate")


@pytest.mark.parametrize("n", FLAT)
def test_flat_kernel_coupled_decay_with_clipping_and_schedule(n):
    check_flat_coupled("cpu", emu(), n)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("net", sorted(NETS))
def test_trainer_paths_coupled_decay_with_clipping_and_schedule(net, path):
    check_path_coupled(net, "cpu", emu(), path)
