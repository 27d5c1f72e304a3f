"""The Adam update on every path against a float64 reference (adam_check.py), kernels emulated on the CPU."""
import pytest

from adam_check import (HYPER, NETS, PATH_NETS, PATHS, T0, check_adam_kernel, check_epoch_of_many, check_resume,
                        check_trainer_paths)
from emu_api import emu


@pytest.mark.parametrize("t0", T0)
@pytest.mark.parametrize("hyper", range(len(HYPER)))
@pytest.mark.parametrize("n", [1, 257, 4273])
def test_adam_kernel(n, hyper, t0):
    check_adam_kernel("cpu", emu(), n, HYPER[hyper], t0)


@pytest.mark.parametrize("t0", [0, 999])
@pytest.mark.parametrize("hyper", range(len(HYPER)))
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("net,task,n_out", PATH_NETS)
def test_trainer_paths(net, task, n_out, path, hyper, t0):
    check_trainer_paths(net, "cpu", emu(), path, HYPER[hyper], t0, task=task, n_out=n_out)


@pytest.mark.parametrize("hyper", [1, 2])
@pytest.mark.parametrize("net", sorted(NETS))
def test_epoch_of_many(net, hyper):
    check_epoch_of_many(net, "cpu", emu(), HYPER[hyper])


@pytest.mark.parametrize("net", sorted(NETS))
def test_resume(net):
    check_resume(net, "cpu", emu())
