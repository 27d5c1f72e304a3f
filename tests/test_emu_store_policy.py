"""Host-emulation twin of test_gpu_store_policy.py: the index logic of the routines whose output stores go through
out_store (plain stores in the emulation), at the same shapes.  CPU only; see store_policy_check.py."""
import os
import subprocess
import sys

import pytest
import torch

import store_policy_check as sp
from emu_api import emu

HERE = os.path.dirname(os.path.abspath(__file__))
CPU = torch.device("cpu")


@pytest.mark.parametrize("n_feat", sp.FEATS)
@pytest.mark.parametrize("n", sp.NODES)
@pytest.mark.parametrize("net_name", sp.NETS)
def test_emu_co_built_workspace_and_tiles_equal_an_own_launch_build(net_name, n, n_feat):
    sp.check_workspace(net_name, n, n_feat, CPU, emu())


@pytest.mark.parametrize("n_feat", sp.FEATS)
@pytest.mark.parametrize("n", sp.NODES)
@pytest.mark.parametrize("net_name", sp.NETS)
def test_emu_pipelined_steps_equal_the_own_launch_route(net_name, n, n_feat):
    sp.check_routes(net_name, n, n_feat, CPU, emu())


def test_emu_ginet_one_workgroup_form_pipelined_steps_equal_the_own_launch_route():
    """(the plan default is read from the environment once per process: a process of its own for every case at once)"""
    code = ("import torch, store_policy_check as sp\n"
            "from emu_api import emu\n"
            "for n in sp.NODES:\n"
            "    for f in sp.FEATS:\n"
            "        sp.check_routes('GINet', n, f, torch.device('cpu'), emu())\n"
            "print('one-workgroup form ok')\n")
    emu()       # (built before the child starts)
    env = dict(os.environ, DRGNN_STEP_PLAN="one", PYTHONPATH=os.pathsep.join([HERE, os.path.dirname(HERE)] + sys.path))
    run = subprocess.run([sys.executable, "-c", code], cwd=HERE, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert run.returncode == 0 and b"one-workgroup form ok" in run.stdout, run.stdout.decode()[-4000:]


def test_emu_step_reads_the_workspace_the_step_before_wrote():
    sp.check_replay(CPU, emu(), replays=10, record=False)
