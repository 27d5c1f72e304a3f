"""Write-through stores of what the next launch reads, on the MI355X: see store_policy_check.py (the emulated counterpart is
test_emu_store_policy.py)."""
import os
import subprocess
import sys

import pytest
import torch

import store_policy_check as sp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.mark.parametrize("n_feat", sp.FEATS)
@pytest.mark.parametrize("n", sp.NODES)
@pytest.mark.parametrize("net_name", sp.NETS)
def test_co_built_workspace_and_tiles_equal_an_own_launch_build(net_name, n, n_feat):
    sp.check_workspace(net_name, n, n_feat, _dev())


@pytest.mark.parametrize("n_feat", sp.FEATS)
@pytest.mark.parametrize("n", sp.NODES)
@pytest.mark.parametrize("net_name", sp.NETS)
def test_pipelined_steps_equal_the_own_launch_route(net_name, n, n_feat):
    sp.check_routes(net_name, n, n_feat, _dev())


def test_ginet_one_workgroup_form_pipelined_steps_equal_the_own_launch_route():
    """GINet's one-workgroup-per-graph (3b) form: the plan default is read from the environment once per process, hence a
    process of its own for every case at once."""
    code = ("import torch, store_policy_check as sp\n"
            "dev = torch.device('cuda:0')\n"
            "for n in sp.NODES:\n"
            "    for f in sp.FEATS:\n"
            "        sp.check_routes('GINet', n, f, dev)\n"
            "        sp.check_workspace('GINet', n, f, dev)\n"
            "print('one-workgroup form ok')\n")
    env = dict(os.environ, DRGNN_STEP_PLAN="one", PYTHONPATH=os.pathsep.join([HERE, os.path.dirname(HERE)] + sys.path))
    run = subprocess.run([sys.executable, "-c", code], cwd=HERE, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert run.returncode == 0 and b"one-workgroup form ok" in run.stdout, run.stdout.decode()[-4000:]


def test_recorded_graph_reads_the_workspace_the_step_before_wrote():
    sp.check_replay(_dev(), replays=10, record=True)
