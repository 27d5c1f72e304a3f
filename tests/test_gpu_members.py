"""FusedTrainer.adopt_storage on the MI355X: a trainer moved onto caller-owned rows (as members.MemberPack moves a cohort's)
steps bit for bit like a trainer of its own -- GINet with its default plan (two workgroups per graph: the exchange words and
the dropout stream are in play) and sGAT (its default plan splits a graph's nodes over two workgroups)."""
import pytest

from test_gpu_ensemble import graphs_of
from test_members import check_adopt_storage
from deeprank_gnn_amd.ginet import GINet
from deeprank_gnn_amd.sGAT import sGAT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Net", [GINet, sGAT])
def test_adopt_storage(Net):
    trainers = check_adopt_storage(Net, graphs_of(8, 28), "cuda:0", None, B=4, steps=3, wgs=2)
    for tr in trainers:
        tr.check_faults()
