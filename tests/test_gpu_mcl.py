"""Markov clustering (drgnn_mcl) on the MI355X against oracle/mcl_ref.py: the cases, the robustness filter and the
comparison of tests/mcl_check.py, as tests/test_mcl.py runs them on the host-emulation build -- plus what only the
device can show: column loops with a second trip (N > 1024), more workgroups than compute units, repeat launches,
and the arithmetic the emulation does not have (FMA contraction of the expansion product, the convergence test
reduced over 1024 lanes)."""
import time

import numpy as np
import pytest
import torch

import louvain_ref as R
import mcl_check as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _run(cases):
    """one launch on the batch of ``cases``: (labels, info)"""
    from deeprank_gnn_amd.clustering import mcl_labels
    ei, nptr, eptr = (t.to(DEV) for t in R.batch_of(cases))
    labels, info = mcl_labels(ei, nptr, eptr)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize("case", C.named_cases(), ids=[c[0] for c in C.named_cases()])
def test_device_equals_oracle_per_named_case(case):
    C.run_named_case(case, _run)


def test_device_equals_oracle_in_one_batch_and_repeat_launch_is_bit_identical():
    """every kept case in ONE launch (more workgroups than the 256 compute units), an empty and a one-node graph in
    the middle; a second launch returns the same bytes"""
    cases = C.one_batch_cases()
    assert len(cases) > 256
    first = _run(cases)
    C.check_exact(cases, *first)
    second = _run(cases)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


def test_300_small_graphs_in_one_launch():
    kept = C.filter_report()
    small = [c for c in kept if c[0].startswith("rnd")]
    assert len(small) >= 285                                  # the filter's 5 % cap on the 300 random graphs
    small = (small + C.kept_named())[:300]
    assert len(small) == 300
    C.check_exact(small, *_run(small))


def test_result_does_not_depend_on_the_position_in_the_batch():
    C.run_position_independence(_run)


def test_1030_nodes_second_trip_of_the_column_loops():
    """N = 1030, alone in its batch: the smallest size at which FOR_TID(j, N) (column sums, arg-max, attractor flags,
    ranks, labels) takes a second trip.  A path plus N random chords; filter variants (a) and (c) (the long-double
    restatement takes minutes at this size).  Prints the device time of the launch: 7.3 s measured for its 16
    iterations (one workgroup; about 5 s of it is the ranking of the 646 attractor rows, not the iterations)."""
    pairs, n = C.big_graph(1030, seed=1030)
    assert C.robust(pairs, n, use_longdouble=False)
    case = ("chords1030", pairs, n)
    ei, nptr, eptr = (t.to(DEV) for t in R.batch_of([case]))
    from deeprank_gnn_amd.clustering import mcl_labels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    labels, info = mcl_labels(ei, nptr, eptr)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print("mcl N = 1030 on the device: %.3f s for %d iterations" % (seconds, int(info[0])))
    C.check_exact([case], labels.cpu().numpy(), info.cpu().numpy())
    assert len(C.reference(pairs, n)[2]) > 100                # many clusters: ranks and labels beyond node 1023 matter


def test_pruning_keeps_the_column_maximum():
    """1030 nodes again (mcl_check.cocktail_party): after the first inflation EVERY column maximum lies below the pruning
    threshold, which only a graph of more than 1000 nodes can do; the pruning must keep it.  3 iterations, 1030
    clusters; 5.9 s measured on the device, nearly all of it the ranking of 1030 attractor rows.  Too slow for the
    emulation build (10 s), so it runs here only."""
    C.run_keep_maximum_case(_run)


def test_precluster_on_other_graphs_than_the_fixture():
    from deeprank_gnn_amd.clustering import precluster
    C.run_precluster(precluster, device=DEV)


def test_PreCluster_in_four_chunks_reproduces_the_fixture():
    C.run_PreCluster_in_chunks('cuda')


def test_community_detection_functions_on_the_device():
    """community_detection(method='mcl') on the reference's toy graph and community_detection_per_batch with the
    reference's shared-id offset (tests/test_mcl.py pins the same on the emulation build)"""
    from oracle import mcl_ref
    from deeprank_gnn_amd import community_pooling as cp
    ei = torch.tensor([[0, 1, 1, 2, 3, 4, 4, 5], [1, 0, 2, 1, 4, 3, 5, 4]])
    got = cp.community_detection(ei.to(DEV), 6, method='mcl').cpu().numpy()
    np.testing.assert_array_equal(got, mcl_ref.community_detection_mcl(ei.numpy(), 6))
    assert got.tolist() == [0, 0, 0, 1, 1, 1]
    per_batch = cp.community_detection_per_batch(torch.cat([ei, ei + 6], 1).to(DEV),
                                                 torch.tensor([0] * 6 + [1] * 6).to(DEV), 12)
    assert per_batch.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2]
    with pytest.raises(ValueError):
        cp.community_detection(ei.to(DEV), 6, method='xxx')


def test_precluster_on_device_reproduces_the_fixture_labels():
    """Offline MCL (fp64, one workgroup per graph) + pooling on the MI355X == the reference's stored
    clustering/mcl/depth_0 and depth_1 for all 10 fixture graphs."""
    from test_mcl import _fixture_batch_without_clusters
    from deeprank_gnn_amd.clustering import precluster
    batch, expect0, expect1 = _fixture_batch_without_clusters()
    d0, d1 = precluster(batch.to(DEV))
    np.testing.assert_array_equal(d0.cpu().numpy(), expect0)
    np.testing.assert_array_equal(d1.cpu().numpy(), expect1)
