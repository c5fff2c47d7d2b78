"""lamp.data.GraphBatchStream's host side, without a GPU: graphBatchPlan against tables worked out by hand, and the torch restatement of
the reference's fold (tests/graph_batch_ref.py) against the reference's own known answer (gcn.test.scala "small graph mode
batchstream")."""
import numpy as np
import torch

from lamp_amd.data import JavaRandom
from lamp_amd.graphbatch import graphBatchPlan
from tests import graph_batch_ref as R

NODES, EDGES = (5, 1, 4, 7), (5, 0, 3, 9)       # nodePtr 0 5 6 10 17, edgePtr 0 5 5 8 17
# rows (srcNodeBase, dstNodeBase, srcEdgeBase, dstEdgeBase) per graph id, the destination bases left to the case
SRC = {0: (0, 0), 1: (5, 5), 2: (6, 5), 3: (10, 8)}


def test_plan_full_and_short_batch():
    p = graphBatchPlan(NODES, EDGES, (2, 0, 3, 1), 3)
    # batch 0 = graphs 2, 0, 3: nodes at 0, 4, 9 (16 in all), edges at 0, 3, 8 (17 in all); batch 1 = graph 1 alone, no edge
    assert p.table.tolist() == [[6, 0, 5, 0], [0, 4, 0, 3], [10, 9, 8, 8], [5, 0, 5, 0]]
    assert p.offsets.tolist() == [0, 3] and p.totals.tolist() == [[3, 16, 17], [1, 1, 0]]
    assert p.table.dtype == np.int64 and p.offsets.dtype == np.int64 and p.totals.dtype == np.int64


def test_plan_minibatch_of_one():
    p = graphBatchPlan(NODES, EDGES, (2, 0, 3, 1), 1)
    assert p.table.tolist() == [[6, 0, 5, 0], [0, 0, 0, 0], [10, 0, 8, 0], [5, 0, 5, 0]]
    assert p.offsets.tolist() == [0, 1, 2, 3] and p.totals.tolist() == [[1, 4, 3], [1, 5, 5], [1, 7, 9], [1, 1, 0]]


def test_plan_minibatch_larger_than_the_set():
    p = graphBatchPlan(NODES, EDGES, (0, 1, 2, 3), 9)
    assert p.table.tolist() == [[0, 0, 0, 0], [5, 5, 5, 5], [6, 6, 5, 5], [10, 10, 8, 8]]
    assert p.offsets.tolist() == [0] and p.totals.tolist() == [[4, 17, 17]]


def test_plan_repeated_graph():
    p = graphBatchPlan(NODES, EDGES, (3, 3), 2)
    assert p.table.tolist() == [[10, 0, 8, 0], [10, 7, 8, 9]] and p.totals.tolist() == [[2, 14, 18]]


def test_plan_over_a_shuffled_order():
    """the order JavaRandom(seed).shuffle draws: every batch's rows are those of its graphs, one after the other"""
    order = JavaRandom(42).shuffle(list(range(4)))
    assert sorted(order) == [0, 1, 2, 3] and order == JavaRandom(42).shuffle(list(range(4)))
    p = graphBatchPlan(NODES, EDGES, order, 3)
    assert p.offsets.tolist() == [0, 3]
    for off, (b, nb, eb) in zip(p.offsets.tolist(), p.totals.tolist()):
        dn = de = 0
        for k in range(off, off + b):
            g = order[k]
            assert p.table[k].tolist() == [SRC[g][0], dn, SRC[g][1], de]
            dn, de = dn + NODES[g], de + EDGES[g]
        assert (nb, eb) == (dn, de)
    assert int(p.totals[:, 0].sum()) == 4


def kat_graphs():
    """gcn.test.scala:295-329: ones(5, 2) and zeros(5, 2), both with the edges (0,1) (0,2) (0,3) (0,4) (1,2) and edge features zeros([5])"""
    ei, ej = torch.tensor([0, 0, 0, 0, 1]), torch.tensor([1, 2, 3, 4, 2])
    return [(torch.ones(5, 2, dtype=torch.float64), torch.zeros(5), ei, ej), (torch.zeros(5, 2, dtype=torch.float64), torch.zeros(5), ei, ej)]


def check_kat(batch):
    """gcn.test.scala:341-348; holds for either order of the two graphs"""
    assert list(batch["nodeFeatures"].shape) == [10, 2]
    assert batch["edgeI"][9].item() >= 5 and batch["edgeI"][0].item() < 5
    assert batch["vertexPoolingIndices"].tolist() == [0] * 5 + [1] * 5
    assert list(batch["target"].shape) == [2]


def test_fold_restatement_against_the_reference_known_answer():
    target = torch.tensor([0.0, 1.0], dtype=torch.float64)
    for order in ([0, 1], [1, 0], JavaRandom(7).shuffle([0, 1])):
        groups = R.batches(order, 2)
        assert len(groups) == 1
        batch = R.fold(kat_graphs(), groups[0], target)
        check_kat(batch)
        assert batch["edgeI"].tolist() == [0, 0, 0, 0, 1, 5, 5, 5, 5, 6] and batch["edgeJ"].tolist() == [1, 2, 3, 4, 2, 6, 7, 8, 9, 7]
        assert batch["target"].tolist() == [float(g) for g in order] and batch["nodeFeatures"][0, 0].item() == 1.0 - order[0]
    assert R.batches([3, 1, 2, 0, 4], 2) == [[3, 1], [2, 0], [4]]
