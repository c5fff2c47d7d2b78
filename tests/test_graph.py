"""The f64 restatement of the GCN path (tests/graph_ref.py) against the reference's own two known answers (gcn.test.scala:23-125, as
data in tests/golden/graph_kats.json) and against the multiplicity rule of the reference's COO addition.  No GPU."""
import json
import os

import torch

from lamp_amd import graph as G
from tests import graph_ref as R

KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "graph_kats.json")))
F64 = torch.float64
HALF_ULP_4 = 0.5e-4 * (1 + 1e-9)      # "equal after rounding to 4 decimals": the expected values are rounded, the results are not


def _edges():
    return torch.tensor(KATS["edgeI"]), torch.tensor(KATS["edgeJ"])


def test_degrees_of_the_star():
    i, j = _edges()
    assert R.degrees(i, j, KATS["numNodes"]).tolist() == KATS["degreesPlusOne"]


def test_aggregation_kat():
    i, j = _edges()
    k = KATS["aggregation"]
    out = R.gcn_aggregation(torch.tensor(k["nodes"], dtype=F64), i, j)
    assert (out - torch.tensor(k["expected"], dtype=F64)).abs().max().item() <= HALF_ULP_4


def test_module_kat():
    i, j = _edges()
    k = KATS["module"]
    out = R.gcn_linear_relu(torch.tensor(k["nodes"], dtype=F64), i, j, torch.tensor(k["weight"], dtype=F64), torch.tensor(k["bias"], dtype=F64))
    assert list(out.shape) == [4, 3]
    assert (out - torch.tensor(k["expected"], dtype=F64)).abs().max().item() <= HALF_ULP_4


def test_duplicates_and_two_way_pairs_count_twice():
    # 0-1 twice, 2-3 and 3-2, 1-2 once
    i, j = torch.tensor([0, 0, 2, 3, 1]), torch.tensor([1, 1, 3, 2, 2])
    a = R.dense_adjacency(i, j, 5)
    assert a[0, 1] == 2 and a[1, 0] == 2 and a[2, 3] == 2 and a[3, 2] == 2 and a[1, 2] == 1 and a[2, 1] == 1
    assert torch.equal(a.diagonal(), torch.ones(5, dtype=F64)) and a[4].sum() == 1          # node 4 is isolated
    assert torch.equal(a, a.t())
    assert R.degrees(i, j, 5).tolist() == [3, 4, 4, 3, 1]
    x = torch.arange(10, dtype=F64).reshape(5, 2)
    d = R.degrees(i, j, 5).pow(-0.5)
    assert torch.allclose(R.gcn_aggregation(x, i, j), torch.diag(d) @ a @ torch.diag(d) @ x, rtol=0, atol=1e-15)


def test_vertex_pooling():
    x = torch.arange(12, dtype=F64).reshape(6, 2)
    idx = torch.tensor([0, 0, 1, 2, 2, 2])
    assert R.vertex_pooling(x, idx, "Sum").tolist() == [[2, 4], [4, 5], [24, 27]]
    assert R.vertex_pooling(x, idx, "Mean").tolist() == [[1, 2], [4, 5], [8, 9]]


def test_python_surface_without_a_gpu():
    """the switch returns the previous setting and the split threshold comes from the library (neither needs a GPU)"""
    assert G.gcnFused(False) is True and G.gcnFused(True) is False and G.gcnFused(True) is True
    assert G.longRow() >= 64
    for name in ("Graph", "GCN", "gcn", "computeAdjacency", "gcnAggregation", "gcnAggregationComposed", "VertexPooling", "ResidualModule"):
        assert hasattr(G, name), name
