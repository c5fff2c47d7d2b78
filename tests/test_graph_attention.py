"""The f64 restatement of graph attention (tests/graph_attention_ref.py) against the reference's own known answer
(graphattention.test.scala:17-158, as data in tests/golden/graph_attention_kats.json) and against the properties of a softmax per
destination, and the part of lamp_amd.graph's attention surface that needs no GPU."""
import json
import os

import torch

from lamp_amd import graph as G
from tests import graph_attention_ref as R

KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "graph_attention_kats.json")))
F64 = torch.float64


def _t(name):
    return torch.tensor(KATS[name], dtype=F64)


def _edges():
    return torch.tensor(KATS["edgeI"]), torch.tensor(KATS["edgeJ"])


def _kat(dot):
    i, j = _edges()
    return R.multihead_graph_attention(_t("nodes"), _t("edges"), i, j, _t("wNodeKey1"), _t("wNodeKey2"), _t("wEdgeKeyDot" if dot else "wEdgeKey"),
                                       _t("wNodeValue"), None if dot else _t("wAttention"), KATS["numHeads"])


def test_restatement_reproduces_the_reference_kat():
    """both scoring branches: 5 x 6, [0, 0] = 1.0 and [0, 3] = 1.5 after rounding to 10 decimals (the reference's assertions), and the
    rows worked out by hand (edges (3, 4) and (4, 4) occur twice and count twice)"""
    for dot in (False, True):
        out = _kat(dot)
        assert list(out.shape) == KATS["expectedShape"]
        assert round(out[0, 0].item(), 10) == KATS["expected_0_0"] and round(out[0, 3].item(), 10) == KATS["expected_0_3"]
        assert (out - _t("restatement")).abs().max().item() <= 1e-12


def test_weights_sum_to_one_per_destination():
    i, j = _edges()
    score = torch.sin(torch.arange(22, dtype=F64)).reshape(11, 2) * 3
    w = R.attention_weights(score, j, 5)
    total = torch.zeros(5, 2, dtype=F64).index_add(0, j, w)
    assert (total - 1).abs().max().item() <= 1e-15
    out = R.attention_aggregate(score, torch.ones(5, 2, 3, dtype=F64), i, j)
    assert (out - 1).abs().max().item() <= 1e-15


def test_a_destination_without_an_incoming_edge_gets_zeros():
    i, j = torch.tensor([0, 1, 2]), torch.tensor([0, 0, 2])           # nothing arrives at node 1
    out = R.attention_aggregate(torch.zeros(3, 1, dtype=F64), torch.ones(3, 1, 2, dtype=F64), i, j)
    assert out.tolist() == [[1, 1], [0, 0], [1, 1]]


def test_restatement_is_shift_invariant_per_destination():
    """adding a constant per destination to the scores changes nothing: +64 on even destinations, -64 on odd ones, scores in eighths"""
    i, j = _edges()
    score = (torch.arange(22, dtype=F64).reshape(11, 2) * 5 % 17 - 8) / 8
    value = torch.cos(torch.arange(30, dtype=F64)).reshape(5, 2, 3)
    shift = torch.where(j % 2 == 0, 64.0, -64.0).to(F64).unsqueeze(1)
    a, b = R.attention_aggregate(score, value, i, j), R.attention_aggregate(score + shift, value, i, j)
    assert (a - b).abs().max().item() <= 1e-15


def test_python_surface_without_a_gpu():
    """the switch returns the previous setting, the split threshold comes from the library, the public names exist"""
    assert G.graphAttentionFused(False) is True and G.graphAttentionFused(True) is False and G.graphAttentionFused(True) is True
    assert G.gatLongRow() >= 64
    for name in ("GraphAttention", "multiheadGraphAttention", "multiheadGraphAttentionComposed", "graphAttentionAggregate",
                 "graphAttentionAggregateComposed", "graphAttentionFused", "gatLongRow", "EdgeCsr", "computeEdgeCsr"):
        assert hasattr(G, name), name
    assert hasattr(G.Graph, "edgeCsr") and hasattr(G.GraphAttention, "apply")
