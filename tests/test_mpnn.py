"""The f64 restatement of MPNN's message and MPNN.aggregate (tests/mpnn_ref.py) against the reference's own known answers
(mpnn.test.scala, as data in tests/golden/mpnn_kats.json) and the true gradient of the message, and the part of lamp_amd.graph's MPNN
surface that needs no GPU."""
import json
import os

import torch

from lamp_amd import graph as G
from tests import mpnn_ref as R

KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "mpnn_kats.json")))
F64 = torch.float64


def test_restatement_counts_occurences():
    k = KATS["countOccurences"]
    assert R.count_occurences(torch.tensor(k["t"]), k["elems"]).tolist() == k["expected"]


def test_restatement_reproduces_every_aggregate_kat():
    """the seven flag combinations of mpnn.test.scala; the last one rounded to 4 decimals as the reference rounds it"""
    k = KATS["aggregate"]
    msg, ei, ej = torch.tensor(k["message"], dtype=F64), torch.tensor(k["edgeI"]), torch.tensor(k["edgeJ"])
    assert len(k["cases"]) == 7
    for case in k["cases"]:
        out = R.aggregate(k["numVertices"], msg, ei, ej, case["degreeNormalizeI"], case["degreeNormalizeJ"], case["aggregateJ"])
        if case["roundTo"] is not None:
            out = torch.round(out * 10 ** case["roundTo"]) / 10 ** case["roundTo"]
        assert out.tolist() == case["expected"], case


def test_the_factor_is_an_f32_value():
    """torch's pow of an integer tensor is f32, so an f64 factor is an f32 value widened: 2^-1/2 in f32, not in f64"""
    f = R.degree_factor(torch.tensor([0, 0, 1]), 3, -0.5)
    assert f.dtype == F64 and f[0].item() == torch.tensor(2.0, dtype=torch.float32).rsqrt().double().item() and f[0].item() != 2.0 ** -0.5
    assert f[1].item() == 1.0 and f[2].item() == float("inf")


def test_message_gradient_is_out_degree_plus_in_degree():
    """all-ones dmsg: dx[n, :] = outdeg(n) + indeg(n), the true gradient (IndexSelect's literal closure would double what x already holds)"""
    ei, ej = torch.tensor([0, 0, 1, 3, 3, 3]), torch.tensor([1, 2, 2, 0, 3, 1])
    x = torch.arange(8, dtype=F64).reshape(4, 2).requires_grad_(True)
    ef = torch.arange(18, dtype=F64).reshape(6, 3).requires_grad_(True)
    msg = R.message(x, ef, ei, ej)
    assert list(msg.shape) == [6, 3 + 2 * 2]
    assert torch.equal(msg[3], torch.cat([ef[3], x[3], x[0]]).detach())
    msg.sum().backward()
    degree = torch.bincount(ei, minlength=4) + torch.bincount(ej, minlength=4)
    assert torch.equal(x.grad, degree.double().unsqueeze(1).expand(4, 2)) and torch.equal(ef.grad, torch.ones(6, 3, dtype=F64))


def test_python_surface_without_a_gpu():
    """the switch returns the previous setting, the split threshold comes from the library, the public names exist"""
    assert G.mpnnFused(False) is True and G.mpnnFused(True) is False and G.mpnnFused(True) is True
    assert G.mpnnLongRow() >= 64
    for name in ("MPNN", "mpnnMessage", "mpnnMessageComposed", "mpnnAggregate", "mpnnAggregateComposed", "mpnnFused", "mpnnLongRow", "countOccurences"):
        assert hasattr(G, name), name
    for name in ("forward", "state", "parameters", "zeroGrad", "asEval", "asTraining", "load"):
        assert hasattr(G.MPNN, name), name
