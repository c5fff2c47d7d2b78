"""lamp.nn.graph's GraphAttention on the GPU, everything through lamp_amd.graph: the reference's known answer, the fused
GraphAttentionAggregate node and the composed chain against the f64 restatement (tests/graph_attention_ref.py) with a tolerance measured on
the composed chain, invariance under a shift per destination, bitwise run-to-run equality, the launch budget, the error paths, and a
two-layer attention network that has to beat the same network without attention on a planted-community graph."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from lamp_amd import autograd as A, graph as G, nn, sten as S
from lamp_amd._capi import lib, LampError
from tests import graph_attention_ref as R
from tests.test_graph_gpu import _planted_graph, _random_edges, _timer_counts
from tests.util import closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu
F64 = torch.float64
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "graph_attention_kats.json")))
# The rule e_f <= 4 * e_c + FLOOR_EPS * eps of tests/test_graph_gpu.py: e_c / e_f are the max-abs errors of the composed chain and of the
# fused node against the f64 restatement over the restatement's max magnitude, for out, dscore and dvalue through a fixed linear
# functional, on closed-form operands rounded to the type (scores multiples of 1/8 in [-4, 4], values in [-2, 2]).
# Measured on an MI355X, max over out, dscore and dvalue, in multiples of the type's eps ("needed" = (e_f - 4 e_c) / eps where positive):
#   case          f32 e_c   f32 e_f   needed   f64 e_c   f64 e_f   needed
#   n1            0.00      0.00      0.00     0.00      0.00      0.00
#   kat           7.11      9.24      0.00     13.76     11.61     0.00
#   n70_1x1       2.26      1.54      0.00     5.72      3.81      0.00
#   n70_1x64      2.75      1.87      0.00     2.59      3.21      0.00
#   n70_1x65      2.40      1.69      0.00     3.01      2.23      0.00
#   n70_2x3       3.46      3.25      0.00     2.60      3.09      0.00
#   n70_3x17      2.84      2.43      0.00     3.07      3.12      0.00
#   n70_4x16      2.82      3.91      0.00     4.71      4.27      0.00
#   n70_4x65      2.92      3.22      0.00     4.82      3.10      0.00
#   n70_8x64      3.02      3.36      0.00     4.38      4.66      0.00
#   hole          1.94      2.55      0.00     3.69      2.31      0.00
#   hub_in        9.89      0.50      0.00     9.89      3.71      0.00
#   hub_out       5.05      3.80      0.00     5.90      3.47      0.00
#   hub_in_4x16   13.62     1.40      0.00     13.62     4.25      0.00
#   hub_out_4x16  6.61      3.87      0.00     11.09     5.28      0.00
#   shifted       3.46      3.25      0.00     2.60      3.09      0.00     (e_c of the unshifted run, e_f of the shifted one)
# No case needs a floor, so twice the measured need is 0 and the floor is the count of the fused form's own roundings per element beyond
# the sums (s, the weighted row, the dot products), each half an ulp unless said otherwise: score - m, which enters exp and is worth
# |score - m| <= 8 half-ulps = 4 eps of the weight; exp itself, 1 eps; the weight times the value, 0.5; the division by s, 0.5; one rescale
# of the sums per new maximum (exp 1 eps and a product 0.5, rarely more than once past the first edges), 1.5; 7.5 eps, rounded up to 8.
# (Before the score gradient took m and s from the scores again, a = exp(score - lse) needed 16.25 eps in the shifted case: lse near 64
# has lost six bits.  That was a fault of the code and was fixed there, not covered by the floor.)
FLOOR_EPS = 8
MAX_COMPOSED_EPS = 64      # e_c above this means the chain is broken, and a broken chain must not loosen the rule
MEASURED_COMPOSED_EPS = 14 # the largest e_c of the table above (13.76, the known answer in f64; 13.62 in f32), rounded up


def _long_row():
    return G.gatLongRow()


@functools.lru_cache(maxsize=None)
def _graph(name):
    """-> (N, edgeI, edgeJ); self loops are the last N edges unless the case says otherwise"""
    loops = lambda n: torch.arange(n, dtype=torch.int64)
    if name == "n1":
        return 1, loops(1), loops(1)
    if name == "kat":
        return KATS["numNodes"], torch.tensor(KATS["edgeI"]), torch.tensor(KATS["edgeJ"])
    if name in ("n70", "hole"):
        i, j = _random_edges(70, 300, 5)
        i, j = torch.cat([i, loops(70)]), torch.cat([j, loops(70)])
        if name == "hole":                    # nothing arrives at node 5, its self loop included
            keep = j != 5
            assert int((~keep).sum()) > 1
            i, j = i[keep], j[keep]
        return 70, i, j
    if name in ("hub_in", "hub_out"):
        # N = 2L + 4.  Into node 0: nodes 1 .. 2L + 2 and itself, 2L + 3 edges (split, uneven shares); into node 1: nodes 3 .. L + 1 and itself,
        # L edges (the longest row one wave takes); into node 2: nodes L + 2 .. 2L + 1 and itself, L + 1 edges (the shortest split row)
        l = _long_row()
        n = 2 * l + 4
        pairs = [(k, 0) for k in range(1, 2 * l + 3)] + [(k, 1) for k in range(3, l + 2)] + [(k, 2) for k in range(l + 2, 2 * l + 2)]
        order = torch.tensor([(p * 7919) % len(pairs) for p in range(len(pairs))])          # a fixed shuffle: 7919 is prime
        assert sorted(order.tolist()) == list(range(len(pairs)))
        src, dst = torch.tensor([p[0] for p in pairs])[order], torch.tensor([p[1] for p in pairs])[order]
        src, dst = torch.cat([src, loops(n)]), torch.cat([dst, loops(n)])
        deg = torch.bincount(dst, minlength=n)
        assert deg[0] == 2 * l + 3 and deg[1] == l and deg[2] == l + 1
        return (n, src, dst) if name == "hub_in" else (n, dst, src)
    raise KeyError(name)


# case -> (graph, H, V).  The 70-node shapes: scalar (1, 1), 16-byte packets and the packet form of the score gradient (1, 64), (4, 16),
# scalar with H * V past one wave's columns (1, 65), (4, 65), a head boundary inside an 8-byte packet (2, 3), odd everything (3, 17), and
# packets over more than one column tile, in the gathers and in the packet form of the score gradient (8, 64).
CASES = {"n1": ("n1", 1, 1), "kat": ("kat", 2, 3)}
CASES.update({f"n70_{h}x{v}": ("n70", h, v) for h, v in ((1, 1), (1, 64), (1, 65), (2, 3), (3, 17), (4, 16), (4, 65), (8, 64))})
CASES.update({"hole": ("hole", 2, 3), "hub_in": ("hub_in", 2, 3), "hub_out": ("hub_out", 2, 3), "hub_in_4x16": ("hub_in", 4, 16),
              "hub_out_4x16": ("hub_out", 4, 16)})
KEYS = ("out", "dscore", "dvalue")


@functools.lru_cache(maxsize=None)
def _problem(name, dt, shifted=False):
    """closed-form operands rounded to dt (as f64) and the restatement's result and gradients, computed once per case.  shifted: +64 on
    the scores of even destinations, -64 on those of odd ones (exact: the scores are multiples of 1/8 below 4 in magnitude)"""
    g, h, v = CASES[name]
    n, ei, ej = _graph(g)
    rd = lambda t: t.to(dt).to(F64)
    score = torch.round(closed_form((ei.numel(), h), 11, 8.0, F64) * 8) / 8
    if shifted:
        score = score + torch.where(ej % 2 == 0, 64.0, -64.0).to(F64).unsqueeze(1)
        assert torch.equal(rd(score), score)
    value, lf = rd(closed_form((n, h, v), 7, 4.0, F64)), rd(closed_form((n, h * v), 301, 1.0, F64))
    sr, vr = score.clone().requires_grad_(True), value.clone().requires_grad_(True)
    out = R.attention_aggregate(sr, vr, ei, ej)
    (out * lf).sum().backward()
    return n, ei, ej, h, score, value, lf, {"out": out.detach(), "dscore": sr.grad.detach(), "dvalue": vr.grad.detach()}


def _library(name, dt, fused, csr=None, shifted=False, transposed=False, device=0):
    n, ei, ej, h, score, value, lf, _ = _problem(name, dt, shifted)
    prev = G.graphAttentionFused(fused)
    try:
        ts = lambda t: to_sten(t.to(dt), device=device)
        if transposed:                         # an [H, E] buffer read as [E, H]
            sv = A.param(ts(score.t().contiguous()).t)
            assert sv.value.strides == [1, score.shape[0]] or score.shape[1] == 1
        else:
            sv = A.param(ts(score))
        vv = A.param(ts(value))
        out = G.graphAttentionAggregate(sv, vv, to_sten(ei, device=device), to_sten(ej, device=device), h, csr)
        (out * A.const(ts(lf))).sum().backprop()
        return {"out": to_torch(out.value), "dscore": to_torch(sv.partialDerivative), "dvalue": to_torch(vv.partialDerivative)}
    finally:
        G.graphAttentionFused(prev)


def _err(got, ref):
    assert list(got.shape) == list(ref.shape), f"shape {list(got.shape)} vs {list(ref.shape)}"
    den = ref.abs().max().item()
    return (got.double() - ref).abs().max().item() / (den if den > 0 else 1.0)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_and_composed_vs_restatement(gpu, name, dt):
    """out, dscore, dvalue: e_f <= 4 * e_c + FLOOR_EPS * eps, and e_c <= 64 eps.  Figures are printed (-s)."""
    ref = _problem(name, dt)[-1]
    comp, fus = _library(name, dt, fused=False), _library(name, dt, fused=True)
    floor = FLOOR_EPS * EPS[dt]
    bad = []
    for key in KEYS:
        e_c, e_f = _err(comp[key], ref[key]), _err(fus[key], ref[key])
        print(f"PARITY {name} {key} {dt}: e_c {e_c:.3e} ({e_c / EPS[dt]:.2f} eps) e_f {e_f:.3e} ({e_f / EPS[dt]:.2f} eps) needed {max(0.0, e_f - 4 * e_c) / EPS[dt]:.2f} eps")
        if not e_c <= MAX_COMPOSED_EPS * EPS[dt]:
            bad.append(f"{key}: composed error {e_c:.3e} > {MAX_COMPOSED_EPS} eps")
        if not e_f <= 4 * e_c + floor:
            bad.append(f"{key}: fused error {e_f:.3e} > 4 * composed error {e_c:.3e} + {floor:.1e}")
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_hole_gives_zeros_and_no_nan(gpu, dt):
    """node 5 has no incoming edge: its output row is zero, the restatement's too, and nothing is NaN anywhere"""
    fus = _library("hole", dt, fused=True)
    for key in KEYS:
        assert not torch.isnan(fus[key]).any(), key
    assert torch.equal(fus["out"][5], torch.zeros_like(fus["out"][5]))
    assert torch.equal(_problem("hole", dt)[-1]["out"][5], torch.zeros(6, dtype=F64))


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_shift_per_destination_is_free(gpu, dt):
    """the (2, 3) problem with +64 / -64 on the scores by destination: the fused error against the restatement of the shifted problem obeys
    the rule with the composed error of the unshifted run (the chain itself underflows to log(0) under one global maximum)"""
    name = "n70_2x3"
    comp = _library(name, dt, fused=False)
    fus = _library(name, dt, fused=True, shifted=True)
    plain, shifted = _problem(name, dt)[-1], _problem(name, dt, True)[-1]
    for key in KEYS:
        e_c, e_f = _err(comp[key], plain[key]), _err(fus[key], shifted[key])
        print(f"SHIFTED {key} {dt}: e_c {e_c:.3e} e_f {e_f:.3e} needed {max(0.0, e_f - 4 * e_c) / EPS[dt]:.2f} eps")
        assert e_c <= MAX_COMPOSED_EPS * EPS[dt]
        assert e_f <= 4 * e_c + FLOOR_EPS * EPS[dt], key


def test_transposed_score_gives_the_bits_of_its_contiguous_copy(gpu):
    a = _library("n70_3x17", torch.float32, fused=True)
    b = _library("n70_3x17", torch.float32, fused=True, transposed=True)
    for key in KEYS:
        assert torch.equal(a[key], b[key]), key


def _kat_args(device, dot, dt=F64):
    ts = lambda name: A.const(to_sten(torch.tensor(KATS[name], dtype=dt), device=device))
    ei, ej = to_sten(torch.tensor(KATS["edgeI"]), device=device), to_sten(torch.tensor(KATS["edgeJ"]), device=device)
    return (ts("nodes"), ts("edges"), ei, ej, ts("wNodeKey1"), ts("wNodeKey2"), ts("wEdgeKeyDot" if dot else "wEdgeKey"), ts("wNodeValue"),
            None if dot else ts("wAttention"), KATS["numHeads"])


@pytest.mark.parametrize("dot", [False, True], ids=["tanh", "dot"])
@pytest.mark.parametrize("device", [0, S.CPU], ids=["gpu", "cpu"])
def test_reference_kat(gpu, device, dot):
    """graphattention.test.scala:17-158 in f64, both scoring branches: fused and composed on the GPU, and multiheadGraphAttention on
    lamp's CPU device (host tensors are staged through the GPU)"""
    want = torch.tensor(KATS["restatement"], dtype=F64)
    forms = [(True, G.multiheadGraphAttention), (False, G.multiheadGraphAttention)] + ([(True, G.multiheadGraphAttentionComposed)] if device == 0 else [])
    for fused, fn in forms:
        prev = G.graphAttentionFused(fused)
        try:
            out = fn(*_kat_args(device, dot))
        finally:
            G.graphAttentionFused(prev)
        assert out.value.device == device and out.shape == KATS["expectedShape"]
        got = to_torch(out.value)
        assert round(got[0, 0].item(), 10) == KATS["expected_0_0"] and round(got[0, 3].item(), 10) == KATS["expected_0_3"], (fused, fn.__name__)
        assert (got - want).abs().max().item() <= 1e-10, (fused, fn.__name__)


@pytest.mark.parametrize("dot", [False, True], ids=["tanh", "dot"])
def test_module_kat(gpu, dot):
    """the reference's two constructor calls: a 5 x 6 result, five state tensors with wAttention and four without"""
    m = KATS["module"]
    layer = G.GraphAttention.apply(m["nodeDim"], m["edgeDim"], m["attentionKeyHiddenDimPerHead"], m["attentionNumHeads"], m["valueDimPerHead"], m["dropout"],
                                   S.F64, 0, dotProductAttention=dot, nonLinearity=m["nonLinearity"])
    nodes, edges, ei, ej = _kat_args(0, dot)[:4]
    out = layer.forward(G.Graph(nodes, edges, ei, ej, to_sten(torch.zeros(5, dtype=torch.int64))))
    assert out.nodeFeatures.shape == m["shape"]
    assert len(layer.state) == (m["stateDotProduct"] if dot else m["stateWithAttention"]) and len(layer.parameters) == len(layer.state)
    assert [v.shape for v in layer.state[:4]] == [[3, 4], [3, 4], [2, 2] if dot else [2, 4], [3, 6]]
    assert not torch.isnan(to_torch(out.nodeFeatures.value)).any()
    layer.load([S.STen.ones(v.shape, S.F64, 0) for v in layer.state])
    assert all(bool((to_torch(v.value) == 1).all()) for v in layer.state)
    assert layer.asEval().training is False and layer.asTraining().training is True


@pytest.mark.parametrize("name", ["n70_3x17", "hub_in"])
def test_fused_is_bitwise_reproducible(gpu, name):
    """two runs, and two edge CSRs built from one edge list: the same bits in out, dscore and dvalue"""
    dt = torch.float32
    n, ei, ej = _problem(name, dt)[:3]
    a, b = _library(name, dt, fused=True), _library(name, dt, fused=True)
    csr1, csr2 = G.computeEdgeCsr(to_sten(ei), to_sten(ej), n), G.computeEdgeCsr(to_sten(ei), to_sten(ej), n)
    for t1, t2 in zip(csr1.tensors, csr2.tensors):
        assert torch.equal(to_torch(t1), to_torch(t2))
    c, d = _library(name, dt, fused=True, csr=csr1), _library(name, dt, fused=True, csr=csr2)
    for key in KEYS:
        assert torch.equal(a[key], b[key]) and torch.equal(a[key], c[key]) and torch.equal(c[key], d[key]), key


def test_edge_csr_groups_in_edge_list_order(gpu):
    """rowptr and perm of both groupings against torch's stable sort; E = 0 is valid"""
    n, ei, ej = _graph("n70")
    csr = G.computeEdgeCsr(to_sten(ei), to_sten(ej), n)
    for (rowptr, perm), index in ((csr.incoming, ej), (csr.outgoing, ei)):
        assert to_torch(perm).tolist() == torch.sort(index, stable=True).indices.tolist()
        assert to_torch(rowptr).tolist() == [0] + torch.cumsum(torch.bincount(index, minlength=n), 0).tolist()
    none = to_sten(torch.zeros(0, dtype=torch.int64))
    empty = G.computeEdgeCsr(none, none, 3)
    assert to_torch(empty.inRowptr).tolist() == [0, 0, 0, 0] and empty.inPerm.shape == [0]


def test_launch_budget(gpu):
    """prebuilt CSR: forward + backward run gat_forward, gat_backward_score and gat_backward_value once each, no other gat_ kernel and no
    index_add; with graphAttentionFused(False) no gat_ kernel runs and index_add does - a fused path that fell back would show here"""
    dt, name = torch.float32, "n70_4x16"
    n, ei, ej = _problem(name, dt)[:3]
    csr = G.computeEdgeCsr(to_sten(ei), to_sten(ej), n)
    fused = _timer_counts(lambda: _library(name, dt, fused=True, csr=csr))
    assert {k: v for k, v in fused.items() if k.startswith("gat_")} == {"gat_forward": 1, "gat_backward_score": 1, "gat_backward_value": 1}, fused
    assert "index_add" not in fused and "graph_edge_rowptr" not in fused, fused
    composed = _timer_counts(lambda: _library(name, dt, fused=False, csr=csr))
    assert not any(k.startswith("gat_") for k in composed) and composed.get("index_add", 0) >= 1, composed
    built = _timer_counts(lambda: G.computeEdgeCsr(to_sten(ei), to_sten(ej), n))
    assert built.get("graph_index_range", 0) == 2 and built.get("graph_edge_rowptr", 0) == 2 and not any(k.startswith("gat_") for k in built), built


def test_graph_caches_its_edge_csr(gpu):
    """three stacked layers over one graph build the two groupings once"""
    n, ei, ej = _graph("n70")
    x = closed_form((n, 8), 3, 2.0, torch.float32)
    edges = A.const(to_sten(torch.ones(ei.numel(), 1)))
    graph = G.Graph(A.const(to_sten(x)), edges, to_sten(ei), to_sten(ej), None)
    layers = [G.GraphAttention.apply(8, 1, 4, 2, 4, 0.0, S.F32, 0, dotProductAttention=k == 1, nonLinearity=True) for k in range(3)]

    def run():
        g = graph
        for layer in layers:
            g = layer.forward(g)
        return g
    counts = _timer_counts(run)
    assert counts.get("graph_edge_rowptr", 0) == 2 and counts.get("gat_forward", 0) == 3, counts
    assert run().nodeFeatures.shape == [n, 8]


def test_bad_arguments_are_errors(gpu):
    """shape and type errors surface as LampError (an out-of-range endpoint is checked in the code, before anything dereferences it, and
    deliberately not fed to the GPU here)"""
    i3, j2 = to_sten(torch.tensor([0, 1, 2])), to_sten(torch.tensor([1, 2]))
    score, value = A.const(to_sten(torch.zeros(3, 2))), A.const(to_sten(torch.zeros(4, 2, 3)))
    with pytest.raises(LampError, match="differ in length"):
        G.graphAttentionAggregate(score, value, i3, j2, 2)
    with pytest.raises(LampError, match=r"score must be \[E, 3\]"):
        G.graphAttentionAggregate(score, value, i3, i3, 3)
    with pytest.raises(LampError, match="int64 vector"):
        G.computeEdgeCsr(to_sten(torch.tensor([0.0, 1.0, 2.0])), i3, 4)
    csr = G.computeEdgeCsr(i3, i3, 4)
    o, l = C.c_void_p(), C.c_void_p()
    score16, value16 = to_sten(torch.zeros(3, 2, dtype=torch.bfloat16)), to_sten(torch.zeros(4, 2, 3, dtype=torch.bfloat16))
    with pytest.raises(LampError, match="f32 and f64 only"):
        lib.lamp_gat_forward(C.byref(o), C.byref(l), score16.h, value16.h, i3.h, csr.inRowptr.h, csr.inPerm.h)
    with pytest.raises(LampError, match="heads of score"):
        G.graphAttentionAggregate(score, A.const(to_sten(torch.zeros(4, 3, 3))), i3, i3, 2, csr)


def _train(attend, fused=True, steps=30):
    """two GraphAttention layers (2 heads of 8, swish1, residual) + Linear + logSoftMax on _planted_graph with self loops and unit edge
    features.  attend = False: every node keeps its own value row (the attention replaced by the identity on nodeValue)."""
    x, i, j, label, train, held = _planted_graph()
    n = x.shape[0]
    i, j = torch.cat([i, torch.arange(n)]), torch.cat([j, torch.arange(n)])
    lib.lamp_manual_seed(7)
    layers = [G.GraphAttention.apply(16, 1, 8, 2, 8, 0.0, S.F32, 0, dotProductAttention=False, nonLinearity=True) for _ in range(2)]
    head = nn.Linear(16, 2, S.F32, 0)
    params = [p for m in layers + [head] for p in m.parameters]
    opt = nn.AdamW([p.value for p in params], 0.0, 0.01)
    graph = G.Graph(A.const(to_sten(x)), A.const(to_sten(torch.ones(i.numel(), 1))), to_sten(i), to_sten(j), None)
    weights, target, rows = S.STen.ones([2], S.F32), to_sten(label[train]), A.const(to_sten(train))

    def identity(layer, g):
        h = g.nodeFeatures.mm(layer.wNodeValue)
        return g.copy(nodeFeatures=g.nodeFeatures + h * h.sigmoid())

    def logits():
        g = graph
        for layer in layers:
            g = layer.forward(g) if attend else identity(layer, g)
        return head.forward(g.nodeFeatures).logSoftMax(1)

    prev = G.graphAttentionFused(fused)
    try:
        losses = []
        for _ in range(steps):
            for m in layers + [head]:
                m.zeroGrad()
            loss = logits().indexSelect(0, rows).nllLoss(target, weights)
            loss.backprop()
            opt.step([p.partialDerivative for p in params])
            losses.append(loss.value.item())
        pred = to_torch(logits().value).argmax(1)
    finally:
        G.graphAttentionFused(prev)
    return losses, (pred[held] == label[held]).double().mean().item()


def test_two_layer_attention_learns_and_beats_no_attention(gpu):
    """NLL on a tenth of the nodes, AdamW, 30 steps in f32: the losses are finite and fall, and the held-out accuracy exceeds what the same
    network reaches with the attention replaced by the identity on nodeValue (same seed, same data).  The composed path's step-0 loss
    agrees with the fused one's: with the chain's measured error e_c <= 14 eps the rule puts the fused node within 4 * 14 + FLOOR_EPS eps
    of the restatement, so the two paths differ by at most (5 * 14 + FLOOR_EPS) eps per attention layer, two layers, relative to a loss of
    order one (the log-softmax and the mean that follow do not amplify a relative error of the features of order one)."""
    losses, acc = _train(True)
    losses_id, acc_id = _train(False)
    first_composed = _train(True, fused=False, steps=1)[0][0]
    print(f"loss {losses[0]:.6f} -> {losses[-1]:.6f}, held-out accuracy {acc:.3f}; without attention {losses_id[0]:.6f} -> {losses_id[-1]:.6f}, {acc_id:.3f}; "
          f"composed step-0 loss {first_composed:.6f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert acc > acc_id, f"held-out accuracy {acc:.3f} with attention, {acc_id:.3f} without"
    bound = 2 * (5 * MEASURED_COMPOSED_EPS + FLOOR_EPS) * EPS[torch.float32] * max(1.0, abs(first_composed))
    assert abs(losses[0] - first_composed) <= bound, (losses[0], first_composed, bound)
