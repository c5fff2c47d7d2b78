"""lamp.nn.graph's GCN path on the GPU, everything through lamp_amd.graph: the reference's two known answers, the fused GcnAggregation
node and the composed chain against the f64 restatement (tests/graph_ref.py) with a tolerance measured on the composed chain, bitwise
run-to-run equality, symmetry, the launch budget, VertexPooling, and a two-layer GCN that has to beat the same network without
aggregation on a planted-community graph."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from lamp_amd import autograd as A, graph as G, nn, sten as S
from lamp_amd._capi import lib
from tests import graph_ref as R
from tests.util import closed_form, to_sten, to_torch, TORCH2LAMP

pytestmark = pytest.mark.gpu
F64 = torch.float64
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "graph_kats.json")))
HALF_ULP_4 = 0.5e-4 * (1 + 1e-9)
# The floor of the rule e_f <= 4 * e_c + floor (tests/test_recurrent_gpu.py), as a multiple of the dtype's eps: e_c / e_f are the max-abs
# errors of the composed chain and of the fused node against the f64 restatement over the restatement's max magnitude.
# Measured on an MI355X, max over forward and gradient ("needed" = (e_f - 4 e_c) / eps where positive):
#   case      f32 e_c   f32 e_f   needed   f64 e_c   f64 e_f   needed
#   n1        0.00e+00  0.00e+00  0.00     0.00e+00  0.00e+00  0.00
#   n5        4.19e-08  5.05e-08  0.00     6.27e-17  1.25e-16  0.00
#   n70_d1    1.63e-07  1.63e-07  0.00     2.30e-16  2.30e-16  0.00
#   n70_d3    1.13e-07  1.33e-07  0.00     2.36e-16  2.36e-16  0.00
#   n70_d64   1.61e-07  1.32e-07  0.00     3.39e-16  3.39e-16  0.00
#   n70_d65   1.53e-07  1.20e-07  0.00     3.29e-16  3.29e-16  0.00
#   n70_d130  1.65e-07  1.23e-07  0.00     3.75e-16  3.75e-16  0.00
#   n70_d260  1.77e-07  1.43e-07  0.00     4.09e-16  4.09e-16  0.00
#   pitch68   1.66e-07  1.34e-07  0.00     3.37e-16  3.30e-16  0.00
#   pitch67   1.46e-07  1.46e-07  0.00     3.30e-16  3.30e-16  0.00
#   hub_d8    2.15e-07  1.62e-07  0.00     4.54e-16  2.42e-16  0.00
#   hub_d65   5.26e-07  2.33e-07  0.00     7.35e-16  5.78e-16  0.00
# No shape needs a floor (e_f is at most 2 eps everywhere, and where e_c is exactly 0, at N = 1, so is e_f), so twice the measured need
# is 0.  The floor is kept for one case the factor 4 cannot carry: a shape on which the chain happens to be exact while the fused form
# rounds.  Its own roundings per element beyond the sum are three (dinv * x, the outer dinv, dinv itself rounded from f64), half an
# ulp each: 1.5 eps, rounded up to 2.  (The composed chain's e_c moves by some 30 % between runs - its atomics - e_f does not.)
FLOOR_EPS = 2
L = None   # lamp_gcn_long_row(), read once the library is loaded


def _long_row():
    global L
    if L is None:
        L = G.longRow()
    return L


def _random_edges(n, e, salt):
    k = torch.arange(e, dtype=torch.int64) + salt
    i = (k * 37 + 11) % n
    j = (i + 1 + (k * 53) % (n - 1)) % n          # never i itself
    return i, j


def _hub_edges():
    """N = 2L + 4: node 0 joined to all 2L + 3 others (split-row path), node 1 to exactly L (the longest row a single wave takes), node 2
    to L + 1 (the shortest split row); directions alternate"""
    l = _long_row()
    n = 2 * l + 4
    pairs = [(0, k) if k % 2 else (k, 0) for k in range(1, n)]
    pairs += [(1, k) if k % 2 else (k, 1) for k in range(3, l + 2)]       # node 1: 0 and 3 .. L + 1  -> L neighbours
    pairs += [(2, k) if k % 2 else (k, 2) for k in range(l + 2, 2 * l + 2)]   # node 2: 0 and L + 2 .. 2L + 1 -> L + 1 neighbours
    i, j = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
    deg = torch.bincount(torch.cat([i, j]), minlength=n)
    assert deg[0] == 2 * l + 3 and deg[1] == l and deg[2] == l + 1
    return n, i, j


def _case(name):
    """-> (N, edgeI, edgeJ, D, row pitch or None)"""
    if name == "n1":
        return 1, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 3, None
    if name == "n5":   # node 4 isolated, 0-1 twice, 2-3 both ways, unsorted
        return 5, torch.tensor([3, 0, 1, 2, 0]), torch.tensor([2, 1, 2, 3, 1]), 4, None
    if name.startswith("n70_d"):
        i, j = _random_edges(70, 300, 5)
        return 70, i, j, int(name[5:]), None
    if name.startswith("pitch"):
        i, j = _random_edges(70, 300, 9)
        return 70, i, j, 64, int(name[5:])
    if name.startswith("hub_d"):
        n, i, j = _hub_edges()
        return n, i, j, int(name[5:]), None
    raise KeyError(name)


CASES = ["n1", "n5"] + [f"n70_d{d}" for d in (1, 3, 64, 65, 130, 260)] + ["pitch68", "pitch67", "hub_d8", "hub_d65"]


@functools.lru_cache(maxsize=None)
def _problem(name, dt):
    """closed-form operands rounded to dt (as f64) and the restatement's result and gradient, computed once per case"""
    n, ei, ej, d, pitch = _case(name)
    rd = lambda t: t.to(dt).to(F64)
    x, lf = rd(closed_form((n, d), 7, 2.0, F64)), rd(closed_form((n, d), 301, 1.0, F64))
    xr = x.clone().requires_grad_(True)
    out = R.gcn_aggregation(xr, ei, ej)
    (out * lf).sum().backward()
    return n, ei, ej, d, pitch, x, lf, {"out": out.detach(), "dx": xr.grad.detach()}


def _library(name, dt, fused, device=0, adjacency=None):
    n, ei, ej, d, pitch, x, lf, _ = _problem(name, dt)
    prev = G.gcnFused(fused)
    try:
        ts = lambda t: to_sten(t.to(dt), device=device)
        if pitch is None:
            xv = A.param(ts(x))
        else:
            wide = torch.zeros(n, pitch, dtype=F64)
            wide[:, :d] = x
            xv = A.param(ts(wide).narrow(1, 0, d))
            assert xv.value.strides == [pitch, 1]
        si, sj = to_sten(ei, device=device), to_sten(ej, device=device)
        out = G.gcnAggregation(xv, adjacency) if adjacency is not None else G.gcnAggregation(xv, si, sj)
        (out * A.const(ts(lf))).sum().backprop()
        return {"out": to_torch(out.value), "dx": to_torch(xv.partialDerivative)}
    finally:
        G.gcnFused(prev)


def _err(got, ref):
    assert list(got.shape) == list(ref.shape), f"shape {list(got.shape)} vs {list(ref.shape)}"
    den = ref.abs().max().item()
    return (got.double() - ref).abs().max().item() / (den if den > 0 else 1.0)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", CASES)
def test_fused_and_composed_vs_restatement(gpu, name, dt):
    """forward and gradient (through a fixed linear functional): e_f <= 4 * e_c + FLOOR_EPS * eps.  Figures are printed (-s)."""
    ref = _problem(name, dt)[-1]
    comp, fus = _library(name, dt, fused=False), _library(name, dt, fused=True)
    floor = FLOOR_EPS * EPS[dt]
    for key, r in ref.items():
        e_c, e_f = _err(comp[key], r), _err(fus[key], r)
        print(f"{name} {key} {dt}: e_c {e_c:.3e} e_f {e_f:.3e} needed {max(0.0, e_f - 4 * e_c) / EPS[dt]:.2f} eps")
        assert e_f <= 4 * e_c + floor, f"{name}: {key}: fused error {e_f:.3e} > 4 * composed error {e_c:.3e} + {floor:.1e}"


@pytest.mark.parametrize("device", [0, S.CPU], ids=["gpu", "cpu"])
def test_reference_kats(gpu, device):
    """gcn.test.scala:23-125 in f64 on the GPU and on lamp's CPU device (host tensors are staged through the GPU)"""
    ei, ej = to_sten(torch.tensor(KATS["edgeI"]), device=device), to_sten(torch.tensor(KATS["edgeJ"]), device=device)
    ts = lambda rows: to_sten(torch.tensor(rows, dtype=F64), device=device)
    adj = G.computeAdjacency(ei, ej, KATS["numNodes"], S.F64)
    assert adj.rowptr.device == device and adj.rowptr.to_numpy().tolist() == [0, 3, 4, 5, 6] and adj.col.to_numpy().tolist() == [1, 2, 3, 0, 0, 0]
    assert np.allclose(adj.dinv.to_numpy() ** -2.0, KATS["degreesPlusOne"], rtol=1e-15)
    k = KATS["aggregation"]
    for fused in (True, False):
        prev = G.gcnFused(fused)
        try:
            out = G.gcnAggregation(A.const(ts(k["nodes"])), ei, ej)
            assert out.value.device == device
            assert (to_torch(out.value) - torch.tensor(k["expected"], dtype=F64)).abs().max().item() <= HALF_ULP_4, f"fused={fused}"
        finally:
            G.gcnFused(prev)
    k = KATS["module"]
    linear = nn.Linear(4, 3, S.F64, device, bias=True)
    linear.load([S.STen.ones(v.shape, S.F64, device) for v in linear.state])
    module = G.GCN(G.ResidualModule(nn.Sequential(linear, nn.Fun("relu"))))
    graph = G.Graph(A.const(ts(k["nodes"])), None, ei, ej, None)
    out = module.forward(graph).nodeFeatures
    assert out.shape == [4, 3] and len(module.state) == 2
    assert (to_torch(out.value) - torch.tensor(k["expected"], dtype=F64)).abs().max().item() <= HALF_ULP_4


@pytest.mark.parametrize("name", ["n70_d65", "hub_d8"])
def test_fused_is_bitwise_reproducible(gpu, name):
    """two runs, and two adjacency objects built from one edge list: the same bits, forward and gradient"""
    dt = torch.float32
    n, ei, ej = _problem(name, dt)[:3]
    a = _library(name, dt, fused=True)
    b = _library(name, dt, fused=True)
    adj1 = G.computeAdjacency(to_sten(ei), to_sten(ej), n, TORCH2LAMP[dt])
    adj2 = G.computeAdjacency(to_sten(ei), to_sten(ej), n, TORCH2LAMP[dt])
    for t1, t2 in zip(adj1.tensors, adj2.tensors):
        assert torch.equal(to_torch(t1), to_torch(t2))
    c, d = _library(name, dt, fused=True, adjacency=adj1), _library(name, dt, fused=True, adjacency=adj2)
    for key in ("out", "dx"):
        assert torch.equal(a[key], b[key]) and torch.equal(a[key], c[key]) and torch.equal(c[key], d[key]), key


def _asymmetry(name, fused):
    """|<agg(x), y> - <x, agg(y)>| over sum |agg(x)| |y| in f64"""
    n, ei, ej, d = _problem(name, F64)[:4]
    x, y = closed_form((n, d), 17, 2.0, F64), closed_form((n, d), 401, 2.0, F64)
    prev = G.gcnFused(fused)
    try:
        si, sj = to_sten(ei), to_sten(ej)
        ax = to_torch(G.gcnAggregation(A.const(to_sten(x)), si, sj).value)
        ay = to_torch(G.gcnAggregation(A.const(to_sten(y)), si, sj).value)
    finally:
        G.gcnFused(prev)
    return abs(((ax * y).sum() - (x * ay).sum()).item()) / (ax.abs() * y.abs()).sum().item()


@pytest.mark.parametrize("name", ["n70_d65", "hub_d8"])
def test_operator_is_symmetric(gpu, name):
    """<agg(x), y> = <x, agg(y)> in f64, to the bound of the parity test (the composed chain's own asymmetry as e_c)"""
    s_c, s_f = _asymmetry(name, False), _asymmetry(name, True)
    print(f"{name}: asymmetry composed {s_c:.3e} fused {s_f:.3e}")
    assert s_f <= 4 * s_c + FLOOR_EPS * EPS[F64]


def _timer_counts(fn):
    lib.lamp_device_synchronize()
    buf = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_report(buf, len(buf))            # clears the log
    lib.lamp_kernel_timer_enable(1)
    try:
        fn()
        lib.lamp_device_synchronize()
    finally:
        lib.lamp_kernel_timer_enable(0)
    lib.lamp_kernel_timer_report(buf, len(buf))
    counts = {}
    for line in buf.value.decode().splitlines():
        f = line.split()
        counts[f[0]] = int(f[1])
    return counts


def test_launch_budget(gpu):
    """prebuilt adjacency: forward + backward run the gcn_aggregate kernel exactly twice, no other gcn_ kernel and no index_add; with
    gcnFused(False) no gcn_ kernel runs and index_add does - a fused path that fell back would show here"""
    dt = torch.float32
    n, ei, ej = _problem("n70_d64", dt)[:3]
    adj = G.computeAdjacency(to_sten(ei), to_sten(ej), n, S.F32)
    fused = _timer_counts(lambda: _library("n70_d64", dt, fused=True, adjacency=adj))
    assert fused.get("gcn_aggregate", 0) == 2, fused
    assert [k for k in fused if k.startswith("gcn_")] == ["gcn_aggregate"] and "index_add" not in fused, fused
    composed = _timer_counts(lambda: _library("n70_d64", dt, fused=False, adjacency=adj))
    assert not any(k.startswith("gcn_") for k in composed) and composed.get("index_add", 0) >= 1, composed
    built = _timer_counts(lambda: G.computeAdjacency(to_sten(ei), to_sten(ej), n, S.F32))
    assert built.get("gcn_index_range", 0) == 1 and built.get("gcn_rowptr_dinv", 0) == 1 and "gcn_aggregate" not in built, built


def test_graph_caches_its_adjacency(gpu):
    """three stacked layers over one graph build the adjacency once"""
    n, ei, ej, d, _, x = _problem("n70_d64", torch.float32)[:6]
    graph = G.Graph(A.const(to_sten(x.float())), None, to_sten(ei), to_sten(ej), None)
    layers = [G.gcn(d, d, S.F32, 0) for _ in range(3)]
    def run():
        g = graph
        for layer in layers:
            g = layer.forward(g)
        return g
    counts = _timer_counts(run)
    assert counts.get("gcn_rowptr_dinv", 0) == 1 and counts.get("gcn_aggregate", 0) == 3, counts
    assert run().nodeFeatures.shape == [n, d]


def test_bad_edge_lists_are_errors(gpu):
    """shape and type errors surface as exceptions (an out-of-range endpoint is checked in the code, before anything dereferences it, and
    deliberately not fed to the GPU here)"""
    from lamp_amd._capi import LampError
    i3, j2 = to_sten(torch.tensor([0, 1, 2])), to_sten(torch.tensor([1, 2]))
    with pytest.raises(LampError, match="differ in length"):
        G.computeAdjacency(i3, j2, 4, S.F32)
    with pytest.raises(LampError, match="f32 and f64 only"):
        G.computeAdjacency(i3, i3, 4, S.BF16)
    with pytest.raises(LampError, match="int64 vector"):
        G.computeAdjacency(to_sten(torch.tensor([0.0, 1.0])), j2, 4, S.F32)


@pytest.mark.parametrize("pooling", ["Sum", "Mean"])
def test_vertex_pooling(gpu, pooling):
    """a batch of three graphs (5, 1 and 4 nodes) against the restatement, value and gradient, f64"""
    x = closed_form((10, 6), 3, 2.0, F64)
    lf = closed_form((3, 6), 31, 1.0, F64)
    idx = torch.tensor([0, 0, 0, 0, 0, 1, 2, 2, 2, 2])
    xr = x.clone().requires_grad_(True)
    ref = R.vertex_pooling(xr, idx, pooling)
    (ref * lf).sum().backward()
    xv = A.param(to_sten(x))
    graph = G.Graph(xv, None, to_sten(torch.tensor([0, 5])), to_sten(torch.tensor([1, 6])), to_sten(idx))
    out = G.VertexPooling(graph, pooling)
    (out * A.const(to_sten(lf))).sum().backprop()
    assert _err(to_torch(out.value), ref.detach()) <= 8 * EPS[F64]
    assert _err(to_torch(xv.partialDerivative), xr.grad) <= 8 * EPS[F64]


def _planted_graph():
    """two communities of 100 nodes, 800 edges (9 in 10 inside a community), 16 features of unit noise plus a class shift of +-0.15 per
    feature, labels on every tenth node; fixed seed"""
    g = torch.Generator().manual_seed(20)
    n, e, d = 200, 800, 16
    label = torch.arange(n) % 2
    i = torch.randint(0, n, (e,), generator=g)
    same = torch.rand(e, generator=g) < 0.9
    off = torch.randint(1, n // 2, (e,), generator=g) * 2            # an even offset stays in the community and is never 0
    j = torch.where(same, (i + off) % n, (i + off + 1) % n)
    assert bool((i != j).all())
    x = torch.randn(n, d, generator=g) + 0.15 * (2.0 * label.double().unsqueeze(1) - 1.0).float()
    train = torch.arange(0, n, 10) + torch.arange(n // 10) % 2      # 0, 11, 20, 31, ...: ten nodes of each community
    held = torch.tensor(sorted(set(range(n)) - set(train.tolist())))
    return x.float(), i, j, label, train, held


def _train(aggregate):
    x, i, j, label, train, held = _planted_graph()
    lib.lamp_manual_seed(7)
    layers = [G.gcn(16, 16, S.F32, 0), G.gcn(16, 16, S.F32, 0)]
    head = nn.Linear(16, 2, S.F32, 0)
    params = [p for m in layers + [head] for p in m.parameters]
    opt = nn.AdamW([p.value for p in params], 0.0, 0.01)
    graph = G.Graph(A.const(to_sten(x)), None, to_sten(i), to_sten(j), None)
    weights, target, rows = S.STen.ones([2], S.F32), to_sten(label[train]), A.const(to_sten(train))

    def logits():
        g = graph
        for layer in layers:
            g = layer.forward(g) if aggregate else g.copy(nodeFeatures=layer.transform.forward(g.nodeFeatures))
        return head.forward(g.nodeFeatures).logSoftMax(1)

    losses = []
    for _ in range(30):
        for m in layers + [head]:
            m.zeroGrad()
        loss = logits().indexSelect(0, rows).nllLoss(target, weights)
        loss.backprop()
        opt.step([p.partialDerivative for p in params])
        losses.append(loss.value.item())
    pred = to_torch(logits().value).argmax(1)
    return losses, (pred[held] == label[held]).double().mean().item()


def test_two_layer_gcn_learns_and_beats_no_aggregation(gpu):
    """two gcn layers + Linear + logSoftMax, NLL on a tenth of the nodes, AdamW, 30 steps in f32: the loss falls, and the held-out
    accuracy exceeds what the same network reaches with the aggregation replaced by the identity (same seed, same data)"""
    losses, acc = _train(True)
    losses_id, acc_id = _train(False)
    print(f"loss {losses[0]:.4f} -> {losses[-1]:.4f}, held-out accuracy {acc:.3f}; without aggregation {losses_id[0]:.4f} -> {losses_id[-1]:.4f}, {acc_id:.3f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert acc > acc_id, f"held-out accuracy {acc:.3f} with aggregation, {acc_id:.3f} without"
