"""lamp.nn.graph's MPNN on the GPU, everything through lamp_amd.graph: the reference's known answers, the fused MpnnMessage and
MpnnAggregate nodes and the composed chains against the f64 restatement (tests/mpnn_ref.py) with a tolerance measured on the composed
chain, bitwise equality of the copies and of repeated runs, the true gradient of nodeFeatures, strided inputs, the launch budget, the
error paths, and the MPNN module on a planted-community graph."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from lamp_amd import autograd as A, graph as G, nn, sten as S
from lamp_amd._capi import lib, LampError
from tests import mpnn_ref as R
from tests.test_graph_gpu import _planted_graph, _random_edges, _timer_counts
from tests.util import closed_form, to_sten, to_torch, TORCH2LAMP

pytestmark = pytest.mark.gpu
F64 = torch.float64
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "mpnn_kats.json")))
# The rule e_f <= 4 * e_c + FLOOR_EPS * eps with e_c <= 64 eps of tests/test_graph_gpu.py and tests/test_graph_attention_gpu.py: e_c / e_f
# are the max-abs errors of the composed chain and of the fused node against the f64 restatement over the restatement's max magnitude,
# for msg, dedge and dx (the message) and out and dmsg (the aggregate) through a fixed linear functional, on closed-form operands rounded to
# the type.
# The floor, from the fused form's own roundings per element beyond the sums: msg and dedge are copies (none); dx is the chain's two sums
# (over the outgoing and the incoming edges) added as the chain adds them, and nothing else (none); a term of out is
# (message * fI) * fJ and an element of dmsg ((dout_j + dout_i) * fJ) * fI, multiplied in the chain's order and not contracted into the
# additions, so every term has the chain's bits and carries no rounding the chain's does not, and the two partial sums of out are added
# last, as in the chain; the factors are the restatement's own f32 values (1 / sqrt(count) in two f32 roundings, or 1 / count), bit for
# bit.  None per term, none per element: the floor is 0.  The forms differ in the order of the additions inside a sum alone, which the
# factor 4 has to carry; where a sum has at most two terms (n1, kat) they agree bit for bit.
# Measured on an MI355X, max over the case's tensors, in multiples of the type's eps ("needed" = (e_f - 4 e_c) / eps where positive):
#   case                          f32 e_c   f32 e_f   needed   f64 e_c   f64 e_f   needed
#   message n1                    0.34      0.34      0.00     0.00      0.00      0.00
#   message kat                   0.30      0.30      0.00     0.00      0.00      0.00
#   message n70_1x1               0.48      0.71      0.00     0.77      0.00      0.00
#   message n70_3x5               0.58      0.69      0.00     0.62      0.00      0.00
#   message n70_4x64              0.92      0.77      0.00     0.79      0.00      0.00
#   message n70_2x64              0.83      0.83      0.00     1.10      0.00      0.00
#   message n70_64x64             0.77      0.89      0.00     1.29      0.00      0.00
#   message n70_1x65              0.94      0.83      0.00     0.88      0.00      0.00
#   message n70_4x256             0.80      0.80      0.00     1.05      0.00      0.00
#   message isolated              0.76      1.01      0.00     0.73      0.00      0.00
#   message hub_in                5.08      3.96      0.00     13.85     4.85      0.00
#   message hub_out               12.76     4.12      0.00     10.05     6.70      0.00
#   message hub_in_4x4            7.75      3.67      0.00     10.99     3.09      0.00
#   message hub_out_4x4           1.71      1.71      0.00     5.68      4.47      0.00
#   aggregate n1                  0.00      0.00      0.00     0.00      0.00      0.00
#   aggregate kat                 0.42      0.42      0.00     0.00      0.00      0.00
#   aggregate isolated            0.67      0.67      0.00     0.75      0.00      0.00
#   aggregate n70_m1              0.69      0.62      0.00     0.58      0.00      0.00
#   aggregate n70_m64             1.06      0.91      0.00     0.81      0.00      0.00
#   aggregate n70_m65             0.75      0.77      0.00     1.21      0.00      0.00
#   aggregate n70_m256            0.78      0.85      0.00     0.98      0.00      0.00
#   aggregate n70_m3_fff          0.61      0.52      0.00     0.97      0.00      0.00
#   aggregate n70_m3_fft          0.51      0.98      0.00     1.28      0.00      0.00
#   aggregate n70_m3_ftf          0.70      0.53      0.00     0.56      0.00      0.00
#   aggregate n70_m3_ftt          0.58      0.58      0.00     1.19      0.00      0.00
#   aggregate n70_m3_tff          0.55      0.55      0.00     0.56      0.00      0.00
#   aggregate n70_m3_tft          0.83      0.83      0.00     1.34      0.00      0.00
#   aggregate n70_m3_ttf          0.77      0.75      0.00     0.60      0.00      0.00
#   aggregate n70_m3_ttt          0.67      0.67      0.00     0.63      0.00      0.00
#   aggregate hub_in_m3_ttt       16.44     1.83      0.00     9.57      1.30      0.00
#   aggregate hub_in_m3_fff       6.58      1.26      0.00     5.28      3.52      0.00
#   aggregate hub_in_m64_ttt      9.70      2.24      0.00     13.56     9.86      0.00
#   aggregate hub_in_m64_fff      4.96      2.86      0.00     8.56      7.13      0.00
#   aggregate hub_out_m3_ttt      7.11      2.79      0.00     6.52      3.48      0.00
#   aggregate hub_out_m3_fff      0.26      0.26      0.00     0.00      0.00      0.00
#   aggregate hub_out_m64_ttt     7.24      2.24      0.00     9.25      11.09     0.00
#   aggregate hub_out_m64_fff     0.49      0.49      0.00     0.00      0.00      0.00
#   true-gradient n70             0.87      0.71      0.00     1.07      1.07      0.00
# One training step's parameter gradients (f32 against the composed run in f64, classes weighted 1 : 3), per parameter of the two layers
# (message transform, vertex transform: weight, bias of each Linear) and the head:
#   parameter  shape       e_c    e_f    needed
#   0          [33, 16]    1.46   1.34   0.00
#   1          [1, 16]     1.38   1.63   0.00
#   2          [16, 8]     1.56   1.54   0.00
#   3          [1, 8]      0.81   0.79   0.00
#   4          [24, 16]    1.15   0.69   0.00
#   5          [1, 16]     1.35   1.24   0.00
#   6          [16, 16]    1.74   1.25   0.00
#   7          [1, 16]     1.49   0.71   0.00
#   8          [33, 16]    1.47   1.11   0.00
#   9          [1, 16]     0.75   0.85   0.00
#   10         [16, 8]     1.51   1.01   0.00
#   11         [1, 8]      1.39   0.93   0.00
#   12         [24, 16]    0.79   1.10   0.00
#   13         [1, 16]     0.99   0.37   0.00
#   14         [16, 16]    1.29   1.11   0.00
#   15         [1, 16]     0.63   1.02   0.00
#   16         [16, 2]     1.79   1.20   0.00
#   17         [1, 2]      0.88   0.83   0.00
# No case needs anything.  In f64 a node that is not split has e_f = 0: its sums run in the order of the edge list, which is the
# restatement's own.  (The chain's e_c moves between runs - its atomics - e_f does not.)  The factors are bit for bit the restatement's
# because the kernel computes each f32 operation in f64 and rounds it: the f32 square root instruction is an ulp of f32 off ATen's in places,
# 1.6e8 eps of f64.
FLOOR_EPS = 0
MAX_COMPOSED_EPS = 64      # e_c above this means the chain is broken, and a broken chain must not loosen the rule
ALL_ON, ALL_OFF = (True, True, True), (False, False, False)


@functools.lru_cache(maxsize=None)
def _graph(name):
    """-> (N, edgeI, edgeJ)"""
    if name == "n1":                          # one node, one self loop
        return 1, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    if name == "kat":
        k = KATS["aggregate"]
        return k["numVertices"], torch.tensor(k["edgeI"]), torch.tensor(k["edgeJ"])
    if name in ("n70", "isolated"):
        i, j = _random_edges(70, 300, 5)
        if name == "isolated":                # node 5 occurs in no edge: both its factors are inf, and no edge reads them
            keep = (i != 5) & (j != 5)
            assert int((~keep).sum()) > 1
            i, j = i[keep], j[keep]
        return 70, i, j
    if name in ("hub_in", "hub_out"):
        # N = 2L + 4; every edge runs from a node >= 3 into node 0, 1 or 2, which have no outgoing edge, so the edges a kernel sums for
        # them are their incoming ones in whichever grouping.  Into node 0: nodes 3 .. 2L + 3 and nodes 3 and 4 a second time, 2L + 3 edges
        # (split, uneven shares); into node 1: nodes 3 .. L + 2, L edges (the longest row one wave takes); into node 2: nodes L + 2 ..
        # 2L + 2, L + 1 edges (the shortest split row).  hub_out is the same graph with every edge reversed.
        l = G.mpnnLongRow()
        n = 2 * l + 4
        pairs = [(k, 0) for k in range(3, 2 * l + 4)] + [(3, 0), (4, 0)] + [(k, 1) for k in range(3, l + 3)] + [(k, 2) for k in range(l + 2, 2 * l + 3)]
        order = torch.tensor([(p * 7919) % len(pairs) for p in range(len(pairs))])          # a fixed shuffle: 7919 is prime
        assert sorted(order.tolist()) == list(range(len(pairs)))
        src, dst = torch.tensor([p[0] for p in pairs])[order], torch.tensor([p[1] for p in pairs])[order]
        deg = torch.bincount(dst, minlength=n)
        assert deg[0] == 2 * l + 3 and deg[1] == l and deg[2] == l + 1 and int(torch.bincount(src, minlength=n)[:3].sum()) == 0
        return (n, src, dst) if name == "hub_in" else (n, dst, src)
    raise KeyError(name)


# message case -> (graph, Fe, D).  On the 70-node graph: scalar throughout (1, 1) and odd (3, 5); 16-byte packets throughout in f32
# (4, 64); column offsets that break 16-byte but not 8-byte alignment in f32 (2, 64); wide edge features (64, 64); past one wave's columns
# and unaligned (1, 65); more than one column tile (4, 256).  The small and the hub graphs with a scalar and a packet shape; the hubs' packet
# shape is narrow (4, 4): the chain's float atomics over 2L + 3 terms come to 50 eps at 64 columns (the maximum grows with the number of
# columns), too close to the 64 eps that tell a broken chain.
WIDTHS = ((1, 1), (3, 5), (4, 64), (2, 64), (64, 64), (1, 65), (4, 256))
MSG_CASES = {"n1": ("n1", 3, 5), "kat": ("kat", 3, 5)}
MSG_CASES.update({f"n70_{fe}x{d}": ("n70", fe, d) for fe, d in WIDTHS})
MSG_CASES.update({"isolated": ("isolated", 3, 5), "hub_in": ("hub_in", 3, 5), "hub_out": ("hub_out", 3, 5), "hub_in_4x4": ("hub_in", 4, 4),
                  "hub_out_4x4": ("hub_out", 4, 4)})
MSG_KEYS = ("msg", "dedge", "dx")
# aggregate case -> (graph, M, (degreeNormalizeI, degreeNormalizeJ, aggregateJ)): every width with everything on, every flag combination
# at M = 3, all on and all off on the hubs
FLAGS = [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)]
_fl = lambda f: "".join("ft"[int(v)] for v in f)
AGG_CASES = {"n1": ("n1", 3, ALL_ON), "kat": ("kat", 3, ALL_ON), "isolated": ("isolated", 3, ALL_ON)}
AGG_CASES.update({f"n70_m{m}": ("n70", m, ALL_ON) for m in (1, 64, 65, 256)})
AGG_CASES.update({f"n70_m3_{_fl(f)}": ("n70", 3, f) for f in FLAGS})
AGG_CASES.update({f"{h}_m{m}_{_fl(f)}": (h, m, f) for h in ("hub_in", "hub_out") for m in (3, 64) for f in (ALL_ON, ALL_OFF)})
AGG_KEYS = ("out", "dmsg")


@functools.lru_cache(maxsize=None)
def _message_problem(name, dt):
    """closed-form operands rounded to dt (as f64) and the restatement's result and gradients, computed once per case"""
    g, fe, d = MSG_CASES[name]
    n, ei, ej = _graph(g)
    rd = lambda t: t.to(dt).to(F64)
    x, ef, lf = rd(closed_form((n, d), 7, 4.0, F64)), rd(closed_form((ei.numel(), fe), 11, 2.0, F64)), rd(closed_form((ei.numel(), fe + 2 * d), 301, 1.0, F64))
    xr, er = x.clone().requires_grad_(True), ef.clone().requires_grad_(True)
    msg = R.message(xr, er, ei, ej)
    (msg * lf).sum().backward()
    return n, ei, ej, x, ef, lf, {"msg": msg.detach(), "dedge": er.grad.detach(), "dx": xr.grad.detach()}


def _message_library(name, dt, fused, csr=None, pitch=None, transposed=False):
    n, ei, ej, x, ef, lf, _ = _message_problem(name, dt)
    prev = G.mpnnFused(fused)
    try:
        ts = lambda t: to_sten(t.to(dt))
        if pitch is None:
            xv = A.param(ts(x))
        else:                                  # rows of x inside a wider buffer
            wide = torch.zeros(n, pitch, dtype=F64)
            wide[:, :x.shape[1]] = x
            xv = A.param(ts(wide).narrow(1, 0, x.shape[1]))
            assert xv.value.strides == [pitch, 1]
        if transposed:                         # an [Fe, E] buffer read as [E, Fe]
            ev = A.param(ts(ef.t().contiguous()).t)
            assert ev.value.strides == [1, ef.shape[0]]
        else:
            ev = A.param(ts(ef))
        msg = G.mpnnMessage(xv, ev, to_sten(ei), to_sten(ej), csr)
        (msg * A.const(ts(lf))).sum().backprop()
        return {"msg": to_torch(msg.value), "dedge": to_torch(ev.partialDerivative), "dx": to_torch(xv.partialDerivative)}
    finally:
        G.mpnnFused(prev)


@functools.lru_cache(maxsize=None)
def _aggregate_problem(name, dt):
    g, m, flags = AGG_CASES[name]
    n, ei, ej = _graph(g)
    rd = lambda t: t.to(dt).to(F64)
    msg, lf = rd(closed_form((ei.numel(), m), 13, 4.0, F64)), rd(closed_form((n, m), 301, 1.0, F64))
    mr = msg.clone().requires_grad_(True)
    out = R.aggregate(n, mr, ei, ej, *flags, dtype=dt)
    (out * lf).sum().backward()
    return n, ei, ej, msg, lf, flags, {"out": out.detach(), "dmsg": mr.grad.detach()}


def _aggregate_library(name, dt, fused, csr=None, cache=None):
    n, ei, ej, msg, lf, flags, _ = _aggregate_problem(name, dt)
    prev = G.mpnnFused(fused)
    try:
        ts = lambda t: to_sten(t.to(dt))
        mv = A.param(ts(msg))
        out = G.mpnnAggregate(n, mv, to_sten(ei), to_sten(ej), *flags, csr, cache)
        (out * A.const(ts(lf))).sum().backprop()
        return {"out": to_torch(out.value), "dmsg": to_torch(mv.partialDerivative)}
    finally:
        G.mpnnFused(prev)


def _err(got, ref):
    assert list(got.shape) == list(ref.shape), f"shape {list(got.shape)} vs {list(ref.shape)}"
    den = ref.abs().max().item()
    return (got.double() - ref).abs().max().item() / (den if den > 0 else 1.0)


def _rule(tag, name, dt, keys, ref, comp, fus):
    """e_f <= 4 * e_c + FLOOR_EPS * eps and e_c <= 64 eps for every key; the figures are printed (-s)"""
    bad = []
    for key in keys:
        e_c, e_f = _err(comp[key], ref[key]), _err(fus[key], ref[key])
        print(f"PARITY {tag} {name} {key} {dt}: e_c {e_c:.3e} ({e_c / EPS[dt]:.2f} eps) e_f {e_f:.3e} ({e_f / EPS[dt]:.2f} eps) needed {max(0.0, e_f - 4 * e_c) / EPS[dt]:.2f} eps")
        if not e_c <= MAX_COMPOSED_EPS * EPS[dt]:
            bad.append(f"{key}: composed error {e_c:.3e} > {MAX_COMPOSED_EPS} eps")
        if not e_f <= 4 * e_c + FLOOR_EPS * EPS[dt]:
            bad.append(f"{key}: fused error {e_f:.3e} > 4 * composed error {e_c:.3e} + {FLOOR_EPS} eps")
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(MSG_CASES))
def test_message_fused_and_composed_vs_restatement(gpu, name, dt):
    """msg, dedge and dx under the rule; msg and dedge are copies, so the fused node's equal the chain's and the restatement's bit for bit"""
    ref = _message_problem(name, dt)[-1]
    comp, fus = _message_library(name, dt, fused=False), _message_library(name, dt, fused=True)
    for key in ("msg", "dedge"):
        assert torch.equal(fus[key], comp[key]) and torch.equal(fus[key].double(), ref[key]), key
    _rule("message", name, dt, MSG_KEYS, ref, comp, fus)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(AGG_CASES))
def test_aggregate_fused_and_composed_vs_restatement(gpu, name, dt):
    """out and dmsg under the rule"""
    ref = _aggregate_problem(name, dt)[-1]
    comp, fus = _aggregate_library(name, dt, fused=False), _aggregate_library(name, dt, fused=True)
    _rule("aggregate", name, dt, AGG_KEYS, ref, comp, fus)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_isolated_node_gets_zeros_and_nothing_leaks_from_its_inf_factor(gpu, dt):
    """node 5 occurs in no edge: both its degree factors are inf (as in the reference), its rows of out and dx are zero, and every
    result is finite"""
    n, ei, ej = _graph("isolated")
    csr = G.computeEdgeCsr(to_sten(ei), to_sten(ej), n)
    for rowptr in (csr.inRowptr, csr.outRowptr):
        f = to_torch(G.mpnnDegreeFactor(rowptr, -0.5, TORCH2LAMP[dt]))
        assert torch.isinf(f[5]) and f[5] > 0 and int(torch.isinf(f).sum()) == 1
    agg, msg = _aggregate_library("isolated", dt, fused=True, csr=csr), _message_library("isolated", dt, fused=True, csr=csr)
    for res in (agg, msg):
        for key, t in res.items():
            assert bool(torch.isfinite(t).all()), key
    assert torch.equal(agg["out"][5], torch.zeros_like(agg["out"][5])) and torch.equal(msg["dx"][5], torch.zeros_like(msg["dx"][5]))


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_degree_factor_is_the_restatement_s_f32_value(gpu, dt):
    """both exponents, counts 0 .. 2L + 3 among them: the bits of torch's pow of an integer tensor (f32), cast to the type"""
    n, ei, ej = _graph("hub_in")
    csr = G.computeEdgeCsr(to_sten(ei), to_sten(ej), n)
    for p in (-0.5, -1.0):
        for rowptr, index in ((csr.inRowptr, ej), (csr.outRowptr, ei)):
            got = to_torch(G.mpnnDegreeFactor(rowptr, p, TORCH2LAMP[dt]))
            assert got.dtype == dt and torch.equal(got, R.degree_factor(index, n, p, dt)), p
    with pytest.raises(LampError, match="exponent"):
        G.mpnnDegreeFactor(csr.inRowptr, -2.0, S.F32)


@pytest.mark.parametrize("name", ["n70_3x5", "n70_4x64", "hub_in_4x4", "hub_out"])
def test_message_gradient_is_bitwise_reproducible(gpu, name):
    dt = torch.float32
    a, b = _message_library(name, dt, fused=True), _message_library(name, dt, fused=True)
    assert torch.equal(a["dx"], b["dx"])


@pytest.mark.parametrize("name", ["n70_m3_ttt", "n70_m65", "hub_in_m64_ttt", "hub_out_m3_ttt"])
def test_aggregate_is_bitwise_reproducible(gpu, name):
    dt = torch.float32
    a, b = _aggregate_library(name, dt, fused=True), _aggregate_library(name, dt, fused=True)
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["dmsg"], b["dmsg"])


@pytest.mark.parametrize("pitch", [68, 67])
def test_strided_inputs_give_the_bits_of_their_contiguous_copies(gpu, pitch):
    """edgeFeatures as the transpose of an [Fe, E] buffer and the rows of x inside a buffer of pitch 68 (16-byte packets still) or 67
    (scalar accesses)"""
    name, dt = "n70_4x64", torch.float32
    a = _message_library(name, dt, fused=True)
    b = _message_library(name, dt, fused=True, pitch=pitch, transposed=True)
    for key in MSG_KEYS:
        assert torch.equal(a[key], b[key]), key


def _linear(in_, out, dt, salt):
    """a Linear without bias with closed-form weights -> (module, the same map on f64 torch tensors)"""
    m = nn.Linear(in_, out, TORCH2LAMP[dt], 0, bias=False)
    shape = m.state[0].shape
    assert sorted(shape) == sorted([in_, out]) and in_ != out
    w = closed_form(tuple(shape), salt, 1.0, F64).to(dt)
    m.load([to_sten(w)])
    w = w.to(F64)
    return m, (lambda t: t @ w) if shape == [in_, out] else (lambda t: t @ w.t())


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_node_features_receive_the_true_gradient(gpu, dt):
    """MPNN.forward with nodeFeatures a parameter that another consumer (x * 2, summed into the loss) has already used: five consumers
    in all with the two gathers, the vertex transform's input and the residual.  dx must match the restatement under the rule, fused and
    composed alike; the reference's literal chain (IndexSelect straight on nodeFeatures) doubles what x already holds."""
    n, ei, ej = _graph("n70")
    d, fe, m = 5, 3, 4
    rd = lambda t: t.to(dt).to(F64)
    x, ef, lf = rd(closed_form((n, d), 7, 2.0, F64)), rd(closed_form((ei.numel(), fe), 11, 2.0, F64)), rd(closed_form((n, d), 301, 1.0, F64))
    res = {}
    for fused in (False, True):
        mt, mt_ref = _linear(fe + 2 * d, m, dt, 21)
        vt, vt_ref = _linear(d + m, d, dt, 23)
        layer = G.MPNN(mt, vt)
        ts = lambda t: to_sten(t.to(dt))
        xv = A.param(ts(x))
        prev = G.mpnnFused(fused)
        try:
            prior = (xv * 2.0).sum()
            out = layer.forward(G.Graph(xv, A.const(ts(ef)), to_sten(ei), to_sten(ej), None)).nodeFeatures
            ((out * A.const(ts(lf))).sum() + prior).backprop()
        finally:
            G.mpnnFused(prev)
        res[fused] = {"out": to_torch(out.value), "dx": to_torch(xv.partialDerivative)}
    xr = x.clone().requires_grad_(True)
    agg = R.aggregate(n, mt_ref(R.message(xr, ef, ei, ej)), ei, ej, True, True, True, dtype=dt)
    out = xr + vt_ref(torch.cat([xr, agg], 1))
    ((out * lf).sum() + (xr * 2.0).sum()).backward()
    _rule("true-gradient", "n70", dt, ("out", "dx"), {"out": out.detach(), "dx": xr.grad.detach()}, res[False], res[True])


def test_launch_budget(gpu):
    """prebuilt CSR and factors: mpnnMessage runs one kernel forward and two backward, mpnnAggregate one and one, no other mpnn_ kernel and
    no index_add; with mpnnFused(False) no such kernel runs and index_add does - a fused path that fell back would show here"""
    dt = torch.float32
    n, ei, ej = _graph("n70")
    csr, cache = G.computeEdgeCsr(to_sten(ei), to_sten(ej), n), {}
    _aggregate_library("n70_m64", dt, fused=True, csr=csr, cache=cache)          # fills the factor cache
    mpnn = lambda counts: {k: v for k, v in counts.items() if k.startswith("mpnn_")}
    fused = _timer_counts(lambda: _message_library("n70_4x64", dt, fused=True, csr=csr))
    assert mpnn(fused) == {"mpnn_message": 1, "mpnn_message_backward_x": 1, "mpnn_message_backward_edge": 1}, fused
    assert "index_add" not in fused and "graph_edge_rowptr" not in fused, fused
    fused = _timer_counts(lambda: _aggregate_library("n70_m64", dt, fused=True, csr=csr, cache=cache))
    assert mpnn(fused) == {"mpnn_aggregate": 1, "mpnn_aggregate_backward": 1}, fused
    assert "index_add" not in fused and "graph_edge_rowptr" not in fused, fused
    for run in (lambda: _message_library("n70_4x64", dt, fused=False, csr=csr), lambda: _aggregate_library("n70_m64", dt, fused=False, csr=csr, cache=cache)):
        composed = _timer_counts(run)
        assert not mpnn(composed) and composed.get("index_add", 0) >= 1, composed


def test_message_backward_skips_the_gradient_nobody_needs(gpu):
    """constant edge features: one backward launch; constant node features: the other one"""
    n, ei, ej, x, ef, lf, _ = _message_problem("n70_4x64", torch.float32)
    csr = G.computeEdgeCsr(to_sten(ei), to_sten(ej), n)
    for xw, ew, want in ((A.param, A.const, "mpnn_message_backward_x"), (A.const, A.param, "mpnn_message_backward_edge")):
        def run():
            msg = G.mpnnMessage(xw(to_sten(x.float())), ew(to_sten(ef.float())), to_sten(ei), to_sten(ej), csr)
            (msg * A.const(to_sten(lf.float()))).sum().backprop()
        counts = _timer_counts(run)
        assert {k: v for k, v in counts.items() if k.startswith("mpnn_message_backward")} == {want: 1}, counts


def _mlp(in_, out, hidden, dropout=0.0):
    return nn.MLP(in_, out, [hidden], S.F32, 0, dropout=dropout, norm="NoNorm")


def test_graph_caches_the_degree_factors(gpu):
    """two stacked layers over one graph: the two groupings are built once, each of the two factor vectors (sources, destinations) by one
    mpnn_degree_factor launch, and the layers run one mpnn_message and one mpnn_aggregate each"""
    x, i, j = _planted_graph()[:3]
    graph = G.Graph(A.const(to_sten(x)), A.const(to_sten(torch.ones(i.numel(), 1))), to_sten(i), to_sten(j), None)
    layers = [G.MPNN(_mlp(1 + 32, 8, 16), _mlp(16 + 8, 16, 16)) for _ in range(2)]

    def run():
        g = graph
        for layer in layers:
            g = layer.forward(g)
        return g
    counts = _timer_counts(run)
    assert counts.get("mpnn_degree_factor", 0) == 2 and counts.get("graph_edge_rowptr", 0) == 2, counts
    assert counts.get("mpnn_message", 0) == 2 and counts.get("mpnn_aggregate", 0) == 2, counts
    assert run().nodeFeatures.shape == [x.shape[0], 16]
    other = _timer_counts(lambda: G.MPNN(_mlp(1 + 32, 8, 16), _mlp(16 + 8, 16, 16), degreeNormalizeJ=False).forward(graph))
    assert other.get("mpnn_degree_factor", 0) == 1 and "graph_edge_rowptr" not in other, other        # p = -1: another key


def test_bad_arguments_are_errors(gpu):
    """LampError, and nothing dereferenced: an endpoint outside [0, N) is found by the range reduction of the grouping, before any kernel
    uses an endpoint as an index"""
    x, ef = A.const(to_sten(torch.zeros(4, 2))), A.const(to_sten(torch.zeros(3, 1)))
    i3, j3 = to_sten(torch.tensor([0, 1, 2])), to_sten(torch.tensor([1, 2, 3]))
    for bad in (to_sten(torch.tensor([0, 4, 2])), to_sten(torch.tensor([0, -1, 2]))):
        with pytest.raises(LampError, match="edge endpoints must lie in"):
            G.mpnnMessage(x, ef, bad, j3)
        with pytest.raises(LampError, match="edge endpoints must lie in"):
            G.mpnnAggregate(4, A.const(to_sten(torch.zeros(3, 2))), i3, bad, True, True, True)
    with pytest.raises(LampError, match="one row per edge"):
        G.mpnnMessage(x, A.const(to_sten(torch.zeros(2, 1))), i3, j3)
    with pytest.raises(LampError, match="differ in type"):
        G.mpnnMessage(x, A.const(to_sten(torch.zeros(3, 1, dtype=F64))), i3, j3)
    with pytest.raises(LampError, match="a row per edge"):
        G.mpnnAggregate(4, A.const(to_sten(torch.zeros(2, 2))), i3, j3, True, True, True)
    csr = G.computeEdgeCsr(i3, j3, 4)
    with pytest.raises(LampError, match="not of message's type"):
        A.apply_op("MpnnAggregate", [A.const(to_sten(torch.zeros(3, 2)))], tensors=csr.tensors + [G.mpnnDegreeFactor(csr.outRowptr, -1.0, S.F64)], i=[1, 1, 0])
    with pytest.raises(AssertionError, match="belongs to a graph of 4 nodes"):
        G.mpnnMessage(A.const(to_sten(torch.zeros(5, 2))), ef, i3, j3, csr)
    with pytest.raises(AssertionError, match="was built from 3 edges"):
        G.mpnnAggregate(4, A.const(to_sten(torch.zeros(2, 2))), to_sten(torch.tensor([0, 1])), to_sten(torch.tensor([1, 2])), True, True, True, csr)
    with pytest.raises(LampError, match="nodeFeatures has"):
        A.apply_op("MpnnMessage", [A.const(to_sten(torch.zeros(5, 2))), ef], tensors=csr.tensors)


@pytest.mark.parametrize("device", [0, S.CPU], ids=["gpu", "cpu"])
def test_reference_kats(gpu, device):
    """mpnn.test.scala in f64, fused and composed, on the GPU and on lamp's CPU device (host tensors are staged through the GPU): the
    count-occurrences vector, six aggregate cases exactly and the seventh to the reference's 4 decimals"""
    k = KATS["countOccurences"]
    counts = G.countOccurences(to_sten(torch.tensor(k["t"]), device=device), k["elems"])
    assert counts.device == device and to_torch(counts).tolist() == k["expected"]
    k = KATS["aggregate"]
    ei, ej = to_sten(torch.tensor(k["edgeI"]), device=device), to_sten(torch.tensor(k["edgeJ"]), device=device)
    for fused in (True, False):
        prev = G.mpnnFused(fused)
        try:
            for case in k["cases"]:
                msg = A.const(to_sten(torch.tensor(k["message"], dtype=F64), device=device))
                out = G.mpnnAggregate(k["numVertices"], msg, ei, ej, case["degreeNormalizeI"], case["degreeNormalizeJ"], case["aggregateJ"])
                assert out.value.device == device
                got = to_torch(out.value)
                if case["roundTo"] is not None:
                    got = torch.round(got * 10 ** case["roundTo"]) / 10 ** case["roundTo"]
                assert got.tolist() == case["expected"], (fused, case)
        finally:
            G.mpnnFused(prev)


def test_module_state_load_and_training_mode(gpu):
    """state is the message transform's followed by the vertex transform's, load splits by the two lengths, asEval / asTraining reach both
    transforms (dropout in one of them at a time), edgeFeatures = None is an assertion error, the residual needs equal widths"""
    x, i, j = _planted_graph()[:3]
    n, si, sj = x.shape[0], to_sten(i), to_sten(j)
    edges = A.const(to_sten(torch.ones(i.numel(), 1)))
    graph = G.Graph(A.const(to_sten(x)), edges, si, sj, None)
    mt, vt = _mlp(1 + 32, 8, 16), _mlp(16 + 8, 16, 16)
    layer = G.MPNN(mt, vt, degreeNormalizeI=False)
    assert (layer.degreeNormalizeI, layer.degreeNormalizeJ, layer.aggregateJ) == (False, True, True)
    k, m = len(mt.state), len(vt.state)
    assert k > 0 and m > 0 and [v.shape for v in layer.state] == [v.shape for v in mt.state] + [v.shape for v in vt.state]
    assert len(layer.parameters) == len(mt.parameters) + len(vt.parameters)
    layer.load([S.STen.ones(v.shape, S.F32, 0) * float(q + 1) for q, v in enumerate(layer.state)])
    for q, v in enumerate(list(mt.state) + list(vt.state)):
        assert bool((to_torch(v.value) == q + 1).all()), q
    with pytest.raises(AssertionError):
        layer.load([S.STen.ones(v.shape, S.F32, 0) for v in mt.state])
    with pytest.raises(AssertionError):
        layer.forward(G.Graph(A.const(to_sten(x)), None, si, sj, None))
    # the residual: widths 16 -> 16 add the input, 16 -> 12 cannot
    lib.lamp_manual_seed(3)
    same, other = G.MPNN(_mlp(33, 8, 16), _mlp(24, 16, 16)), G.MPNN(_mlp(33, 8, 16), _mlp(24, 12, 16))
    assert same.forward(graph).nodeFeatures.shape == [n, 16] and other.forward(graph).nodeFeatures.shape == [n, 12]
    for v in same.vertexTransform.state:                        # a vertex transform that returns zeros leaves the residual alone
        v.value.copyFrom(S.STen.zeros(v.shape, S.F32, 0))
    assert torch.equal(to_torch(same.forward(graph).nodeFeatures.value), x)
    # training mode: dropout in the message transform alone, then in the vertex transform alone
    for dm, dv in ((0.5, 0.0), (0.0, 0.5)):
        lib.lamp_manual_seed(5)
        drop = G.MPNN(_mlp(33, 8, 16, dm), _mlp(24, 16, 16, dv))
        run = lambda: to_torch(drop.forward(graph).nodeFeatures.value)
        assert drop.asEval() is drop and torch.equal(run(), run())
        assert drop.asTraining() is drop and not torch.equal(run(), run())
    drop.zeroGrad()


def _train(messages, fused=True, steps=30, dtype=torch.float32, class_weights=(1.0, 1.0)):
    """two MPNN layers (MLP transforms with one hidden layer, residual) + Linear + logSoftMax on _planted_graph with unit edge features.
    messages = False: the aggregated messages are replaced by zeros, so every node sees its own features alone."""
    x, i, j, label, train, held = _planted_graph()
    n, dt = x.shape[0], TORCH2LAMP[dtype]
    lib.lamp_manual_seed(7)
    layers = [G.MPNN(nn.MLP(1 + 32, 8, [16], S.F32, 0, norm="NoNorm"), nn.MLP(16 + 8, 16, [16], S.F32, 0, norm="NoNorm")) for _ in range(2)]
    head = nn.Linear(16, 2, S.F32, 0)
    if dt != S.F32:                           # the same initial weights in another type
        wide = [G.MPNN(nn.MLP(1 + 32, 8, [16], dt, 0, norm="NoNorm"), nn.MLP(16 + 8, 16, [16], dt, 0, norm="NoNorm")) for _ in range(2)] + [nn.Linear(16, 2, dt, 0)]
        for w, m in zip(wide, layers + [head]):
            w.load([v.value.castToType(dt) for v in m.state])
        layers, head = wide[:2], wide[2]
    params = [p for m in layers + [head] for p in m.parameters]
    opt = nn.AdamW([p.value for p in params], 0.0, 0.01)
    graph = G.Graph(A.const(to_sten(x.to(dtype))), A.const(to_sten(torch.ones(i.numel(), 1, dtype=dtype))), to_sten(i), to_sten(j), None)
    weights, target, rows = to_sten(torch.tensor(class_weights, dtype=dtype)), to_sten(label[train]), A.const(to_sten(train))
    nothing = A.const(S.STen.zeros([n, 8], dt, 0))

    def silent(layer, g):
        updated = layer.vertexTransform.forward(A.apply_op("Concatenate", [g.nodeFeatures, nothing], i=[1]))
        return g.copy(nodeFeatures=g.nodeFeatures + updated)

    def logits():
        g = graph
        for layer in layers:
            g = layer.forward(g) if messages else silent(layer, g)
        return head.forward(g.nodeFeatures).logSoftMax(1)

    prev = G.mpnnFused(fused)
    try:
        losses, grads = [], None
        for _ in range(steps):
            for m in layers + [head]:
                m.zeroGrad()
            loss = logits().indexSelect(0, rows).nllLoss(target, weights)
            loss.backprop()
            if grads is None:
                grads = [to_torch(p.partialDerivative).double() for p in params]
            opt.step([p.partialDerivative for p in params])
            losses.append(loss.value.item())
    finally:
        G.mpnnFused(prev)
    return losses, grads


def test_one_step_s_parameter_gradients_agree_between_fused_and_composed(gpu):
    """the first training step of the two-layer network: every parameter gradient of the fused and of the composed f32 run against the
    composed run in f64 from the same weights (whose own error is of the order of f64's eps, nothing beside f32's), under the whole rule
    per parameter: e_c <= 64 eps and e_f <= 4 * e_c + FLOOR_EPS * eps.  The figures are in the header's table.  The classes are weighted
    1 : 3 here.  With equal weights, balanced labels and initial probabilities near 1/2 the sum over the training nodes of (p - y), which is
    the head's bias gradient and a factor of the last vertex transform's, cancels to a small part of its terms; an error measured against
    such a gradient's own maximum measures that cancellation (25 eps fused against 7 - 17 eps composed, from run to run, on the head's
    bias), not the nodes under test.  Unequal weights leave every parameter's gradient of the size of its terms."""
    ref = _train(True, fused=False, steps=1, dtype=F64, class_weights=(1.0, 3.0))[1]
    comp = _train(True, fused=False, steps=1, class_weights=(1.0, 3.0))[1]
    fus = _train(True, fused=True, steps=1, class_weights=(1.0, 3.0))[1]
    assert len(ref) == len(comp) == len(fus) > 0
    eps = EPS[torch.float32]
    for q, (r, c, f) in enumerate(zip(ref, comp, fus)):
        e_c, e_f = _err(c, r), _err(f, r)
        print(f"PARITY step gradient {q} {list(r.shape)}: e_c {e_c / eps:.2f} eps e_f {e_f / eps:.2f} eps needed {max(0.0, e_f - 4 * e_c) / eps:.2f} eps")
        assert e_c <= MAX_COMPOSED_EPS * eps, f"parameter {q}: composed error {e_c / eps:.2f} eps > {MAX_COMPOSED_EPS} eps"
        assert e_f <= 4 * e_c + FLOOR_EPS * eps, f"parameter {q}: fused error {e_f / eps:.2f} eps > 4 * composed error {e_c / eps:.2f} eps + {FLOOR_EPS} eps"


def test_two_layer_mpnn_learns_and_beats_no_messages(gpu):
    """NLL on a tenth of the nodes, AdamW, 30 steps in f32 (the step count of test_two_layer_gcn_learns_and_beats_no_aggregation): the
    losses are finite and fall, and the run ends with a lower loss than the same network, from the same seed, with the aggregated
    messages zeroed"""
    losses = _train(True)[0]
    losses_silent = _train(False)[0]
    print(f"loss {losses[0]:.4f} -> {losses[-1]:.4f}; with the messages zeroed {losses_silent[0]:.4f} -> {losses_silent[-1]:.4f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert losses[-1] < losses_silent[-1], f"final loss {losses[-1]:.4f} with messages, {losses_silent[-1]:.4f} without"
