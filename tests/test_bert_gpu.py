"""lamp.nn.bert on the GPU, everything through lamp_amd.bert: the fused BertEmbedding node and the composed chain against the f64
restatement (tests/bert_ref.py), forward bit for bit and backward under the project's rule, bf16 against a derived bound, bitwise
repeatability, the launch budget, NULL outputs, the error paths, the modules at f64 against the restatement over the oracle's transformer
blocks, a checkpoint round trip, and one short training loop on batches from the batch builder."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from lamp_amd import autograd as A, bert as B, data as D, nn, sten as S
from lamp_amd._capi import LampError
from tests import bert_ref as R
from tests.test_graph_gpu import _timer_counts
from tests.test_transformer import _oracle_encoder_block, _rand_params
from tests.util import closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu
F64 = torch.float64
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
# The rule of tests/test_mpnn_gpu.py: e_f <= 4 * e_c + floor * eps with e_c <= 64 eps.  e_c / e_f are the max-abs errors of the composed
# chain and of the fused node against the f64 restatement over the restatement's max magnitude, for dToken, dSegment and dPositional
# through a fixed linear functional on closed-form operands rounded to the type.  The restatement writes its sums out in ascending order
# (bert_ref.embedding_gradients), which is the fused node's order for dPositional and for every table row of at most bertLongRow()
# occurrences: such a row is one ascending sum in acc_t rounded once, it carries no rounding the chain's sum does not, and its floor is 0
# (in f64 it has the restatement's bits: e_f = 0).  A row of n > bertLongRow() = L occurrences is the sum, in chunk order, of ceil(n / L)
# partial sums of at most L terms: at most L - 1 + ceil(n / L) - 1 additions stand behind any term, so it is off the exact sum by at most
# (L + ceil(n / L) - 2) u * sum|addends| with u = eps / 2, whatever the chain does.  The restatement is an f64 sum of n terms, n - 1
# additions: in f64 that is as many roundings of the same size again and the two differ by at most (L + ceil(n / L) - 2 + n - 1) u *
# sum|addends|; in f32 the restatement's roundings are 2^-29 of the type's and are not charged.  That is the floor of a case with long
# rows, over the restatement's max magnitude and maximised over the long rows and the columns (`_floor`, computed from the operands); the
# chain's serial f64 sum of a table row has the restatement's bits (e_c = 0), so in f64 the floor is all a long row has.
# Measured on an MI355X, max over the three gradients, in multiples of the type's eps ("needed" = (e_f - 4 e_c) / eps where positive):
#   case                         f32 e_c    f32 e_f    floor      needed     f64 e_c    f64 e_f    floor      needed
#   embedding d1                 0.70       0.45       0          0.00       0.00       0.00       0          0.00
#   embedding d3                 0.40       0.40       0          0.00       0.00       0.00       0          0.00
#   embedding d4                 0.79       0.79       0          0.00       0.34       0.00       0          0.00
#   embedding d8                 0.89       0.89       0          0.00       0.54       0.00       0          0.00
#   embedding d255               1.02       1.02       0          0.00       0.00       0.00       0          0.00
#   embedding d256               0.79       0.79       0          0.00       0.00       0.00       0          0.00
#   embedding d257               0.87       0.87       0          0.00       0.00       0.00       0          0.00
#   embedding d260               0.64       0.64       0          0.00       0.00       0.00       0          0.00
#   embedding b1t1               0.00       0.00       0          0.00       0.00       0.00       0          0.00
#   embedding b1t5_vs5           0.00       0.00       0          0.00       0.00       0.00       0          0.00
#   embedding b3t7_full          0.47       0.40       0          0.00       0.54       0.00       0          0.00
#   embedding b64t20             4.65       4.41       1220       0.00       4.64       2.32       7171       2.32
#   embedding b64t20_vs1         0.90       2.30       0          0.00       1.61       0.00       0          0.00
#   embedding distinct_v70000    0.79       0.79       0          0.00       0.34       0.00       0          0.00
#   embedding spread_v70000      4.65       3.29       2099       0.00       4.64       3.00       6314       3.00
#   embedding hub_1280x8         10.57      6.95       13150      0.00       4.64       26.57      136816     26.57
#   embedding hub_1280x4         18.19      6.90       13373      0.00       4.64       9.72       139143     9.72
#   embedding hub_4200x3         16.55      9.94       22545      0.00       5.10       55.22      528263     55.22
#   embedding long_d5            4.81       5.79       4113       0.00       1.68       3.62       24176      3.62
#   embedding long_d8            4.65       3.29       2099       0.00       4.64       3.00       6314       3.00
#   embedding wild               0.50       0.50       0          0.00       0.34       0.00       0          0.00
#   bert-loss, 1 block (22 tensors)                                          11.38      11.38      0          0.00
#   bert-loss, 2 blocks (32 tensors)                                         23.14      23.14      0          0.00
# In f32 no case needs its floor.  In f64 only the long rows need anything, at most 55 eps (dSegment of hub_4200x3) where that tensor's
# bound allows 353464: the bound is a worst case over n = 4200 addends of one sign pattern, the operands are not.  What it cannot see,
# test_long_rows_have_the_bits_of_the_chunked_sum does: there the restatement adds in the kernels' order and the fused gradients must have
# its bits, in f32 and in f64.  (The chain's f64 e_c is not 0 everywhere: its dPositional comes from a tree reduction.)  The module
# figures are equal because the two forms differ in the embedding's gradients alone, and those agree to the last bit at these sizes.
# The training loop carries no figure: its 32 losses and 31 final parameters are equal bit for bit between the two forms (mean loss over
# the corpus 5.2567 before, 4.4723 after 30 steps, in both).
MAX_COMPOSED_EPS = 64      # e_c above this means the chain is broken, and a broken chain must not loosen the rule
KEYS = ("dToken", "dSegment", "dPositional")


def _long():
    return B.bertLongRow()


# case -> (B, T, L, D, V, Vs, pattern).  D: scalar (1, 3), one packet in f32 (4), packets in every type (8), scalar just under a column
# tile (255), a full tile of scalars / 64 packets of four (256), scalar past it (257), 65 packets of four: a second column tile of one
# packet (260).  (B, T): one position, one row, a few rows, and 1280 positions, where the segment rows are long.  T = L and T < L.
CASES = {f"d{d}": (3, 7, 9, d, 11, 2, "mod") for d in (1, 3, 4, 8, 255, 256, 257, 260)}
CASES.update({
    "b1t1": (1, 1, 1, 4, 2, 1, "mod"),
    "b1t5_vs5": (1, 5, 8, 3, 11, 5, "mod"),
    "b3t7_full": (3, 7, 7, 8, 11, 5, "mod"),
    "b64t20": (64, 20, 20, 8, 11, 2, "mod"),
    "b64t20_vs1": (64, 20, 24, 3, 11, 1, "mod"),
    "distinct_v70000": (3, 7, 7, 4, 70000, 2, "distinct"),
    "spread_v70000": (64, 20, 24, 8, 70000, 5, "spread"),
    "hub_1280x8": (64, 20, 20, 8, 11, 2, "hub"),
    "hub_1280x4": (64, 20, 20, 4, 11, 2, "hub"),
    "hub_4200x3": (210, 20, 20, 3, 11, 2, "hub"),
    "long_d5": (64, 20, 20, 5, 700, 2, "long"),
    "long_d8": (64, 20, 24, 8, 700, 5, "long"),
    "wild": (3, 7, 7, 4, 11, 2, "wild"),
})


@functools.lru_cache(maxsize=None)
def _ids(name):
    b, t, l, d, v, vs, pattern = CASES[name]
    n = b * t
    idx = torch.arange(n)
    segments = (idx * 5 + idx // t) % vs
    if pattern == "mod":                       # token 0 present, every token several times where n > v
        tokens = (idx * 7 + 3) % v
    elif pattern == "distinct":                # all distinct, 0 absent, most tokens never occur
        tokens = 1 + idx * 3
    elif pattern == "spread":                  # 70000 rows (the prefix sum walks shares of 69 groups), token 0 at position 0
        tokens = (idx * 7919) % v
    elif pattern == "hub":                     # all equal
        tokens = torch.full((n,), 5)
    elif pattern == "long":                    # counts L - 1, L, L + 1, 2 L + 1 of tokens 1 .. 4, ten of token 0, token 5 never, the rest distinct
        lr = _long()
        counts = [lr - 1, lr, lr + 1, 2 * lr + 1]
        body = [k + 1 for k, c in enumerate(counts) for _ in range(c)] + [0] * 10
        body += list(range(6, 6 + n - len(body)))
        assert len(body) == n and max(body) < v
        order = torch.tensor([(p * 7919) % n for p in range(n)])               # a fixed shuffle: 7919 is prime and does not divide n
        assert sorted(order.tolist()) == list(range(n))
        tokens = torch.tensor(body)[order]
        assert torch.bincount(tokens, minlength=6)[:6].tolist() == [10] + counts + [0]
    elif pattern == "wild":                    # >= V, < -V (zero rows, no gradient), -1 (reads row V - 1, no gradient: the chain's backward does not wrap)
        tokens = (idx * 7 + 3) % v
        tokens[1], tokens[9], tokens[17] = v, -v - 1, -1
        segments[2], segments[8] = vs, -vs - 3
    else:
        raise KeyError(pattern)
    return tokens.view(b, t), segments.view(b, t)


@functools.lru_cache(maxsize=None)
def _problem(name, dt):
    """closed-form operands rounded to dt (as f64), the restatement's output in the type and its gradients in f64, once per case"""
    b, t, l, d, v, vs, _ = CASES[name]
    tokens, segments = _ids(name)
    rd = lambda x: x.to(dt).to(F64)
    tw, sw, pe = rd(closed_form((v, d), 7, 4.0, F64)), rd(closed_form((vs, d), 11, 2.0, F64)), rd(closed_form((1, l, d), 13, 2.0, F64))
    lf = rd(closed_form((b, t, d), 301, 1.0, F64))
    with torch.no_grad():
        out = R.embedding_with_any_index(tokens, segments, tw.to(dt), sw.to(dt), pe.to(dt))          # in the type: the chain's two roundings
    assert out.dtype == dt
    g = R.embedding_gradients(lf, tokens, segments, v, vs, l)
    return tokens, segments, tw, sw, pe, lf, {"out": out, "dToken": g[0], "dSegment": g[1], "dPositional": g[2]}


def _library(name, dt, fused):
    tokens, segments, tw, sw, pe, lf, _ = _problem(name, dt)
    prev = B.bertFused(fused)
    try:
        ts = lambda x: to_sten(x.to(dt))
        twv, swv, pev = A.param(ts(tw)), A.param(ts(sw)), A.param(ts(pe))
        out = B.bertEmbedding(A.const(to_sten(tokens)), A.const(to_sten(segments)), twv, swv, pev)
        (out * A.const(ts(lf))).sum().backprop()
        return {"out": to_torch(out.value), "dToken": to_torch(twv.partialDerivative), "dSegment": to_torch(swv.partialDerivative),
                "dPositional": to_torch(pev.partialDerivative)}
    finally:
        B.bertFused(prev)


def _err(got, ref):
    assert list(got.shape) == list(ref.shape), f"shape {list(got.shape)} vs {list(ref.shape)}"
    den = ref.abs().max().item()
    return (got.double() - ref).abs().max().item() / (den if den > 0 else 1.0)


def _occurrences(idx, rows):
    """how often each of 0 .. rows - 1 counts in the gradient: ids inside (0, rows)"""
    flat = idx.reshape(-1)
    return torch.bincount(flat[(flat > 0) & (flat < rows)], minlength=rows)


def _floor(name, dt, key):
    """the floor of the header, in eps: 0 unless the table has a row of more than bertLongRow() occurrences"""
    tokens, segments, _, _, _, lf, ref = _problem(name, dt)
    if key == "dPositional":
        return 0.0
    idx = (tokens if key == "dToken" else segments).reshape(-1)
    rows = ref[key].shape[0]
    counts = _occurrences(idx, rows)
    lr, worst = _long(), 0.0
    keep = (idx > 0) & (idx < rows)
    mass = torch.zeros(rows, lf.shape[-1], dtype=F64).index_add_(0, idx[keep], lf.reshape(-1, lf.shape[-1])[keep].abs())
    for r in torch.nonzero(counts > lr).view(-1).tolist():
        n = int(counts[r])
        additions = lr + math.ceil(n / lr) - 2 + (n - 1 if dt == F64 else 0)       # the restatement's own n - 1 count only in its own type
        worst = max(worst, additions / 2.0 * mass[r].max().item())
    den = ref[key].abs().max().item()
    return worst / (den if den > 0 else 1.0)


def _rule(tag, name, dt, keys, ref, comp, fus, floor=lambda key: 0.0):
    """e_f <= 4 * e_c + floor * eps and e_c <= 64 eps for every key; the figures are printed (-s)"""
    bad = []
    for key in keys:
        e_c, e_f, fl = _err(comp[key], ref[key]), _err(fus[key], ref[key]), floor(key)
        print(f"PARITY {tag} {name} {key} {dt}: e_c {e_c:.3e} ({e_c / EPS[dt]:.2f} eps) e_f {e_f:.3e} ({e_f / EPS[dt]:.2f} eps) floor {fl:.1f} eps "
              f"needed {max(0.0, e_f - 4 * e_c) / EPS[dt]:.2f} eps")
        if not e_c <= MAX_COMPOSED_EPS * EPS[dt]:
            bad.append(f"{key}: composed error {e_c:.3e} > {MAX_COMPOSED_EPS} eps")
        if not e_f <= 4 * e_c + fl * EPS[dt]:
            bad.append(f"{key}: fused error {e_f:.3e} > 4 * composed error {e_c:.3e} + {fl:.1f} eps")
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(CASES))
def test_fused_and_composed_vs_restatement(gpu, name, dt):
    """the output bit for bit (fused = composed = the restatement in the type), the three gradients under the rule, rows of at most two
    addends bit for bit"""
    tokens, segments, _, _, _, _, ref = _problem(name, dt)
    comp, fus = _library(name, dt, fused=False), _library(name, dt, fused=True)
    assert fus["out"].dtype == dt and torch.equal(fus["out"], comp["out"]) and torch.equal(fus["out"], ref["out"])
    _rule("embedding", name, dt, KEYS, ref, comp, fus, floor=lambda key: _floor(name, dt, key))
    for key, idx in (("dToken", tokens), ("dSegment", segments)):
        few = _occurrences(idx, ref[key].shape[0]) <= 2
        assert torch.equal(fus[key][few], comp[key][few]), key
    if tokens.shape[0] <= 2:
        assert torch.equal(fus["dPositional"], comp["dPositional"])
    # what the kernel writes without being asked to add: row 0, the rows that never occur, the positions past the sequence
    assert not fus["dToken"][0].any() and not fus["dSegment"][0].any() and not fus["dPositional"][0, tokens.shape[1]:].any()
    never = _occurrences(tokens, ref["dToken"].shape[0]) == 0
    assert not fus["dToken"][never].any()


LONG_CASES = ("b64t20", "spread_v70000", "hub_1280x8", "hub_1280x4", "hub_4200x3", "long_d5", "long_d8")


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", LONG_CASES)
def test_long_rows_have_the_bits_of_the_chunked_sum(gpu, name, dt):
    """counts of L - 1, L, L + 1, 2 L + 1 and the hubs: a row of more than L = bertLongRow() occurrences is the sum, in chunk order, of the
    ascending sums of its chunks of L positions, every other row one ascending sum; the restatement adds in that order in the type"""
    b, t, l, d, v, vs, _ = CASES[name]
    tokens, segments, _, _, _, lf, _ = _problem(name, dt)
    want = R.embedding_gradients(lf.to(dt), tokens, segments, v, vs, l, longRow=_long())
    counts = torch.cat([_occurrences(tokens, v), _occurrences(segments, vs)])
    assert int((counts > _long()).sum()) >= 1
    fus = _library(name, dt, fused=True)
    for key, w in zip(KEYS, want):
        assert torch.equal(fus[key], w), key


BF16_CASES = ("d1", "d3", "d8", "d255", "d256", "d260", "b1t1", "b64t20", "spread_v70000", "hub_1280x8", "long_d5", "long_d8", "wild")


@pytest.mark.parametrize("name", BF16_CASES)
def test_bf16_forward_bits_and_backward_bound(gpu, name):
    """forward: ((tok.float() + seg.float()) + pos.float()).bfloat16() bit for bit; backward: one bf16 rounding of an f32 sum of n terms,
    |err| <= 2^-8 |ref| + n 2^-23 sum|addends| per element against the f64 restatement"""
    dt = torch.bfloat16
    b, t, l, d, v, vs, _ = CASES[name]
    tokens, segments = _ids(name)
    rd = lambda x: x.to(dt)
    tw, sw, pe = rd(closed_form((v, d), 7, 4.0, F64)), rd(closed_form((vs, d), 11, 2.0, F64)), rd(closed_form((1, l, d), 13, 2.0, F64))
    lf = rd(closed_form((b, t, d), 301, 1.0, F64))
    with torch.no_grad():
        want = R.embedding_with_any_index(tokens, segments, tw.float(), sw.float(), pe.float()).bfloat16()
    prev = B.bertFused(True)
    try:
        twv, swv, pev = A.param(to_sten(tw)), A.param(to_sten(sw)), A.param(to_sten(pe))
        out = B.bertEmbedding(A.const(to_sten(tokens)), A.const(to_sten(segments)), twv, swv, pev)
        (out * A.const(to_sten(lf))).sum().backprop()
    finally:
        B.bertFused(prev)
    assert out.value.scalarTypeByte == S.BF16 and torch.equal(to_torch(out.value).float(), want.float())
    ref = R.embedding_gradients(lf.double(), tokens, segments, v, vs, l)
    mass = R.embedding_gradients(lf.double().abs(), tokens, segments, v, vs, l)
    terms = (_occurrences(tokens, v).view(v, 1), _occurrences(segments, vs).view(vs, 1), torch.full((1, 1, 1), b))
    for key, var, r, m, n in zip(KEYS, (twv, swv, pev), ref, mass, terms):
        got = to_torch(var.partialDerivative).double()
        bound = 2.0 ** -8 * r.abs() + n.double() * 2.0 ** -23 * m
        worst = ((got - r).abs() - bound).max().item()
        print(f"BF16 {name} {key}: max |err| {(got - r).abs().max().item():.3e}, max (|err| - bound) {worst:.3e}")
        assert worst <= 0, f"{key}: {worst:.3e} over the bound"


def _direct(name, dt, want=(True, True, True)):
    tokens, segments, _, _, _, lf, ref = _problem(name, dt)
    b, t, l, d, v, vs, _ = CASES[name]
    return B.bertEmbeddingBackward(to_sten(lf.to(dt)), to_sten(tokens), to_sten(segments), v, vs, l, 0, *want)


@pytest.mark.parametrize("name", ["hub_1280x8", "hub_4200x3", "long_d5", "long_d8", "b64t20", "spread_v70000"])
def test_backward_is_bitwise_reproducible(gpu, name):
    dt = torch.float32
    a, b = _direct(name, dt), _direct(name, dt)
    for x, y in zip(a, b):
        assert torch.equal(to_torch(x), to_torch(y))
    c = _library(name, dt, fused=True)
    for key, x in zip(KEYS, a):
        assert torch.equal(to_torch(x), c[key]), key


def test_launch_budget(gpu):
    """fused: one bert_embedding_fwd forward; backward none of the chain's kernels; composed: no bert_ kernel - a fused path that fell back
    would show here"""
    dt = torch.float32
    bert = lambda counts: {k: v for k, v in counts.items() if k.startswith("bert_")}
    for name in ("d8", "long_d8"):
        fused = _timer_counts(lambda: _library(name, dt, fused=True))
        assert fused.get("bert_embedding_fwd") == 1, fused
        assert "index_add" not in fused and "embedding_bwd_scan" not in fused and not any(k.startswith("index_select") for k in fused), fused
        expect = {"bert_embedding_fwd": 1, "bert_group_keys": 1, "bert_group_rowptr": 1, "bert_row_sum": 1, "bert_positional_bwd": 1}
        if CASES[name][0] * CASES[name][1] * 2 > _long():
            expect["bert_chunk_sum"] = 1
        assert bert(fused) == expect, fused
        composed = _timer_counts(lambda: _library(name, dt, fused=False))
        assert not bert(composed) and composed.get("embedding_bwd_scan", 0) == 2, composed


def test_null_outputs_skip_their_launches(gpu):
    dt, name = torch.float32, "long_d8"
    full = [to_torch(x) for x in _direct(name, dt)]
    grouping = {"bert_group_keys", "bert_group_rowptr", "bert_row_sum", "bert_chunk_sum"}
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, False, False)):
        got = []
        counts = _timer_counts(lambda: got.extend(_direct(name, dt, want)))
        for w, g, f in zip(want, got, full):
            assert (g is None) == (not w)
            if w:
                assert torch.equal(to_torch(g), f)
        names = {k for k in counts if k.startswith("bert_")}
        assert ("bert_positional_bwd" in names) == want[2], counts
        assert (grouping <= names) if (want[0] or want[1]) else not (grouping & names), counts
        assert all(counts[k] == 1 for k in names), counts


def test_errors(gpu):
    f = lambda *shape: to_sten(torch.zeros(*shape))
    ids = lambda b, t, dtype=torch.int64: to_sten(torch.zeros(b, t, dtype=dtype))
    with pytest.raises(LampError, match="positional table has 4 rows"):
        B.bertEmbeddingForward(f(5, 8), f(2, 8), f(1, 4, 8), ids(2, 5), ids(2, 5))
    with pytest.raises(LampError, match="columns"):
        B.bertEmbeddingForward(f(5, 8), f(2, 7), f(1, 6, 8), ids(2, 5), ids(2, 5))
    with pytest.raises(LampError, match="segments"):
        B.bertEmbeddingForward(f(5, 8), f(2, 8), f(1, 6, 8), ids(2, 5), ids(2, 4))
    with pytest.raises(LampError, match="int64"):
        B.bertEmbeddingForward(f(5, 8), f(2, 8), f(1, 6, 8), ids(2, 5, torch.int32), ids(2, 5))
    with pytest.raises(LampError, match="differ in type"):
        B.bertEmbeddingForward(f(5, 8), to_sten(torch.zeros(2, 8, dtype=F64)), f(1, 6, 8), ids(2, 5), ids(2, 5))
    with pytest.raises(LampError, match="int64"):
        B.bertEmbeddingBackward(f(2, 5, 8), ids(2, 5), ids(2, 5, torch.int32), 5, 2, 6)
    with pytest.raises(LampError, match="L = 4"):
        B.bertEmbeddingBackward(f(2, 5, 8), ids(2, 5), ids(2, 5), 5, 2, 4)
    for fused in (True, False):                # the node checks T against L in both forms
        prev = B.bertFused(fused)
        try:
            with pytest.raises(LampError, match="positional table has 4 rows"):
                B.bertEmbedding(A.const(ids(2, 5)), A.const(ids(2, 5)), A.param(f(5, 8)), A.param(f(2, 8)), A.param(f(1, 4, 8)))
        finally:
            B.bertFused(prev)


# ---- modules -----------------------------------------------------------------------------------------------------------------------------------------
MAXLEN, VOCAB, SEGS, DIM, HEADS, PER_HEAD, MLP, MLM_HIDDEN, WS_HIDDEN, PADTOKEN = 8, 11, 2, 8, 2, 4, 12, 6, 5, 0


def _reference_loss(blocks, linearized, perRow=False):
    dt = F64
    enc = [_oracle_encoder_block(DIM, PER_HEAD, HEADS, MLP, dt, linearized, False, False, 1000 * i) for i in range(blocks)]
    tw, sw, pe = _rand_params([(VOCAB, DIM), (SEGS, DIM), (1, MAXLEN, DIM)], dt, 77, 1.0)
    w1, b1, w2, b2 = _rand_params([(DIM, MLM_HIDDEN), (1, MLM_HIDDEN), (MLM_HIDDEN, VOCAB), (1, VOCAB)], dt, 177, 1.0)
    c1, cb1, c2, cb2 = _rand_params([(DIM, WS_HIDDEN), (1, WS_HIDDEN), (WS_HIDDEN, 1), (1, 1)], dt, 277, 1.0)
    return R.BertLoss(R.BertPretrain(R.BertEncoder(tw, sw, pe, enc), R.MaskedLanguageModel(w1, b1, w2, b2, perRow), c1, cb1, c2, cb2), PADTOKEN)


def _library_loss(om, blocks, linearized, perRow=False):
    hm = B.BertLoss(MAXLEN, VOCAB, SEGS, MLM_HIDDEN, WS_HIDDEN, blocks, DIM, PER_HEAD, HEADS, MLP, 0.0, PADTOKEN, S.F64, 0, linearized, None, perRow)
    assert [v.shape for v in hm.state] == [v.shape for v in om.state()]
    hm.load([to_sten(v.value) for v in om.state()])
    return hm


def _batch(with_max_length):
    t = 6                                                                      # T < maxLength: the last two positional rows get no gradient
    tokens = torch.tensor([[1, 4, 0, 7, 10, 2], [1, 9, 9, 2, 5, 2], [1, 3, 6, 2, 0, 0]])
    segments = torch.tensor([[0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 1, 1], [0, 0, 1, 1, 0, 0]])
    positions = torch.tensor([[1, 4], [2, 0], [1, 0]])
    target = torch.tensor([[4, 10], [9, PADTOKEN], [3, PADTOKEN]])             # two ignored positions
    whole = torch.tensor([1.0, 0.0, 1.0], dtype=F64)
    lengths = torch.tensor([6, 6, 4]) if with_max_length else None
    return tokens, segments, positions, lengths, target, whole


def _run_library(hm, batch, fused):
    tokens, segments, positions, lengths, target, whole = batch
    prev = B.bertFused(fused)
    try:
        loss = hm.forward(A.const(to_sten(tokens)), A.const(to_sten(segments)), to_sten(positions), to_sten(lengths) if lengths is not None else None,
                          to_sten(target), to_sten(whole))
        grads = hm.gradients(loss)
    finally:
        B.bertFused(prev)
    res = {"loss": to_torch(loss.value).reshape(1)}
    res.update({f"g{i}": to_torch(g) for i, g in enumerate(grads)})
    return res


@pytest.mark.parametrize("with_max_length", [True, False], ids=["maxLength", "noMaxLength"])
@pytest.mark.parametrize("linearized", [False, True], ids=["softmax", "linearized"])
@pytest.mark.parametrize("blocks", [1, 2])
def test_bert_loss_and_gradients_vs_restatement(gpu, blocks, linearized, with_max_length):
    """the loss and every parameter gradient under the rule, fused and composed; state order and count"""
    om = _reference_loss(blocks, linearized)
    hm = _library_loss(om, blocks, linearized)
    assert len(hm.state) == 3 + 10 * blocks + 4 + 4 and len(hm.parameters) == len(hm.state)
    assert [v.shape for v in hm.state][:3] == [[VOCAB, DIM], [SEGS, DIM], [1, MAXLEN, DIM]]
    batch = _batch(with_max_length)
    oloss = om.forward(*batch)
    ograds = om.gradients(oloss)
    ref = {"loss": oloss.value.reshape(1)}
    ref.update({f"g{i}": g for i, g in enumerate(ograds)})
    comp, fus = _run_library(hm, batch, False), _run_library(hm, batch, True)
    _rule("bert-loss", f"blocks{blocks}", F64, list(ref), ref, comp, fus)
    assert not fus["g0"][0].any() and not fus["g1"][0].any() and not fus["g2"][0, 6:].any() and fus["g2"][0, :6].any()


def test_per_row_positions_differs_as_the_restatement_says(gpu):
    batch = _batch(True)
    res = {}
    for perRow in (False, True):
        om = _reference_loss(1, False, perRow)
        hm = _library_loss(om, 1, False, perRow)
        ref = om.forward(*batch).value.item()
        got = _run_library(hm, batch, True)["loss"].item()
        assert abs(got - ref) <= 64 * EPS[F64] * abs(ref), (perRow, got, ref)
        res[perRow] = got
    assert abs(res[True] - res[False]) > 1e-6 * abs(res[False])


def test_pretrain_outputs_eval_mode_and_checkpoint_round_trip(gpu, tmp_path):
    om = _reference_loss(2, False)
    hm = _library_loss(om, 2, False)
    batch = _batch(True)
    tokens, segments, positions, lengths = (A.const(to_sten(batch[0])), A.const(to_sten(batch[1])), to_sten(batch[2]), to_sten(batch[3]))
    encoded, scores, whole = hm.pretrain(tokens, segments, positions, lengths)
    oenc, oscores, owhole = om.pretrain.forward(*batch[:4])
    assert encoded.shape == [3, 6, DIM] and scores.shape == [3, 2, VOCAB] and whole.shape == [3]
    for got, want in ((encoded, oenc), (scores, oscores), (whole, owhole)):
        assert _err(to_torch(got.value), want.value) <= 256 * EPS[F64]
    before = _run_library(hm, batch, True)["loss"]
    assert torch.equal(_run_library(hm.asEval(), batch, True)["loss"], before)          # dropout 0: the mode changes nothing
    hm.asTraining()
    path = os.path.join(str(tmp_path), "bert.ckpt")
    D.writeCheckpoint(path, hm)
    other = B.BertLoss(MAXLEN, VOCAB, SEGS, MLM_HIDDEN, WS_HIDDEN, 2, DIM, PER_HEAD, HEADS, MLP, 0.0, PADTOKEN, S.F64, 0, False)
    assert not torch.equal(_run_library(other, batch, True)["loss"], before)
    D.loadFromFile(other, path)
    for a, b in zip(other.state, hm.state):
        assert torch.equal(to_torch(a.value), to_torch(b.value))
    assert torch.equal(_run_library(other, batch, True)["loss"], before)


def test_default_positional_table_is_vaswani_in_single_precision(gpu):
    from oracle.lamp_transformer_oracle import vaswani
    for dtype, dt in ((S.F32, torch.float32), (S.F64, F64)):
        enc = B.BertEncoder(MAXLEN, VOCAB, SEGS, 1, DIM, PER_HEAD, HEADS, MLP, 0.0, dtype, 0)
        pe = enc.state[2]
        assert pe.needsGrad and pe.shape == [1, MAXLEN, DIM]
        assert torch.equal(to_torch(pe.value), vaswani(MAXLEN, DIM).float().to(dt).view(1, MAXLEN, DIM))
        out = enc.forward(A.const(to_sten(_batch(False)[0])), A.const(to_sten(_batch(False)[1])))
        assert out.shape == [3, 6, DIM]


def test_one_length_per_sequence_masks_the_padded_keys_for_every_query(gpu):
    """BertEncoder widens a 1-D maxLength [B] to [B, T]; the restatement does the same, so this is checked on its
    own.  The widened form has the bits of the explicit [B, T] tensor.  With a length of 4 for every sequence (softmax attention, two
    blocks) the tokens at positions >= 4 are keys nobody attends to: replacing them leaves the encoding of positions < 4 as it was, bit
    for bit (a masked key's weight is exactly 0), and changes the rest; without lengths the same replacement reaches every position.
    (Equal lengths on purpose: the reference repeats maxLength head-major over rows that are batch-major, so differing lengths land on
    other sequences' heads, as written.)"""
    enc = B.BertEncoder(MAXLEN, VOCAB, SEGS, 2, DIM, PER_HEAD, HEADS, MLP, 0.0, S.F64, 0)
    tokens, segments = _batch(False)[:2]
    length = 4
    run = lambda tk, mx: to_torch(enc.forward(A.const(to_sten(tk)), A.const(to_sten(segments)), to_sten(mx) if mx is not None else None).value)
    a = run(tokens, torch.full((3,), length))
    assert torch.equal(a, run(tokens, torch.full((3, 6), length)))
    other = tokens.clone()
    other[:, length:] = (tokens[:, length:] + 3) % VOCAB
    assert not torch.equal(other, tokens) and torch.equal(other[:, :length], tokens[:, :length])
    b = run(other, torch.full((3,), length))
    assert torch.equal(a[:, :length], b[:, :length]) and not torch.equal(a[:, length:], b[:, length:])
    assert not torch.equal(run(tokens, None)[:, :length], run(other, None)[:, :length])
    with pytest.raises(LampError, match="maxLength holds 2 lengths"):
        run(tokens, torch.full((2,), length))


# ---- one training loop ---------------------------------------------------------------------------------------------------------------------------------
def test_thirty_adamw_steps_lower_the_loss_and_fused_equals_composed_bit_for_bit(gpu):
    """the example's configuration (maxLength 32, width 32, four heads, two blocks) on a synthetic corpus from the batch builder, f32.  The
    mean loss over the corpus after 30 AdamW steps is below the mean loss before them.

    Fused against composed from one set of initial weights.  Against a restatement the rule's cap cannot be held after 30 steps: AdamW
    divides every gradient by the root of its running second moment, so a rounding in an element whose gradient is small moves that weight
    by up to a learning rate per step whatever the size of the rounding, and two correct f32 runs that differ in one summation order end
    0.13 of the largest weight apart (measured at batches of twelve sequences).  A bound that wide would let a wrong gradient through, so
    the loop is sized for the case where nothing may differ at all: batches of B = 2 sequences of T = 32.  Then no table row has more than
    2 T = 64 <= bertLongRow() occurrences, so every row of dToken and dSegment is one ascending sum in both forms, the scan kernel's order;
    dPositional is a sum of two terms, which has one value in any order; every prediction position is a real one, so a row of the masked
    language model's gather gradient has at most two addends as well; the forward has the chain's bits.  Every loss and every final
    parameter of the fused run must therefore equal the composed run's bit for bit: e_f = e_c against any reference, which is the rule
    with nothing to spare."""
    cls, sep, pad, mask, vocab, maxlen = 1, 2, 0, 3, 64, 32
    rng = np.random.default_rng(11)
    # sentences that continue each other: sentence k + 1 of a paragraph starts where sentence k stopped, so the next-sentence task can be
    # learnt; every sentence fills the window of (32 - 3) // 2 = 14 tokens, so every sequence has 31 tokens and int(31 * 0.15) = 4
    # prediction positions, as many as the batch has room for: no position is padding
    paragraphs = []
    for _ in range(12):
        start = int(rng.integers(4, vocab))
        sentences = []
        for _ in range(3):
            n = int(rng.integers(14, 20))
            sentences.append([4 + (start + k - 4) % (vocab - 4) for k in range(n)])
            start += n
        paragraphs.append(sentences)
    batches = list(B.minibatchesFromParagraphs(1, False, paragraphs, vocab, cls, sep, pad, mask, maxlen, rng))
    assert len(batches) == 12 and all(b["tokens"].shape == [2, maxlen] for b in batches) and 2 * maxlen <= _long()
    assert all(to_torch(b["maxLength"]).tolist() == [31, 31] and b["positions"].shape == [2, 4] for b in batches)
    make = lambda: B.BertLoss(maxlen, vocab, 2, 32, 32, 2, 32, 8, 4, 64, 0.0, pad, S.F32, 0, False)
    init = [v.value.cloneTensor() for v in make().state]

    def run(fused):
        m = make()
        m.load(init)
        params = m.parameters
        opt = nn.AdamW([p.value for p in params], weightDecay=0.0, learningRate=3e-3)
        forward = lambda b: m.forward(b["tokens"], b["segments"], b["positions"], b["maxLength"], b["maskedLanguageModelTarget"], b["wholeSentenceTarget"])
        mean = lambda: sum(to_torch(forward(b).value).item() for b in batches) / len(batches)
        prev = B.bertFused(fused)
        try:
            losses = [mean()]
            for step in range(30):
                loss = forward(batches[step % len(batches)])
                losses.append(to_torch(loss.value).item())
                opt.step(m.gradients(loss))
            losses.append(mean())
        finally:
            B.bertFused(prev)
        return losses, [to_torch(p.value) for p in params]

    comp_losses, comp = run(False)
    fus_losses, fus = run(True)
    worst = max((a.double() - b.double()).abs().max().item() for a, b in zip(fus, comp))
    print(f"TRAIN mean loss before {fus_losses[0]:.4f} after {fus_losses[-1]:.4f}; composed {comp_losses[0]:.4f} -> {comp_losses[-1]:.4f}; "
          f"max |fused - composed| over {len(fus)} parameters {worst:.3e}, over the losses {max(abs(a - b) for a, b in zip(fus_losses, comp_losses)):.3e}")
    assert all(math.isfinite(x) for x in fus_losses)
    assert fus_losses[-1] < fus_losses[0]
    assert fus_losses == comp_losses
    for k, (a, b) in enumerate(zip(fus, comp)):
        assert torch.equal(a, b), f"parameter {k}"
