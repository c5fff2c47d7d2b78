"""Recurrent family on the GPU, everything through the C ABI: the fused nodes against the f64 restatement (tests/recurrent_ref.py)
with a tolerance measured on the library's own composed chain, the launch budget, gradients through the returned states, and the
example model (Embedding -> LSTM -> relu -> SeqLinear -> logSoftMax with SequenceNLL and AdamW) end to end."""
import ctypes as C
import os
import tempfile

import pytest
import torch

from lamp_amd import autograd as A, nn, recurrent as RC, sten as S, transformer as TF
from lamp_amd._capi import lib
from tests import recurrent_ref as R
from tests.util import closed_form, to_sten, to_torch, TORCH2LAMP

pytestmark = pytest.mark.gpu
F64 = torch.float64
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
# The floor of the rule e_f <= 4 * e_c + floor, as a multiple of the dtype's eps.  It keeps an e_c of exactly 0 on tiny shapes from
# failing the test, and it carries the one term the factor 4 does not: the one-product weight gradients sum K = T * B products in one
# dot product where the chain adds T partial sums of B products, and a sum of K rounded terms is off by about eps * sqrt(K) of its
# largest value - sqrt(4096) = 64 eps at the largest shape here.  Measured on an MI355X (max over shapes, bias forms and tensors;
# "needed" = (e_f - 4 e_c) / eps where positive):
#            e_c       e_f       needed   (e_c == 0 cases: e_f <= 2.9 eps, all at shape (1, 1, 1, 1))
#   rnn  f64 1.66e-14  2.04e-14   4.1
#   gru  f64 7.31e-15  1.07e-14  28.4     (recurrent weight gradients at (16, 256, 20, 1024): e_c 1.1e-15, e_f 1.06e-14)
#   lstm f64 6.39e-15  1.10e-14  29.1
#   rnn  f32 3.23e-06  5.08e-06  14.0
#   gru  f32 7.99e-07  5.55e-06  20.8
#   lstm f32 8.48e-07  7.07e-06  37.1
# The f64 run needs 29 eps, the same multiple as f32: rounding of the longer sums, not arithmetic that differs.  64 covers it twice.
FLOOR_EPS = 64

SHAPES = {"rnn": lambda i, h: [(i, h), (h, h)], "gru": lambda i, h: [(i, h), (h, h), (i, h), (i, h), (h, h), (h, h)],
          "lstm": lambda i, h: [(i, h)] * 3 + [(h, h)] * 3 + [(i, h), (h, h)]}
NBIAS = {"rnn": 1, "gru": 3, "lstm": 4}
MODULE = {"rnn": RC.RNN, "gru": RC.GRU, "lstm": RC.LSTM}
BWD_CELL = {"rnn": "rnn_cell_bwd", "gru": "gru_output_bwd", "lstm": "lstm_cell_bwd"}


def _inputs(kind, T, B, In, H, dt, bias2d, with_state, salt=0):
    """closed-form operands rounded to `dt` (so that both sides start from the same numbers), as f64"""
    sc = 2.0 / (In + H) ** 0.5
    w = [closed_form(s, salt + 11 * k, 2 * sc, F64) for k, s in enumerate(SHAPES[kind](In, H))]
    w += [closed_form((1, H) if bias2d else (H,), salt + 101 + k, 0.5, F64) for k in range(NBIAS[kind])]
    x = closed_form((T, B, In), salt + 7, 2.0, F64)
    nstate = 2 if kind == "lstm" else 1
    state = [closed_form((B, H), salt + 201 + k, 1.0, F64) for k in range(nstate)] if with_state else None
    # a fixed linear functional of out, h_T (and c_T): all results receive gradients
    L = [closed_form((T, B, H), salt + 301, 1.0, F64)] + [closed_form((B, H), salt + 311 + k, 1.0, F64) for k in range(nstate)]
    rd = lambda t: t.to(dt).to(F64)
    return [rd(t) for t in w], rd(x), [rd(t) for t in state] if state else None, [rd(t) for t in L]


def _reference(kind, w, x, state, L):
    w = [t.clone().requires_grad_(True) for t in w]
    x = x.clone().requires_grad_(True)
    st = [t.clone().requires_grad_(True) for t in state] if state else None
    if kind == "lstm":
        res = R.lstm(x, w, tuple(st) if st else None)
    else:
        res = (R.rnn if kind == "rnn" else R.gru)(x, w, st[0] if st else None)
    sum((r * l).sum() for r, l in zip(res, L)).backward()
    named = {"out": res[0], "h_T": res[1], "dx": x.grad}
    if kind == "lstm": named["c_T"] = res[2]
    for k, t in enumerate(w): named[f"dstate{k}"] = t.grad
    if st:
        for k, t in enumerate(st): named[f"dinit{k}"] = t.grad
    return {k: v.detach() for k, v in named.items()}


def _library(kind, w, x, state, L, dt, fused, device=0, consume=None):
    """the same computation through the C ABI; consume: which results enter the loss (default all)"""
    prev = RC.recurrentFused(fused)
    try:
        ts = lambda t: to_sten(t.to(dt), device=device)
        mod = MODULE[kind](tensors=[ts(t) for t in w])
        xv = A.param(ts(x))
        st = [A.param(ts(t)) for t in state] if state else None
        out, nxt = mod.forward(xv, st)
        res = [out] + list(nxt)
        use = range(len(res)) if consume is None else consume
        loss = None
        for k in use:
            term = (res[k] * A.const(ts(L[k]))).sum()
            loss = term if loss is None else loss + term
        loss.backprop()
        named = {"out": to_torch(out.value), "h_T": to_torch(nxt[0].value), "dx": to_torch(xv.partialDerivative)}
        if kind == "lstm": named["c_T"] = to_torch(nxt[1].value)
        for k, p in enumerate(mod.state): named[f"dstate{k}"] = to_torch(p.partialDerivative)
        if st:
            for k, p in enumerate(st): named[f"dinit{k}"] = to_torch(p.partialDerivative)
        return named
    finally:
        RC.recurrentFused(prev)


def _err(got, ref):
    assert list(got.shape) == list(ref.shape), f"shape {list(got.shape)} vs {list(ref.shape)}"
    den = ref.abs().max().item()
    return (got.double() - ref).abs().max().item() / (den if den > 0 else 1.0)


def _check_against_composed(kind, w, x, state, L, dt, what, consume=None, ref=None):
    ref = ref if ref is not None else _reference(kind, w, x, state, L)
    comp = _library(kind, w, x, state, L, dt, fused=False, consume=consume)
    fus = _library(kind, w, x, state, L, dt, fused=True, consume=consume)
    floor = FLOOR_EPS * EPS[dt]
    for name, r in ref.items():
        e_c, e_f = _err(comp[name], r), _err(fus[name], r)
        print(f"{what} {name}: e_c {e_c:.3e} e_f {e_f:.3e} (floor {floor:.1e})")
        assert e_f <= 4 * e_c + floor, f"{what}: {name}: fused error {e_f:.3e} > 4 * composed error {e_c:.3e} + {floor:.1e}"


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["rnn", "gru", "lstm"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (7, 5, 3, 33), (3, 2, 20, 130), (16, 256, 20, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_fused_vs_restatement(gpu, kind, dt, shape):
    """e_f <= 4 * e_c + 64 eps per tensor (output, last states, every parameter, input and initial-state gradient), e_c / e_f the max-abs
    errors of the composed and the fused form against the f64 restatement over the restatement's max magnitude.  Both bias shapes, with
    and without a passed initial state.  Measured (MI355X, max over all cases): f64 e_c 1.7e-14, e_f 2.0e-14; f32 e_c 3.2e-6, e_f 7.1e-6; the floor
    multiple is 64 (table at FLOOR_EPS; EXPERIMENTS.md, "Recurrent nodes").  The figures are printed per tensor (run with -s)."""
    T, B, In, H = shape
    big = T * B * H > 1 << 20
    for bias2d, with_state in ([(True, True), (False, False)] if big else [(False, False), (True, True), (False, True)]):
        w, x, state, L = _inputs(kind, T, B, In, H, dt, bias2d, with_state)
        _check_against_composed(kind, w, x, state, L, dt, f"{kind} {shape} bias2d={bias2d} state={with_state}")


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


@pytest.mark.parametrize("kind,per_step,cells", [("lstm", 4, ["lstm_cell_fwd", "lstm_cell_bwd"]), ("rnn", 4, ["rnn_cell_fwd", "rnn_cell_bwd"]),
                                                 ("gru", 8, ["gru_gates_fwd", "gru_output_fwd", "gru_output_bwd", "gru_gates_bwd"])])
def test_launch_budget(gpu, kind, per_step, cells):
    """forward + backward at T = 12 and T = 24: every cell kernel ran exactly T times and the total of tagged launches grows by at most
    2 per added step and direction (GRU 4); the composed chain grows by more, so a fused path that fell back would be noticed."""
    dt = torch.float32
    totals = {}
    for fused in (True, False):
        for T in (12, 24):
            w, x, state, L = _inputs(kind, T, 8, 20, 64, dt, True, False)
            counts = _timer_counts(lambda: _library(kind, w, x, state, L, dt, fused=fused))
            totals[(fused, T)] = sum(counts.values())
            if fused:
                for c in cells:
                    assert counts.get(c, 0) == T, f"{c} ran {counts.get(c, 0)} times at T = {T}: {counts}"
            else:
                assert not any(c in counts for c in cells), f"cell kernels ran with the toggle off: {counts}"
    grow_f = totals[(True, 24)] - totals[(True, 12)]
    grow_c = totals[(False, 24)] - totals[(False, 12)]
    print(f"{kind}: tagged launches fused {totals[(True, 12)]} -> {totals[(True, 24)]}, composed {totals[(False, 12)]} -> {totals[(False, 24)]}")
    assert grow_f <= per_step * 12, f"{kind}: {grow_f} more launches for 12 more steps, the budget is {per_step} per step"
    assert grow_c > grow_f, f"{kind}: the composed chain grew by {grow_c}, the fused form by {grow_f}"


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_gradients_through_states(gpu, kind):
    """two chained calls, the second starting from the first's last state, against the restatement; then only the last state consumed
    (LSTM: only c_T) and `out` not consumed at all: the one shared backward still delivers every gradient"""
    dt = F64
    T, B, In, H = 5, 3, 4, 6
    w, x, _, L = _inputs(kind, T, B, In, H, dt, True, False)
    x2 = closed_form((T, B, In), 999, 2.0, F64)
    # restatement
    wr = [t.clone().requires_grad_(True) for t in w]
    xr = x.clone().requires_grad_(True)
    if kind == "lstm":
        o1, h1, c1 = R.lstm(xr, wr)
        o2, h2, c2 = R.lstm(x2, wr, (h1, c1))
        last = [h2, c2]
    else:
        o1, h1 = R.gru(xr, wr)
        o2, h2 = R.gru(x2, wr, h1)
        last = [h2]
    ((o2 * L[0]).sum() + sum((s * l).sum() for s, l in zip(last, L[1:]))).backward()
    for fused in (False, True):
        prev = RC.recurrentFused(fused)
        try:
            mod = MODULE[kind](tensors=[to_sten(t) for t in w])
            xv = A.param(to_sten(x))
            _, s1 = mod.forward(xv, None)
            out2, s2 = mod.forward(A.const(to_sten(x2)), list(s1))
            loss = (out2 * A.const(to_sten(L[0]))).sum()
            for s, l in zip(s2, L[1:]):
                loss = loss + (s * A.const(to_sten(l))).sum()
            counts = _timer_counts(loss.backprop)
            if fused:                                 # two nodes, each one's backward exactly once: T backward cells per node
                assert counts.get(BWD_CELL[kind], 0) == 2 * T, f"{kind}: chained calls ran {counts} backward cells, expected {2 * T}"
            assert _err(to_torch(xv.partialDerivative), xr.grad) < 1e-12, f"{kind} fused={fused}: input gradient through the state"
            for k, p in enumerate(mod.state):
                assert _err(to_torch(p.partialDerivative), wr[k].grad) < 1e-12, f"{kind} fused={fused}: state tensor {k} through the state"
        finally:
            RC.recurrentFused(prev)
    # one result consumed only: the last one (c_T for LSTM, h_T for GRU)
    w, x, state, L = _inputs(kind, T, B, In, H, dt, False, True, salt=50)
    only = [2] if kind == "lstm" else [1]
    ref = _reference(kind, w, x, state, [l if k in only else torch.zeros_like(l) for k, l in enumerate(L)])
    _check_against_composed(kind, w, x, state, L, dt, f"{kind} only result {only}", consume=only, ref=ref)
    # ... and in that case (`out` has no consumer, LSTM's h_T neither) the shared backward ran once: T backward cells
    counts = _timer_counts(lambda: _library(kind, w, x, state, L, dt, fused=True, consume=only))
    assert counts.get(BWD_CELL[kind], 0) == T, f"{kind}: only result {only} consumed, {counts} backward cells, expected {T}"
    # every result consumed: still once
    counts = _timer_counts(lambda: _library(kind, w, x, state, L, dt, fused=True))
    assert counts.get(BWD_CELL[kind], 0) == T, f"{kind}: all results consumed, {counts} backward cells, expected {T}"


def _example_model(V, H, dt, device=0):
    ldt = TORCH2LAMP[dt]
    emb, lstm, lin = TF.Embedding(V, 20, ldt, device), RC.LSTM(20, H, ldt, device), RC.SeqLinear(H, V, ldt, device)
    return RC.statefulSequence(emb, lstm, nn.Fun("relu"), lin, nn.Fun("logsoftmax", 2)), 1 + 12 + 2


def _example_reference(state, tokens, target, cw):
    e, w, lin = state[0], state[1:13], state[13:15]
    out, _, _ = R.lstm(torch.nn.functional.embedding(tokens, e), w)
    y = torch.log_softmax(R.seq_linear(out.relu(), lin), 2)
    return R.sequence_nll(y, target, cw)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_example_model_end_to_end(gpu, dt):
    """timemachine's model at (T, B, V, H) = (20, 64, 50, 256): three AdamW(clip = 1) steps with SequenceNLL, targets with ignored entries
    and one time step ignored entirely; loss, example count and the parameters after the steps against the restatement under the rule of
    test_fused_vs_restatement (composed vs fused), then a checkpoint round trip in the reference's state order."""
    T, B, V, H = 20, 64, 50, 256
    tokens = (torch.arange(T * B).reshape(T, B) * 7 + 3) % V
    target = (torch.arange(T * B).reshape(T, B) * 11 + 5) % V
    target[4, :] = -100
    target[9, ::3] = -100
    cw = torch.ones(V, dtype=dt)
    init = None
    results = {}
    for fused in (False, True):
        prev = RC.recurrentFused(fused)
        try:
            m, nstate = _example_model(V, H, dt)
            if init is None:
                init = [to_torch(v.value).clone() for v in m.state]
            m.load([to_sten(t) for t in init])
            assert len(m.state) == nstate
            model = nn.SupervisedModel(m, RC.SEQUENCE_NLL, to_sten(cw))
            opt = nn.AdamW([p.value for p in m.parameters], weightDecay=0.0, learningRate=1e-3, clip=1.0)
            acc = S.STen.zeros([1], S.F64)
            n = 0
            for _ in range(3):
                n = model.train_step(opt, to_sten(tokens), to_sten(target), acc)
            results[fused] = (n, to_torch(acc).item(), [to_torch(v.value) for v in m.state], m)
        finally:
            RC.recurrentFused(prev)
    # the restatement: the same three steps with torch's AdamW arithmetic restated (AdamW.scala:113-176, debias, clip = 1)
    ps = [t.double().clone().requires_grad_(True) for t in init]
    mt = [torch.zeros_like(p) for p in ps]; vt = [torch.zeros_like(p) for p in ps]
    total = 0.0
    for step in range(1, 4):
        loss, n_ref = _example_reference(ps, tokens, target, cw.double())
        gs = torch.autograd.grad(loss, ps)
        norm = torch.sqrt(sum((g * g).sum() for g in gs))
        if norm > 1.0: gs = [g / norm for g in gs]
        total += loss.item() * n_ref
        with torch.no_grad():
            for p, g, m1, v1 in zip(ps, gs, mt, vt):
                m1.mul_(0.9).add_(g, alpha=0.1); v1.mul_(0.999).addcmul_(g, g, value=0.001)
                p.sub_(1e-3 * (1 - 0.999 ** step) ** 0.5 / (1 - 0.9 ** step) * m1 / (v1.sqrt() + 1e-8))   # AdamW.scala:150-170
    assert n_ref == T * B - B - len(range(0, B, 3))
    floor = FLOOR_EPS * EPS[dt]
    for fused in (False, True):
        assert results[fused][0] == n_ref, f"example count {results[fused][0]} (fused={fused}), the restatement counts {n_ref}"
    e_c, e_f = abs(results[False][1] - total) / abs(total), abs(results[True][1] - total) / abs(total)
    print(f"{dt}: accumulated loss e_c {e_c:.3e} e_f {e_f:.3e}")
    assert e_f <= 4 * e_c + floor
    for k, p in enumerate(ps):
        e_c, e_f = _err(results[False][2][k], p.detach()), _err(results[True][2][k], p.detach())
        print(f"{dt}: state {k} after three steps e_c {e_c:.3e} e_f {e_f:.3e}")
        assert e_f <= 4 * e_c + floor, f"state {k}: fused {e_f:.3e} > 4 * composed {e_c:.3e} + {floor:.1e}"
    # checkpoint: the reference's order and shapes, reloaded into a fresh model
    m = results[True][3]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ckpt")
        lib.lamp_module_write_checkpoint(m.h, path.encode())
        fresh, _ = _example_model(V, H, dt)
        lib.lamp_module_load_from_file(fresh.h, path.encode())
        want = [(V, 20)] + [(20, H)] * 3 + [(H, H)] * 3 + [(20, H), (H, H)] + [(1, H)] * 4 + [(H, V), (1, V)]
        assert [tuple(v.value.shape) for v in fresh.state] == want
        for a, b in zip(fresh.state, m.state):
            assert torch.equal(to_torch(a.value), to_torch(b.value))


def test_rnn_known_answer_gpu_and_host(gpu):
    """nn.test.scala:618-644 in f64 on the GPU (fused) and with host tensors (the composed fallback), to the reference's 4 decimals; the
    loss is the library's SequenceNLL (loss_kind 3) through SupervisedModel: the accumulator receives loss * count"""
    x = torch.arange(12, dtype=F64).view(2, 3, 2)
    w = [torch.ones(2, 4, dtype=F64), torch.ones(4, 4, dtype=F64), torch.ones(4, dtype=F64)]
    for device in (0, -1):
        mod = RC.RNN(tensors=[to_sten(t, device=device) for t in w])
        out, _ = mod.forward(A.const(to_sten(x, device=device)), None)
        assert list(out.value.shape) == [2, 3, 4]
        model = nn.SupervisedModel(mod, RC.SEQUENCE_NLL, to_sten(torch.ones(4, dtype=F64), device=device))
        acc = S.STen.zeros([1], S.F64, device)
        n = model.addTotalLossAndReturnNumExamples(to_sten(x, device=device), to_sten(torch.ones(2, 3, dtype=torch.int64), device=device), acc)
        assert n == 6
        assert round(to_torch(acc).item() / n, 4) == round(-0.9940025479340507, 4), f"device {device}: loss {to_torch(acc).item() / n}"


FD_SHAPES = {"rnn": [(2, 4), (4, 4), (4,)], "gru": [(2, 4), (4, 4), (2, 4), (2, 4), (4, 4), (4, 4), (4,), (4,), (4,)],
             "lstm": [(2, 4)] * 3 + [(4, 4)] * 3 + [(2, 4), (4, 4)] + [(4,)] * 4, "seq_linear": [(2, 4), (4,)]}


@pytest.mark.parametrize("device", [0, -1], ids=["gpu", "host"])
@pytest.mark.parametrize("kind", ["rnn", "gru", "lstm", "seq_linear"])
def test_gradient_finite_differences_c_abi(gpu, kind, device):
    """testGradientAndValueND (nn.test.scala:105-190) through the C ABI: sum(module(x)) in f64, central differences with eps 1e-6 agree
    with backprop to 4 decimals, for every state tensor; input [2, 3, 2], hidden 4, [4]-shaped biases, closed-form weights.  On the GPU
    device (the fused nodes) and with host tensors (the CPU device: the composed fallback, forward and backward)."""
    x = closed_form((2, 3, 2), 5, 2.0, F64)
    w = [closed_form(s_, 17 + 13 * i, 1.0, F64) for i, s_ in enumerate(FD_SHAPES[kind])]

    def build(ws):
        ts = [to_sten(t, device=device) for t in ws]
        return RC.SeqLinear(tensors=ts) if kind == "seq_linear" else MODULE[kind](tensors=ts)

    def value(ws, backprop=False):
        mod = build(ws)
        r = mod.forward(A.const(to_sten(x, device=device)))
        out = r if kind == "seq_linear" else r[0]
        total = out.sum()
        if backprop:
            total.backprop()
            return [to_torch(p.partialDerivative) for p in mod.state]
        return to_torch(total.value).item()

    grads = value(w, backprop=True)
    eps = 1e-6
    for k, p in enumerate(w):
        fd = torch.zeros(p.numel(), dtype=F64)
        for j in range(p.numel()):
            def at(d):
                q = p.clone().reshape(-1); q[j] += d
                ws = list(w); ws[k] = q.reshape(p.shape)
                return value(ws)
            fd[j] = (at(eps) - at(-eps)) / (2 * eps)
        fd = fd.reshape(p.shape)
        assert torch.equal(torch.round(fd * 1e4), torch.round(grads[k] * 1e4)), \
            f"{kind} device {device}: state tensor {k}: backprop differs from central differences by {(fd - grads[k]).abs().max().item():.3e}"


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_example_model_graph_replay(gpu, dt):
    """the example model's three AdamW(clip = 1) steps with forward + loss + backward replayed from a captured graph equal the eager steps
    bitwise (parameters and the loss accumulator): no host value enters the nodes or the loss.  The batches differ in their ignored
    targets.  Specified for the capture itself: the example count it returns is time * batch (the kept count cannot be read while
    nothing runs); the accumulator receives the sum-reduced loss, a device value, so it is exact on every replay."""
    T, B, V, H = 20, 64, 50, 256
    ldt = TORCH2LAMP[dt]
    batches = []
    for i in range(3):
        tokens = (torch.arange(T * B).reshape(T, B) * (7 + 2 * i) + 3) % V
        target = (torch.arange(T * B).reshape(T, B) * 11 + 5 + i) % V
        target[4 + i, :] = -100
        target[9, i::3] = -100
        batches.append((tokens, target))
    cw = to_sten(torch.ones(V, dtype=dt))
    em, _ = _example_model(V, H, dt)
    init = [to_torch(v.value).clone() for v in em.state]
    emodel = nn.SupervisedModel(em, RC.SEQUENCE_NLL, cw)
    eopt = nn.AdamW([p.value for p in em.parameters], weightDecay=0.0, learningRate=1e-3, clip=1.0)
    eacc = S.STen.zeros([1], ldt)
    kept = []
    for x, t in batches:
        kept.append(emodel.train_step(eopt, to_sten(x), to_sten(t), eacc))
    assert kept == [int((t != -100).sum()) for _, t in batches]
    st = C.c_void_p(); lib.lamp_stream_get_from_pool(0, 0, C.byref(st))
    dflt = C.c_void_p(); lib.lamp_stream_get_default(0, C.byref(dflt))
    lib.lamp_device_synchronize()
    lib.lamp_stream_set_current(st)
    try:
        gm, _ = _example_model(V, H, dt)
        gm.load([to_sten(t) for t in init])
        gmodel = nn.SupervisedModel(gm, RC.SEQUENCE_NLL, cw)
        gopt = nn.AdamW([p.value for p in gm.parameters], weightDecay=0.0, learningRate=1e-3, clip=1.0)
        gacc = S.STen.zeros([1], ldt)
        x_buf, t_buf = to_sten(batches[0][0]), to_sten(batches[0][1])
        gmodel.addTotalLossAndReturnGradientsAndNumExamples(x_buf, t_buf, S.STen.zeros([1], ldt))   # eager warm-up (attributes, caches)
        lib.lamp_device_synchronize()
        lib.lamp_graph_begin_capture()
        n, grads = gmodel.addTotalLossAndReturnGradientsAndNumExamples(x_buf, t_buf, gacc)
        g = C.c_void_p(); lib.lamp_graph_end_capture(C.byref(g))
        assert n == T * B
        for x, t in batches:
            x_buf.copyFrom(to_sten(x)); t_buf.copyFrom(to_sten(t))
            lib.lamp_graph_launch(g)
            gopt.step(grads, 1.0)
        lib.lamp_device_synchronize()
        for k, (a, b) in enumerate(zip(gm.state, em.state)):
            assert torch.equal(to_torch(a.value), to_torch(b.value)), f"state {k} after three replayed steps differs from the eager steps"
        assert torch.equal(to_torch(gacc), to_torch(eacc)), "loss accumulator after three replayed steps"
        lib.lamp_graph_release(g)
    finally:
        lib.lamp_stream_set_current(dflt)


@pytest.mark.parametrize("kind", ["rnn", "gru", "lstm"])
def test_bf16_takes_the_composed_path(gpu, kind):
    """bf16 operands: no cell kernel runs (the toggle is on), and the composed chain agrees with the f64 restatement of the bf16-rounded
    operands at the bf16 tolerances of tests/test_transformer.py (forward 2^-6, gradients 2^-5, max-magnitude scale)."""
    from tests.util import assert_close
    dt = torch.bfloat16
    T, B, In, H = 4, 4, 6, 8
    w, x, state, L = _inputs(kind, T, B, In, H, dt, True, True)
    ref = _reference(kind, w, x, state, L)
    got = {}
    counts = _timer_counts(lambda: got.update(_library(kind, w, x, state, L, dt, fused=True)))
    assert not any("cell" in c or c.startswith("gru_") for c in counts), f"bf16 reached the fused cells: {counts}"
    for name, r in ref.items():
        assert_close(got[name], r, 2.0 ** -6 if name in ("out", "h_T", "c_T") else 2.0 ** -5, f"{kind} bf16 {name}", scale="max")
