"""Recurrent text generation on the GPU, everything through the C ABI: the step kernel and lamp_log_softmax_argmax_rows one by one,
sequencePrediction and sequencePredictionBeam on both paths against the f64 restatement (tests/text_ref.py), the launch budget, and
FreeRunningRNN / Seq2Seq / WithInit as differentiable modules.

The rule is the one of tests/test_recurrent_gpu.py: per tensor e_f <= 4 * e_c + 64 eps, e_c the error of the library's existing path (the
module's forward at one time step, the chain), e_f the new path's, both against the restatement over the restatement's largest magnitude."""
import ctypes as C

import numpy as np
import pytest
import torch

from lamp_amd import autograd as A, nn, recurrent as RC, sten as S, text as TX, transformer as TF
from lamp_amd._capi import lib
from tests import text_ref as TR
from tests.util import FWD_TOL, TORCH2LAMP, assert_close, closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu
F64 = torch.float64
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
FLOOR_EPS = 64
KIND = {"rnn": TX.RNN, "gru": TX.GRU, "lstm": TX.LSTM}
MODULE = {"rnn": RC.RNN, "gru": RC.GRU, "lstm": RC.LSTM}
SHAPES = {"rnn": lambda i, h: [(i, h), (h, h)], "gru": lambda i, h: [(i, h), (h, h), (i, h), (i, h), (h, h), (h, h)],
          "lstm": lambda i, h: [(i, h)] * 3 + [(h, h)] * 3 + [(i, h), (h, h)]}
NBIAS = {"rnn": 1, "gru": 3, "lstm": 4}
DTS = pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
KINDS = pytest.mark.parametrize("kind", ["rnn", "gru", "lstm"])


def _cell_weights(kind, E, H, dt, bias2d, salt=0):
    sc = 2.0 / (E + H) ** 0.5
    w = [closed_form(s, salt + 11 * k, 2 * sc, F64) for k, s in enumerate(SHAPES[kind](E, H))]
    w += [closed_form((1, H) if bias2d else (H,), salt + 101 + k, 0.5, F64) for k in range(NBIAS[kind])]
    return [t.to(dt).to(F64) for t in w]


def _err(got, ref):
    assert list(got.shape) == list(ref.shape), f"shape {list(got.shape)} vs {list(ref.shape)}"
    den = ref.abs().max().item()
    return (got.double() - ref).abs().max().item() / (den if den > 0 else 1.0)


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


# ---- lamp_recurrent_decode_step -------------------------------------------------------------------------------------------------------------
TOKENS = [6, 0, 3, 3, 1, 5, 2, 4, 6, 0, 3, 1, 5, 2, 4, 6]       # a table of 7 rows: 0 and 6 present, repeats across rows
STEP_SHAPES = [(R, E, H) for R in (1, 3, 16) for E in (3, 8) for H in (5, 64, 320)] + [(1, 8, 640), (3, 8, 640)]      # (R, E, H)


def _step_inputs(kind, dt, R, E, H, bias2d):
    """the cell's weights, the embedding table, the tokens and the previous state of a step case, f64 holding values of dt (also the
    inputs of scripts/decode_digest.py)"""
    w = _cell_weights(kind, E, H, dt, bias2d, salt=R + E)
    table = closed_form((7, E), 5, 2.0, F64).to(dt).to(F64)
    tok = torch.tensor(TOKENS[:R] if R > 1 else [6], dtype=torch.int64)
    nstate = 2 if kind == "lstm" else 1
    state = [closed_form((R, H), 201 + k, 1.0, F64).to(dt).to(F64) for k in range(nstate)]
    return w, table, tok, state


def _step_case(kind, dt, R, E, H, bias2d):
    what = f"{kind} {dt} R={R} E={E} H={H} bias2d={bias2d}"
    ts = lambda t: to_sten(t.to(dt))
    w, table, tok, state = _step_inputs(kind, dt, R, E, H, bias2d)
    x = table[tok].unsqueeze(0)                                                     # Embedding(tokens) at one time step
    ref_out, ref_state = TR.cell_forward(kind, x, w, state)
    # e_c: the module's own forward at T = 1
    mod = MODULE[kind](tensors=[ts(t) for t in w])
    _, nxt = mod.forward(A.const(ts(x)), [A.const(ts(t)) for t in state])
    chain = [to_torch(v.value) for v in nxt]
    # e_f: the step kernel, tokens as a strided column
    packed = TX.recurrentDecodePack(KIND[kind], [ts(t) for t in w])
    column = to_sten(torch.stack([tok, tok + 100], 1)).select(1, 0)
    args = dict(hPrev=ts(state[0]), cPrev=ts(state[1]) if kind == "lstm" else None)
    h, c, rl = TX.recurrentDecodeStep(KIND[kind], ts(table), column, packed, relu=True, **args)
    fused = [to_torch(h)] + ([to_torch(c)] if kind == "lstm" else [])
    floor = FLOOR_EPS * EPS[dt]
    for name, r, cc, ff in zip(("h", "c"), ref_state, chain, fused):
        e_c, e_f = _err(cc, r), _err(ff, r)
        print(f"{what} {name}: e_c {e_c:.3e} e_f {e_f:.3e} (floor {floor:.1e})")
        assert e_f <= 4 * e_c + floor, f"{what}: {name}: step kernel error {e_f:.3e} > 4 * module error {e_c:.3e} + {floor:.1e}"
    assert torch.equal(to_torch(rl), fused[0].relu()), f"{what}: the relu copy"
    # twice on the same inputs: the same bits
    h2, c2, _ = TX.recurrentDecodeStep(KIND[kind], ts(table), column, packed, relu=False, **args)
    assert torch.equal(to_torch(h2), fused[0]) and (kind != "lstm" or torch.equal(to_torch(c2), fused[1])), f"{what}: not reproducible"
    # parent: a permutation with a repeat against gathering the state first
    if R > 1:
        parent = torch.tensor([(2 * r + 2) % R for r in range(R - 1)] + [2 % R], dtype=torch.int64)
        hp, cp, _ = TX.recurrentDecodeStep(KIND[kind], ts(table), column, packed, parent=to_sten(parent), **args)
        gathered = dict(hPrev=ts(state[0][parent]), cPrev=ts(state[1][parent]) if kind == "lstm" else None)
        hg, cg, _ = TX.recurrentDecodeStep(KIND[kind], ts(table), column, packed, **gathered)
        assert torch.equal(to_torch(hp), to_torch(hg)) and (kind != "lstm" or torch.equal(to_torch(cp), to_torch(cg))), f"{what}: parent"
        # fewer rows than the previous state: two rows continuing rows of a state of R
        two = to_sten(torch.tensor([tok[0].item(), tok[1].item()]))
        hq, _, _ = TX.recurrentDecodeStep(KIND[kind], ts(table), two, packed, parent=to_sten(torch.tensor([R - 1, 0])), **args)
        sel = torch.tensor([R - 1, 0])
        hr, _, _ = TX.recurrentDecodeStep(KIND[kind], ts(table), two, packed, hPrev=ts(state[0][sel]), cPrev=ts(state[1][sel]) if kind == "lstm" else None)
        assert torch.equal(to_torch(hq), to_torch(hr)), f"{what}: parent into a larger state"


@DTS
@KINDS
def test_step_kernel_vs_module_and_restatement(gpu, kind, dt):
    """R in {1, 3, 16} x E in {3, 8} x H in {5 (element form, partial tile), 64, 320 (several column tiles and slices of K: the ticket path)},
    then H = 640 at E = 8 and R in {1, 3}: 11 slices of K (10 in GRU's second phase), the smallest shape whose slab reduction runs a
    partial second batch of eight.  The two bias shapes alternate.  The figures are printed per tensor (run with -s)."""
    for n, (R, E, H) in enumerate(STEP_SHAPES):
        _step_case(kind, dt, R, E, H, bias2d=bool(n % 2))


def test_step_kernel_refuses_bad_arguments(gpu):
    dt = torch.float32
    E, H = 3, 5
    w = [to_sten(t.to(dt)) for t in _cell_weights("rnn", E, H, dt, True)]
    packed = TX.recurrentDecodePack(TX.RNN, w)
    table = to_sten(closed_form((7, E), 5, 2.0, dt))
    with pytest.raises(Exception, match="out of range"):                              # a token of 7 in a table of 7 rows
        h, _, _ = TX.recurrentDecodeStep(TX.RNN, table, to_sten(torch.tensor([1, 7])), packed, hPrev=S.STen.zeros([2, H], S.F32))
        h.to_numpy()
    h, _, _ = TX.recurrentDecodeStep(TX.RNN, table, to_sten(torch.tensor([1, 6])), packed, hPrev=S.STen.zeros([2, H], S.F32))
    assert np.isfinite(h.to_numpy()).all()                                            # the assertion word is clear again
    with pytest.raises(Exception, match="rows"):
        TX.recurrentDecodeStep(TX.RNN, table, to_sten(torch.zeros(17, dtype=torch.int64)), packed, hPrev=S.STen.zeros([17, H], S.F32))
    with pytest.raises(Exception, match="previous state"):
        hp, two = S.STen.zeros([2, H], S.F32), to_sten(torch.tensor([1, 2]))       # named: the handles live until the call returns
        lib.lamp_recurrent_decode_step(TX.RNN, table.h, two.h, None, packed[0].h, packed[1].h, None, hp.h, None, hp.h, None, None)


# ---- lamp_log_softmax_argmax_rows -----------------------------------------------------------------------------------------------------------
def _argmax(t):
    o = C.c_void_p(); lib.lamp_argmax(C.byref(o), t.h, 1, 0); return S.STen(o).to_numpy()


def _log_softmax(t):
    o = C.c_void_p(); lib.lamp_log_softmax(C.byref(o), t.h, 1); return S.STen(o)


@DTS
@pytest.mark.parametrize("R", [1, 16])
@pytest.mark.parametrize("V", [1, 7, 64, 257, 5000])
def test_log_softmax_argmax_rows(gpu, V, R, dt):
    x = closed_form((R, V), 3, 8.0, dt)
    out, tok = TX.logSoftMaxArgmaxRows(to_sten(x))
    got = to_torch(out)
    assert_close(got, torch.log_softmax(x.double(), 1), FWD_TOL[dt], f"log_softmax_argmax_rows {R}x{V}")
    assert np.array_equal(tok.to_numpy(), np.argmax(got.numpy(), axis=1)), "the token is the first argmax of the stored row"
    # without the log-softmax the logits pass through
    out, tok = TX.logSoftMaxArgmaxRows(to_sten(x), logSoftMax=False)
    assert torch.equal(to_torch(out), x) and np.array_equal(tok.to_numpy(), np.argmax(x.numpy(), axis=1))
    # strided destinations: a time step of [3, R, V] and of [3, R], then a column of [R, 3]
    steps, toks = S.STen.zeros([3, R, V], TORCH2LAMP[dt]), S.STen.zeros([3, R], S.I64)
    TX.logSoftMaxArgmaxRows(to_sten(x), out=steps.select(0, 1), tokens=toks.select(0, 1))
    assert torch.equal(to_torch(steps)[1], got) and np.array_equal(toks.to_numpy()[1], np.argmax(got.numpy(), axis=1))
    assert not to_torch(steps)[0].any() and not to_torch(steps)[2].any() and not toks.to_numpy()[[0, 2]].any()
    cols = S.STen.zeros([R, 3], S.I64)
    TX.logSoftMaxArgmaxRows(to_sten(x), tokens=cols.select(1, 2))
    assert np.array_equal(cols.to_numpy()[:, 2], np.argmax(got.numpy(), axis=1)) and not cols.to_numpy()[:, :2].any()


@DTS
def test_log_softmax_argmax_rows_ties_and_nan(gpu, dt):
    x = closed_form((4, 9), 3, 2.0, dt)
    x[0, 2] = 7.0; x[0, 5] = 7.0                         # the maximum twice: the lower index
    x[1, :] = 0.25                                       # all equal: 0
    x[2, 4] = float("nan")
    for lsm in (True, False):
        out, tok = TX.logSoftMaxArgmaxRows(to_sten(x), logSoftMax=lsm)
        stored = _log_softmax(to_sten(x)) if lsm else to_sten(x)
        assert tok.to_numpy()[0] == 2 and tok.to_numpy()[1] == 0
        assert np.array_equal(tok.to_numpy(), _argmax(stored)), "a row with a NaN gives what lamp_argmax gives for it"
        assert np.array_equal(np.isnan(out.to_numpy()), np.isnan(stored.to_numpy()))


# ---- sequencePrediction ---------------------------------------------------------------------------------------------------------------------
def _params(kind, V, E, H, dt, salt=0, lin_scale=1.0):
    p = [closed_form((V, E), salt + 5, 2.0, F64)] + _cell_weights(kind, E, H, dt, True, salt)
    p += [closed_form((H, V), salt + 17, lin_scale * 4.0 / (H + V) ** 0.5, F64), closed_form((1, V), salt + 19, 0.5, F64)]
    return [t.to(dt).to(F64) for t in p]


def _model(kind, params, dt, relu=True, lsm=True, cells=1):
    V, E = params[0].shape
    H = params[-2].shape[0]
    ldt = TORCH2LAMP[dt]
    mods = [TF.Embedding(V, E, ldt, 0), MODULE[kind](E, H, ldt, 0)] + [MODULE[kind](H, H, ldt, 0) for _ in range(cells - 1)]
    mods += ([nn.Fun("relu")] if relu else []) + [RC.SeqLinear(H, V, ldt, 0)] + ([nn.Fun("logsoftmax", 2)] if lsm else [])
    m = RC.statefulSequence(*mods)
    if cells == 1:
        m.load([to_sten(t.to(dt)) for t in params])
    return m


def _teacher_forced(forward, prefix, tokens, steps):
    """the restatement over prefix + generated tokens: the outputs the library's step i should have produced"""
    full = torch.cat([prefix, tokens[:-1]], 0)
    out, _ = forward(full, None)
    return out[prefix.shape[0] - 1:]


@DTS
@KINDS
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
def test_sequence_prediction_fused_and_chain(gpu, kind, dt, relu):
    """V = 19, E = 6, H = 33, 12 steps, prefixes of 1 and 4 tokens, 1 and 3 rows.  Every step's outputs against the restatement run over the
    prefix and the generated tokens; e_c is the chain's error over all steps, every fused step is held to 4 e_c + 64 eps."""
    V, E, H, steps = 19, 6, 33, 12
    params = _params(kind, V, E, H, dt)
    forward = TR.model_forward(kind, params, relu=relu)
    m = _model(kind, params, dt, relu=relu)
    floor = FLOOR_EPS * EPS[dt]
    for T0, B in ((1, 1), (4, 3), (1, 3), (4, 1)):
        prefix = (torch.arange(T0 * B).reshape(T0, B) * 5 + 2) % V
        res = {}
        for fused in (False, True):
            prev = TX.textGenerationFused(fused)
            try:
                tokens, outputs = TX.sequencePrediction(to_sten(prefix), 0, m, steps, returnOutputs=True)
                assert TX.textGeneratePath() == ("fused" if fused else "chain")
                if fused:
                    again, outputs2 = TX.sequencePrediction(to_sten(prefix), 0, m, steps, returnOutputs=True)
                    assert torch.equal(to_torch(again), to_torch(tokens)) and torch.equal(to_torch(outputs2), to_torch(outputs)), "two fused runs"
            finally:
                TX.textGenerationFused(prev)
            tokens, outputs = to_torch(tokens), to_torch(outputs)
            assert list(tokens.shape) == [steps, B] and list(outputs.shape) == [steps, B, V] and tokens.dtype == torch.int64
            assert np.array_equal(tokens.numpy(), np.argmax(outputs.numpy(), axis=2)), "tokens = first argmax of the library's own outputs"
            ref = _teacher_forced(forward, prefix, tokens, steps)
            res[fused] = [_err(outputs[i], ref[i]) for i in range(steps)]
        e_c = max(res[False])
        print(f"{kind} {dt} relu={relu} T0={T0} B={B}: e_c {e_c:.3e} e_f {max(res[True]):.3e} (floor {floor:.1e})")
        for i, e_f in enumerate(res[True]):
            assert e_f <= 4 * e_c + floor, f"step {i}: fused error {e_f:.3e} > 4 * chain error {e_c:.3e} + {floor:.1e}"


def test_sequence_prediction_chain_takes_over(gpu):
    V, E, H, steps = 19, 6, 33, 5
    dt = torch.float32
    params = _params("lstm", V, E, H, dt)

    def run(m, B):
        prefix = (torch.arange(2 * B).reshape(2, B) * 5 + 2) % V
        tokens, outputs = TX.sequencePrediction(to_sten(prefix), 0, m, steps, returnOutputs=True)
        assert list(tokens.shape) == [steps, B]
        assert np.array_equal(tokens.to_numpy(), np.argmax(to_torch(outputs).float().numpy(), axis=2))
        return TX.textGeneratePath()

    m = _model("lstm", params, dt)
    assert run(m, 16) == "fused"
    assert run(m, 17) == "chain"                                             # more rows than the decode kernels take
    assert run(_model("lstm", params, dt, cells=2), 2) == "chain"            # a two-cell stack
    assert run(_model("lstm", params, torch.bfloat16, cells=1), 2) == "chain"
    prev = TX.textGenerationFused(False)
    try:
        assert run(m, 2) == "chain"
    finally:
        TX.textGenerationFused(prev)
    assert run(m, 2) == "fused"


@pytest.mark.parametrize("kind,per_token", [("rnn", 3), ("lstm", 3), ("gru", 4)])
def test_sequence_prediction_launch_budget(gpu, kind, per_token):
    """between 4 and 12 steps the tagged launches grow by at most 3 per token (GRU 4) plus one to spare, the step kernel's class ran exactly
    steps - 1 times, and the chain grows by more"""
    V, E, H, dt = 19, 6, 33, torch.float32
    m = _model(kind, _params(kind, V, E, H, dt), dt)
    prefix = to_sten((torch.arange(6).reshape(2, 3) * 5 + 2) % V)
    totals = {}
    for fused in (True, False):
        prev = TX.textGenerationFused(fused)
        try:
            for steps in (4, 12):
                counts = _timer_counts(lambda: TX.sequencePrediction(prefix, 0, m, steps))
                totals[(fused, steps)] = sum(counts.values())
                if fused:
                    assert counts.get("recurrent_decode_step", 0) == steps - 1, counts
                    assert counts.get("recurrent_decode_gru_out", 0) == (steps - 1 if kind == "gru" else 0), counts
                    assert counts.get("recurrent_decode_pack", 0) == 1, counts
                else:
                    assert not any(c.startswith("recurrent_decode") for c in counts), counts
        finally:
            TX.textGenerationFused(prev)
    grow_f, grow_c = totals[(True, 12)] - totals[(True, 4)], totals[(False, 12)] - totals[(False, 4)]
    print(f"{kind}: tagged launches fused {totals[(True, 4)]} -> {totals[(True, 12)]}, chain {totals[(False, 4)]} -> {totals[(False, 12)]}")
    assert grow_f <= (per_token + 1) * 8, f"{kind}: {grow_f} more launches for 8 more tokens, the budget is {per_token} + 1 per token"
    assert grow_c > grow_f, f"{kind}: the chain grew by {grow_c}, the fused path by {grow_f}"


# ---- FreeRunningRNN, Seq2Seq, WithInit as modules -------------------------------------------------------------------------------------------
def test_free_running_rnn_module_gradients(gpu):
    """the reference's test shape (nn.test.scala:552-573): [2, 3] int64 input, table [7, 4], RNN 4 -> 4, three steps, f64; sum(outputs) and
    every parameter gradient against torch autograd on the restatement"""
    table = closed_form((7, 4), 5, 2.0, F64)
    w = _cell_weights("rnn", 4, 4, F64, True)
    x = torch.tensor([[1, 6, 0], [3, 3, 5]], dtype=torch.int64)
    ps = [t.clone().requires_grad_(True) for t in [table] + w]

    def forward(tokens, state):
        return TR.cell_forward("rnn", TR.embedding(tokens, ps[0]), ps[1:], state)
    ref, ref_state = TR.free_running(forward, x, None, 3)
    ref.sum().backward()
    emb = TF.Embedding(7, 4, S.F64, 0)
    inner = RC.statefulSequence(emb, RC.RNN(tensors=[to_sten(t) for t in w]))
    inner.state[0].value.copyFrom(to_sten(table))
    free = RC.FreeRunningRNN(inner, 3)
    assert free.stateSlots == 1 and free.initState is None
    assert [tuple(v.value.shape) for v in free.state] == [(7, 4), (4, 4), (4, 4), (1, 4)]          # the wrapped module's, in its order
    out, state = free.forward(A.const(to_sten(x)), None)
    assert list(out.value.shape) == [3, 3, 4] and len(state) == 1
    total = out.sum()
    total.backprop()
    assert abs(to_torch(total.value).item() - ref.sum().item()) <= 1e-12 * abs(ref.sum().item())
    assert _err(to_torch(out.value), ref.detach()) < 1e-12 and _err(to_torch(state[0].value), ref_state[0].detach()) < 1e-12
    for k, p in enumerate(free.state):
        assert _err(to_torch(p.partialDerivative), ps[k].grad) < 1e-12, f"state tensor {k}"


def test_seq2seq_and_with_init(gpu):
    """encoder Embedding -> LSTM (T = 4), decoder Embedding -> LSTM -> SeqLinear (T = 3), B = 2, f64: the output is the two-call composition,
    the encoder's parameters receive through the state the gradient the restatement gives, state = encoder.state ++ decoder.state"""
    V, E, H = 7, 3, 5
    pe = [closed_form((V, E), 5, 2.0, F64)] + _cell_weights("lstm", E, H, F64, True, salt=1)
    pd = [closed_form((V, E), 9, 2.0, F64)] + _cell_weights("lstm", E, H, F64, True, salt=2) + \
         [closed_form((H, V), 17, 1.0, F64), closed_form((1, V), 19, 0.5, F64)]
    source = torch.tensor([[1, 6], [0, 2], [3, 3], [5, 4]], dtype=torch.int64)
    dest = torch.tensor([[2, 2], [6, 0], [1, 4]], dtype=torch.int64)
    L = closed_form((3, 2, V), 301, 1.0, F64)
    re, rd = [t.clone().requires_grad_(True) for t in pe], [t.clone().requires_grad_(True) for t in pd]
    enc_ref = lambda x, st: TR.cell_forward("lstm", TR.embedding(x, re[0]), re[1:], st)
    dec_ref = TR.model_forward("lstm", rd, relu=False, log_softmax=False)
    ref, _ = TR.seq2seq(enc_ref, dec_ref, source, dest, None)
    (ref * L).sum().backward()

    enc = RC.statefulSequence(TF.Embedding(V, E, S.F64, 0), RC.LSTM(E, H, S.F64, 0))
    dec = RC.statefulSequence(TF.Embedding(V, E, S.F64, 0), RC.LSTM(E, H, S.F64, 0), RC.SeqLinear(H, V, S.F64, 0))
    enc.load([to_sten(t) for t in pe]); dec.load([to_sten(t) for t in pd])
    s2s = RC.Seq2Seq(enc, dec)
    assert s2s.stateSlots == 2 and s2s.initState is None
    assert [tuple(v.value.shape) for v in s2s.state] == [tuple(t.shape) for t in pe + pd], "state = encoder.state ++ decoder.state"
    out, state = s2s.forward((A.const(to_sten(source)), A.const(to_sten(dest))), None)
    _, es = enc.forward(A.const(to_sten(source)), None)
    two, ds = dec.forward(A.const(to_sten(dest)), list(es))
    assert torch.equal(to_torch(out.value), to_torch(two.value)) and all(torch.equal(to_torch(a.value), to_torch(b.value)) for a, b in zip(state, ds))
    assert _err(to_torch(out.value), ref.detach()) < 1e-12
    s2s.zeroGrad()
    (out * A.const(to_sten(L))).sum().backprop()
    for k, p in enumerate(s2s.state):
        want = (re + rd)[k].grad
        assert _err(to_torch(p.partialDerivative), want) < 1e-12, f"state tensor {k} ({'encoder' if k < len(pe) else 'decoder'})"
    # WithInit supplies its state: to its own forward through initState, and to sequencePrediction
    init = [closed_form((2, H), 201 + k, 1.0, F64) for k in range(2)]
    wi = RC.WithInit(dec, [A.const(to_sten(t)) for t in init])
    assert wi.stateSlots == 2 and all(torch.equal(to_torch(v.value), t) for v, t in zip(wi.initState, init))
    assert [tuple(v.value.shape) for v in wi.state] == [tuple(t.shape) for t in pd]
    a, _ = wi.forward(A.const(to_sten(dest)), wi.initState)
    b, _ = dec_ref(dest, tuple(init))
    assert _err(to_torch(a.value), b.detach()) < 1e-12
    for fused in (False, True):
        prev = TX.textGenerationFused(fused)
        try:
            tokens, outputs = TX.sequencePrediction(to_sten(dest), 0, wi, 4, returnOutputs=True)
            assert TX.textGeneratePath() == ("fused" if fused else "chain")
        finally:
            TX.textGenerationFused(prev)
        want = _teacher_forced(lambda x, st: dec_ref(x, tuple(init) if st is None else st), dest, to_torch(tokens), 4)
        assert _err(to_torch(outputs), want.detach()) < 1e-12, f"sequencePrediction from WithInit's state, fused={fused}"


# ---- beam -----------------------------------------------------------------------------------------------------------------------------------
# closed-form salts (and an output layer four times the usual scale) under which the restatement's runs keep the candidates apart: the
# smallest gap over the largest |log-probability| is 1.2e-2 (rnn, gru) and 3.6e-3 (lstm), found on the CPU over salts 0 .. 59
BEAM_SALT = {"rnn": 8, "gru": 14, "lstm": 25}
START = -5                                                   # a start-of-sequence marker that is no token


@DTS
@KINDS
@pytest.mark.parametrize("early_end", [False, True], ids=["open", "early_end"])
def test_sequence_prediction_beam(gpu, kind, dt, early_end):
    """V = 11, H = 16, k = 3, 8 steps: the sequences equal the restatement's, the log-probabilities obey the rule.  The inputs are such that at
    every step of the restatement's run the k-th and the (k + 1)-th candidate, and at the last step the k best among themselves, are at
    least 100 times the rule's bound apart (asserted), so rounding can change neither the beams nor their order.  early_end: the end token is the one the restatement ranks third after two steps, so a beam finishes
    there and is carried."""
    V, E, H, k, steps = 11, 5, 16, 3, 8
    params = _params(kind, V, E, H, dt, salt=BEAM_SALT[kind], lin_scale=4.0)
    forward = TR.model_forward(kind, params)
    prefix = [4, 9, 1]
    eos = -1
    if early_end:
        eos = int(TR.beam(forward, prefix, None, 2, START, -1, k)[2][0][-1])
    trace = []
    ref = TR.beam(forward, prefix, None, steps, START, eos, k, trace=trace)
    if early_end:
        assert min(len(t) for t, _ in ref) < steps + 1, "no beam ended early"
    m = _model(kind, params, dt)
    got = {}
    for fused in (False, True):
        prev = TX.textGenerationFused(fused)
        try:
            counts = _timer_counts(lambda: got.__setitem__(fused, TX.sequencePredictionBeam(prefix, 0, m, steps, START, eos, k)))
            assert TX.textGeneratePath() == ("fused" if fused else "chain")
            if fused:
                half = _timer_counts(lambda: TX.sequencePredictionBeam(prefix, 0, m, steps // 2, START, eos, k))
                per_step = (sum(counts.values()) - sum(half.values())) / (steps - steps // 2)
                # step (GRU 2), logits, log-softmax, top-k and the pack of its [rows, 2 k] read: a constant, where a read per entry is rows * V
                print(f"beam {kind}: {per_step} tagged launches per step")
                assert per_step <= 16 < k * V, counts
        finally:
            TX.textGenerationFused(prev)
    scale = max(abs(lp) for _, lp in ref)
    e = {f: max(abs(lp - rlp) for (_, lp), (_, rlp) in zip(got[f], ref)) / scale for f in got if len(got[f]) == len(ref)}
    bound = 4 * e.get(False, 0.0) + FLOOR_EPS * EPS[dt]
    gap = min([c[k - 1] - c[k] for c in trace if len(c) > k] + [trace[-1][i] - trace[-1][i + 1] for i in range(k - 1)])
    print(f"beam {kind} {dt}: e_c {e.get(False)} e_f {e.get(True)} bound {bound:.3e}, smallest gap {gap:.3e} over a scale of {scale:.3f}")
    assert gap >= 100 * bound * scale, f"the inputs leave a gap of {gap:.3e} between candidates, less than 100 x the bound {bound * scale:.3e}"
    for fused in (False, True):
        assert [t.tolist() for t, _ in got[fused]] == [t.tolist() for t, _ in ref], f"fused={fused}: sequences"
        assert all(t.dtype == np.int64 and t[0] == prefix[-1] and len(t) <= steps + 1 for t, _ in got[fused])
    assert e[True] <= bound, f"fused log-probabilities off by {e[True]:.3e} > 4 * chain {e[False]:.3e} + floor"
