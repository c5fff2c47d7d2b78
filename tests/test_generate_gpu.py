"""lamp.data.languagemodel on the GPU: the decode kernels against f64 torch, the sampler against sample_ref, autoregressiveInference
teacher-forced against the oracle's forward on both paths, the launch budget of the cached phase, determinism, the minibatch builder."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import lamp_oracle as O
from tests.generate_ref import cumulative_intervals, decode_attention_ref, decode_linear_ref, sample_ref, window_logits_ref
from tests.test_transformer import _lamp_dtype, _load, _oracle_lm
from tests.util import DTYPES, FWD_TOL, assert_close, closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu


def _L():
    import lamp_amd.languagemodel as L
    return L


def _hip():
    from lamp_amd import sten as S, transformer as TR
    return S, TR


# ---- lamp_decode_linear ---------------------------------------------------------------------------------------------------------------------------
DECORATIONS = ["plain", "ln", "ln_affine", "bias", "gelu", "mult_add", "all"]


def _linear_case(dt, R, K, N, transposed, what):
    x = closed_form((R, K), 3, 2.0, dt)
    w = closed_form((N, K) if transposed else (K, N), 11, 2.0 / K ** 0.5, dt)
    kw_t, kw_s = {}, {}

    def give(name, t):
        kw_t[name] = t; kw_s[name] = to_sten(t)
    if what in ("ln", "ln_affine", "all"):
        kw_t["layerNorm"] = kw_s["layerNorm"] = True
        kw_t["eps"] = kw_s["eps"] = 1e-5
    if what in ("ln_affine", "all"):
        give("lnScale", closed_form((K,), 5, 1.0, dt) + 1.0)
        give("lnBias", closed_form((K,), 7, 0.5, dt))
    if what in ("bias", "all"):
        give("bias", closed_form((1, N), 13, 1.0, dt))
    if what in ("gelu", "all"):
        kw_t["gelu"] = True; kw_s["act"] = _L().ACT_GELU
    if what in ("mult_add", "all"):
        give("scale", closed_form((N,), 17, 2.0, dt))
        give("residual", closed_form((R, N), 19, 2.0, dt))
    return x, w, kw_t, kw_s


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32", "bf16"])
@pytest.mark.parametrize("K,N", [(12, 36), (13, 19), (48, 12), (3072, 768)])
def test_decode_linear_matches_f64(gpu, dt, K, N):
    """every decoration alone and all together at 1, 3 and 16 rows, W as [K, N] and as [N, K]; (13, 19) has no packet anywhere, (3072, 768)
    is split over K; two calls give the same bits"""
    L = _L()
    for R in (1, 3, 16):
        for transposed in (False, True):
            for what in DECORATIONS:
                x, w, kw_t, kw_s = _linear_case(dt, R, K, N, transposed, what)
                ref = decode_linear_ref(x, w, transposed=transposed, **kw_t)
                sx, sw = to_sten(x), to_sten(w)
                got = to_torch(L.decodeLinear(sx, sw, transposed=transposed, **kw_s))
                assert_close(got, ref, FWD_TOL[dt] * 4, f"R={R} transposed={transposed} {what}")
                if what in ("plain", "all"):
                    again = to_torch(L.decodeLinear(sx, sw, transposed=transposed, **kw_s))
                    assert torch.equal(got, again), f"R={R} transposed={transposed} {what}: two calls differ"


def test_decode_linear_rejects_17_rows(gpu):
    L = _L()
    x, w = to_sten(closed_form((17, 12), 3, 1.0, torch.float32)), to_sten(closed_form((12, 36), 5, 1.0, torch.float32))
    with pytest.raises(Exception, match="rows"):
        L.decodeLinear(x, w)
    with pytest.raises(Exception):
        L.decodeLinear(to_sten(closed_form((2, 12), 3, 1.0, torch.float32)), w, scale=to_sten(closed_form((36,), 1, 1.0, torch.float32)))


# ---- lamp_decode_attention ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32", "bf16"])
@pytest.mark.parametrize("H,d", [(3, 4), (12, 64)])
def test_decode_attention_matches_f64(gpu, dt, H, d):
    """cache rows above t hold NaN before the call: the output is finite and right, row t of both caches is the new key / value bit for
    bit, every other row is as it was"""
    L = _L()
    Tmax = 384
    for R in (1, 5):
        kfull = closed_form((R, H, Tmax, d), 23, 2.0, dt)
        vfull = closed_form((R, H, Tmax, d), 29, 2.0, dt)
        qkv = closed_form((R, 3 * H * d), 31, 2.0, dt)
        for t in (0, 1, 7, 63, 64, 65, 383):
            kc, vc = kfull.clone(), vfull.clone()
            kc[:, :, t:] = float("nan"); vc[:, :, t:] = float("nan")
            ref, knew, vnew = decode_attention_ref(qkv, kc, vc, t, H)
            sk, sv = to_sten(kc), to_sten(vc)
            got = to_torch(L.decodeAttention(to_sten(qkv), sk, sv, t, H))
            assert bool(torch.isfinite(got).all()), f"R={R} t={t}: the output is not finite"
            assert_close(got, ref, FWD_TOL[dt] * 4, f"R={R} t={t}")
            for name, cache, before, new in (("kcache", sk, kc, knew), ("vcache", sv, vc, vnew)):
                want = before.double().clone()
                want[:, :, t] = new
                after = to_torch(cache).double()
                assert np.array_equal(after.numpy(), want.numpy(), equal_nan=True), f"R={R} t={t}: {name} is not the old cache with row t replaced"


# ---- lamp_sample_logits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32", "bf16"])
def test_sample_logits_equals_sample_ref(gpu, dt):
    """given uniforms at the midpoints of the reference's cumulative intervals the kernel returns the reference's index"""
    L = _L()
    S, _ = _hip()
    g = torch.Generator().manual_seed(11)
    for V in (1, 19, 256, 1000):
        for temperature in (0.5, 1.0, 2.0):
            for R in (1, 16):
                logits = (torch.randn(R, V, generator=g, dtype=torch.float64) * 2.0).to(dt)
                z = logits.double().numpy()
                u, want = [], []
                for r in range(R):
                    c = cumulative_intervals(z[r], temperature)
                    k = (r * 37 + 5) % V
                    lo = c[k - 1] if k > 0 else 0.0
                    # the running sums of up to 1000 terms carry errors of at most 1000 * 2^-53 = 1.1e-13 of the total
                    assert c[k] - lo > 1e-11, "the chosen category's interval is wider than the rounding of the running sums"
                    u.append((lo + c[k]) / 2.0); want.append(k)
                assert sample_ref(z, temperature, u).tolist() == want
                got = L.sampleLogits(to_sten(logits), temperature, S.STen.from_numpy(np.array(u, dtype=np.float64), dtype=S.F64)).to_numpy()
                assert got.dtype == np.int64 and got.tolist() == want, (V, temperature, R)


def test_sample_logits_own_generator(gpu):
    """the form and bounds of test_randperm_and_multinomial: 20000 identical rows in one launch"""
    L = _L()
    w = np.array([0.1, 1e-30, 0.3, 0.6])
    logits = to_sten(torch.log(torch.tensor(w, dtype=torch.float32)).repeat(20000, 1))
    L.manualSeed(1234)
    a = L.sampleLogits(logits, 1.0).to_numpy()
    b = L.sampleLogits(logits, 1.0).to_numpy()
    assert a.shape == (20000,) and a.dtype == np.int64
    for s in (a, b):
        f = np.bincount(s, minlength=4) / 20000.0
        assert np.abs(f - np.array([0.1, 0.0, 0.3, 0.6])).max() < 0.015, f
    assert not np.array_equal(a, b), "two consecutive calls drew the same numbers"
    L.manualSeed(1234)
    assert np.array_equal(L.sampleLogits(logits, 1.0).to_numpy(), a), "the same seed gives the same draws"


def test_sample_logits_raises_on_nan_and_checks_arguments(gpu):
    L = _L()
    bad = torch.zeros(3, 5, dtype=torch.float32); bad[1, 2] = float("nan")
    with pytest.raises(Exception, match="sample_logits"):
        L.sampleLogits(to_sten(bad), 1.0).to_numpy()
    inf = torch.zeros(2, 5, dtype=torch.float32); inf[0, 0] = float("inf")
    with pytest.raises(Exception, match="sample_logits"):
        L.sampleLogits(to_sten(inf), 1.0).to_numpy()
    with pytest.raises(Exception, match="temperature"):
        L.sampleLogits(to_sten(torch.zeros(2, 5)), 0.0)


def test_decode_embedding(gpu):
    L = _L()
    for dt in DTYPES:
        tw, pw = closed_form((19, 12), 3, 2.0, dt), closed_form((16, 12), 5, 2.0, dt)
        seq = torch.tensor([[3, 18, 0], [7, 1, 11]], dtype=torch.int64)
        column = to_sten(seq).select(1, 1)                                   # a strided column, as the generation loop passes it
        got = to_torch(L.decodeEmbedding(to_sten(tw), to_sten(pw), column, 9))
        assert_close(got, tw.double()[seq[:, 1]] + pw.double()[9], FWD_TOL[dt], "embedding")


# ---- autoregressiveInference ----------------------------------------------------------------------------------------------------------------------
def _models(dt, vocab=19, ctx=16, dim=12, heads=3, blocks=2):
    S, TR = _hip()
    om = _oracle_lm(vocab, ctx, dim, heads, blocks, dt, -1000)
    hm = TR.LanguageModelLoss(ctx, vocab, blocks, dim, dim // heads, heads, dim * 4, 0.0, -1000, _lamp_dtype(S, dt), 0)
    _load(hm, om, S, dt)
    return om, hm


def _check_teacher_forced(om, tokens, logits, P, block, tol):
    """every step's logits against the oracle's forward on the window the step saw"""
    B, total = tokens.shape
    assert logits.shape[0] == B and logits.shape[1] == total - P
    for b in range(B):
        for i in range(total - P):
            window = tokens[b, :P + i][-block:].tolist()
            assert_close(logits[b, i], window_logits_ref(om, window).double(), tol, f"row {b} step {i}")


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
def test_generate_teacher_forced_against_oracle(gpu, dt, fused):
    """the configuration of test_language_model_loss_matches_oracle; 3 + 20 tokens in a context of 16: 13 cached steps, then the window slides"""
    L = _L()
    om, hm = _models(dt)
    prefix = np.array([[3, 1, 4], [15, 9, 2]], dtype=np.int64)
    was = L.languageModelFused(fused)
    try:
        L.manualSeed(7)
        tokens, logits = L.autoregressiveInference(hm, 16, prefix, 20, 0.9, returnLogits=True)
    finally:
        L.languageModelFused(was)
    assert L.languageModelGeneratePath() == ("fused" if fused else "chain")
    assert isinstance(tokens, np.ndarray) and tokens.shape == (2, 23) and tokens.dtype == np.int64
    assert np.array_equal(tokens[:, :3], prefix) and tokens.min() >= 0 and tokens.max() < 19
    assert logits.shape == [2, 20, 19]
    _check_teacher_forced(om, tokens, to_torch(logits), 3, 16, 1e-10 if dt == torch.float64 else 1e-4)


def test_generate_bf16_error_against_the_chain(gpu):
    """the configuration of test_language_model_bf16_flash_path_matches_f32_oracle.  The project has no bf16 logits tolerance, so the chain's
    own error is the yardstick: on the windows of the fused run the existing forward's logits differ from the f32 oracle's by e_chain
    (largest difference over the largest logit), the fused path's by e_fused, and e_fused <= 2 e_chain: the same rounding points, another
    summation order."""
    L = _L()
    S, TR = _hip()
    from lamp_amd import autograd as A
    vocab, ctx, dim, heads, blocks = 32, 16, 128, 2, 2
    om = _oracle_lm(vocab, ctx, dim, heads, blocks, torch.float32, -1000)
    for v in om.state():
        v.value.copy_((v.value * (4.0 / v.value.shape[-1] ** 0.5)).bfloat16().float())
    hm = TR.LanguageModelLoss(ctx, vocab, blocks, dim, dim // heads, heads, dim * 4, 0.0, -1000, S.BF16, 0)
    _load(hm, om, S, torch.bfloat16)
    prefix = np.array([[3, 1, 4], [15, 9, 2]], dtype=np.int64)
    P, length = 3, 20
    was = L.languageModelFused(True)
    try:
        L.manualSeed(7)
        tokens, logits = L.autoregressiveInference(hm, ctx, prefix, length, 0.9, returnLogits=True)
    finally:
        L.languageModelFused(was)
    assert L.languageModelGeneratePath() == "fused"
    logits = to_torch(logits).double()
    e_fused = e_chain = c_fused = c_chain = 0.0               # over every step; over the cached steps 1 .. ctx - P alone
    for b in range(2):
        for i in range(length):
            window = tokens[b, :P + i][-ctx:].tolist()
            ref = window_logits_ref(om, window).double()
            w = len(window)
            _, chain = hm.languageModel(A.const(to_sten(torch.tensor([window]))), None, to_sten(torch.tensor([[w - 1]])))
            chain = to_torch(chain.value).double().reshape(-1)
            den = ref.abs().max().item()
            ef, ec = (logits[b, i] - ref).abs().max().item() / den, (chain - ref).abs().max().item() / den
            e_fused, e_chain = max(e_fused, ef), max(e_chain, ec)
            if 1 <= i <= ctx - P:
                c_fused, c_chain = max(c_fused, ef), max(c_chain, ec)
    print(f"bf16 logits against the f32 oracle: fused {e_fused:.4e}, chain {e_chain:.4e}; cached steps alone: fused {c_fused:.4e}, chain {c_chain:.4e}")
    assert e_chain > 0 and e_fused <= 2.0 * e_chain, (e_fused, e_chain)
    assert c_chain > 0 and c_fused <= 2.0 * c_chain, (c_fused, c_chain)


def test_generate_edges(gpu):
    L = _L()
    dt = torch.float32
    om, hm = _models(dt)
    # a prefix longer than the context, and one that fills it: no cached step, the window slides from the first token on
    for P in (20, 16):
        prefix = ((np.arange(2 * P).reshape(2, P) * 5 + 3) % 19).astype(np.int64)
        tokens, logits = L.autoregressiveInference(hm, 16, prefix, 3, 1.0, returnLogits=True)
        assert L.languageModelGeneratePath() == "fused" and tokens.shape == (2, P + 3) and np.array_equal(tokens[:, :P], prefix)
        _check_teacher_forced(om, tokens, to_torch(logits), P, 16, 1e-4)
    # a model block size below the position table
    tokens, logits = L.autoregressiveInference(hm, 5, np.array([[3, 1, 4]]), 6, 1.0, returnLogits=True)
    _check_teacher_forced(om, tokens, to_torch(logits), 3, 5, 1e-4)
    # a list in, a list out; length 0 returns the prefix
    out = L.autoregressiveInference(hm, 16, [3, 1, 4], 4, 1.0)
    assert isinstance(out, list) and len(out) == 7 and out[:3] == [3, 1, 4] and all(isinstance(t, int) and 0 <= t < 19 for t in out)
    assert L.autoregressiveInference(hm, 16, [3, 1, 4], 0, 1.0) == [3, 1, 4]
    # 17 rows are more than the decode kernels take: the chain runs
    prefix = ((np.arange(17 * 3).reshape(17, 3) * 7 + 1) % 19).astype(np.int64)
    tokens, logits = L.autoregressiveInference(hm, 16, prefix, 2, 1.0, returnLogits=True)
    assert L.languageModelGeneratePath() == "chain" and tokens.shape == (17, 5)
    _check_teacher_forced(om, tokens[:3], to_torch(logits)[:3], 3, 16, 1e-4)
    with pytest.raises(Exception, match="prefix"):
        L.autoregressiveInference(hm, 16, [], 4, 1.0)
    with pytest.raises(Exception, match="temperature"):
        L.autoregressiveInference(hm, 16, [3, 1, 4], 4, 0.0)
    with pytest.raises(Exception, match="modelBlockSize"):
        L.autoregressiveInference(hm, 17, [3, 1, 4], 4, 1.0)


def test_generate_with_attention_dropout_takes_the_chain(gpu):
    """the attention's dropout never leaves training mode (TrainingMode.identity, Transformer.scala:644-645), so a model that has one is
    not the cached path's to run; the chain is reproducible from the seed, and the module is in training mode again afterwards"""
    L = _L()
    S, TR = _hip()
    from lamp_amd import autograd as A
    hm = TR.LanguageModelModule(16, 19, 1, 12, 4, 3, 48, 0.5, S.F32, 0)
    x = A.const(to_sten(torch.tensor([[3, 1, 4, 1, 5]])))
    L.manualSeed(3); a = L.autoregressiveInference(hm, 16, [3, 1, 4], 5, 1.0, returnLogits=True)
    assert L.languageModelGeneratePath() == "chain"
    L.manualSeed(3); b = L.autoregressiveInference(hm, 16, [3, 1, 4], 5, 1.0, returnLogits=True)
    assert a[0] == b[0] and torch.equal(to_torch(a[1]), to_torch(b[1]))
    e1 = to_torch(hm.forward(x)[0].value); e2 = to_torch(hm.forward(x)[0].value)
    assert not torch.equal(e1, e2), "the module is no longer in training mode after a generation"


def _launch_counts():
    from lamp_amd._capi import lib
    buf = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_report(buf, len(buf))
    return {l.split()[0]: int(l.split()[1]) for l in buf.value.decode().splitlines() if l.strip()}


def test_generate_launch_budget(gpu):
    """cached phase: a token costs at most 5 launches per block + 4 (embedding, final norm + logits, sampler, one to spare)"""
    from lamp_amd._capi import lib
    L = _L()
    blocks = 2
    _, hm = _models(torch.float32, ctx=64, blocks=blocks)
    totals = []
    lib.lamp_kernel_timer_enable(1)
    try:
        for length in (4, 12):
            _launch_counts()
            L.manualSeed(5)
            L.autoregressiveInference(hm, 64, [3, 1, 4], length, 1.0, returnLogits=True)
            from lamp_amd import sten as S
            S.synchronize()
            counts = _launch_counts()
            totals.append(sum(counts.values()))
            assert counts.get("decode_attention") == blocks * (length - 1), counts
    finally:
        lib.lamp_kernel_timer_enable(0)
    per_token = (totals[1] - totals[0]) / 8.0
    assert 0 < per_token <= 5 * blocks + 4, (totals, per_token)


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32", "bf16"])
def test_generate_is_deterministic(gpu, dt):
    L = _L()
    dims = dict(vocab=32, ctx=16, dim=128, heads=2) if dt == torch.bfloat16 else {}
    _, hm = _models(dt, **dims)
    prefix = np.array([[3, 1, 4], [15, 9, 2]], dtype=np.int64)
    runs = []
    for _ in range(2):
        L.manualSeed(99)
        tokens, logits = L.autoregressiveInference(hm, 16, prefix, 20, 1.0, returnLogits=True)
        runs.append((tokens, to_torch(logits)))
    assert np.array_equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    L.manualSeed(100)
    other = L.autoregressiveInference(hm, 16, prefix, 20, 1.0)
    assert not np.array_equal(other, runs[0][0]), "another seed drew the same 40 tokens"


# ---- autoregressiveMinibatchesFromCorpus ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("createMaxLength", [True, False])
def test_minibatches_from_corpus(gpu, createMaxLength):
    L = _L()
    S, _ = _hip()
    corpus = S.STen.arange(0, 1000, 1, S.I32, 0)
    batches = list(L.autoregressiveMinibatchesFromCorpus(5, 4, corpus, 8, createMaxLength))
    assert len(batches) == 4
    starts = []
    for tokens, targets, maxLength in batches:
        t, g = tokens.to_numpy(), targets.to_numpy()
        assert t.shape == (5, 8) and t.dtype == np.int64 and g.shape == (5, 8) and g.dtype == np.int64 and tokens.device == 0
        assert np.array_equal(t, t[:, :1] + np.arange(8)[None, :]), "every row is a contiguous window"
        assert np.array_equal(g, t + 1)
        assert t[:, 0].min() >= 0 and t[:, 0].max() <= 990
        starts.extend(t[:, 0].tolist())
        if createMaxLength:
            assert np.array_equal(maxLength.to_numpy(), np.tile(np.arange(1, 9), (5, 1)))
        else:
            assert maxLength is None
    assert len(set(starts)) > 1
    # the shape SupervisedModel(LanguageModelLoss, IDENTITY).train_step takes
    from lamp_amd import nn
    _, TR = _hip()
    hm = TR.LanguageModelLoss(8, 1001, 1, 8, 4, 2, 16, 0.0, -1000, S.F32, 0)
    model = nn.SupervisedModel(hm, nn.SupervisedModel.IDENTITY)
    opt = nn.AdamW([p.value for p in hm.parameters], weightDecay=0.0, learningRate=1e-3)
    tokens, targets, _ = batches[0]
    assert model.train_step(opt, tokens, targets, S.STen.zeros([1], S.F32)) == 5
