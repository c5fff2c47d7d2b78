"""RAdam and Yogi through the public interface on the GPU (and, staged, on the CPU device) against the restatement of tests/optim_ref.py:
the reference's known answers, every form of the multi-tensor descriptor, Yogi's discrete cases, half-precision storage, clipping,
the state round trip, rejected arguments and the convolutions' re-pack hook."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from lamp_amd import nn
from lamp_amd import sten as S
from lamp_amd._capi import LampError, f64_array, handle_array, lib
from tests import optim_ref as R
from tests.util import assert_close, to_sten, to_torch

pytestmark = pytest.mark.gpu

KINDS = {"radam": (nn.RAdam, R.RAdam), "yogi": (nn.Yogi, R.Yogi)}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def moments(opt, n):
    st = opt.state
    assert len(st) == 1 + 2 * n
    return st[1:1 + n], st[1 + n:]


# ---- 1. the reference's known answers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [0, S.CPU], ids=["gpu", "cpu-device"])
def test_radam_kat(gpu, device):
    k = R.KATS["radam"]
    p = S.STen.from_numpy(np.array([k["init"]]), device, S.F64)
    g = S.STen.from_numpy(np.array([k["gradients"]]), device, S.F64)
    opt = nn.RAdam([p], weightDecay=k["weightDecay"], learningRate=k["learningRate"], beta1=k["beta1"], beta2=k["beta2"])
    for step in ("step1", "step2"):
        opt.step([g], 1.0)
        assert p.device == device
        np.testing.assert_allclose(p.to_numpy()[0], k[step], rtol=1e-14, atol=0)
    assert g.to_numpy()[0].tolist() == k["gradients"], "RAdam only reads its gradients"
    assert opt.state[0].to_numpy() == 2.0


@pytest.mark.parametrize("device", [0, S.CPU], ids=["gpu", "cpu-device"])
def test_yogi_kat_steps_twice_on_one_gradient_tensor(gpu, device):
    k = R.KATS["yogi"]
    p = S.STen.from_numpy(np.array([k["init"]]), device, S.F64)
    g = S.STen.from_numpy(np.array([k["gradients"]]), device, S.F64)
    opt = nn.Yogi([p], weightDecay=k["weightDecay"], learningRate=k["learningRate"], beta1=k["beta1"], beta2=k["beta2"])
    opt.step([g], 1.0)
    assert np.array_equal(np.round(p.to_numpy()[0], 4), np.round(k["step1"], 4))
    assert g.device == device and g.to_numpy()[0].tolist() == k["gradients_after_step1"], "Yogi writes g*g*sign(v - g*g) back"
    opt.step([g], 1.0)
    assert np.array_equal(np.round(p.to_numpy()[0], 4), np.round(k["step2"], 4))
    assert opt.state[0].to_numpy() == 2.0


# ---- 2. every form of the descriptor ---------------------------------------------------------------------------------------------
# 46 tensors > MT_MAX = 40: two groups per launch; 1025 and 2049 put a chunk boundary inside a tensor; 1, 3 and 7 are tails shorter
# than a 16-byte packet; two tensors with beta2 = 0.5 are never rectified, so from step 5 on both RAdam branches occur in one call
SIZES = [1, 7, 1024, 1025, 2049] + [3] * 41
HALF_B2 = (3, 10)
NONE_AT = 20
STEPS = 8
SEED = 2
HYPER = dict(weightDecay=0.05, learningRate=0.01, beta1=0.9, beta2=[0.5 if i in HALF_B2 else 0.999 for i in range(len(SIZES))])


@functools.lru_cache(maxsize=None)
def descriptor_inputs():
    """f32-representable parameters and per-step gradients (seeded normal, every 97th element zero, one tensor's gradient None)"""
    gen = torch.Generator().manual_seed(SEED)
    params = [torch.randn(n, generator=gen, dtype=torch.float32) for n in SIZES]
    steps = []
    for _ in range(STEPS):
        flat = torch.randn(sum(SIZES), generator=gen, dtype=torch.float32)
        flat[::97] = 0.0
        gs = list(torch.split(flat, SIZES))
        gs[NONE_AT] = None
        steps.append(gs)
    return params, steps


@functools.lru_cache(maxsize=None)
def restated_trajectory(kind, dt):
    """[(p, m, v) lists after each step] of the restatement run in dtype dt on the shared inputs"""
    params0, steps = descriptor_inputs()
    ps = [p.to(dt).clone() for p in params0]
    opt = KINDS[kind][1](ps, **HYPER)
    out = []
    for gs in steps:
        opt.step([None if g is None else g.to(dt).clone() for g in gs], 1.0)
        out.append(([p.clone() for p in ps], [m.clone() for m in opt.mt], [v.clone() for v in opt.vt]))
    return out


def kernel_trajectory(kind, dt):
    params0, steps = descriptor_inputs()
    ps = [to_sten(p.to(dt)) for p in params0]
    opt = KINDS[kind][0](ps, **HYPER)
    out = []
    for gs in steps:
        opt.step([None if g is None else to_sten(g.to(dt)) for g in gs], 1.0)
        ms, vs = moments(opt, len(ps))
        out.append(([to_torch(p) for p in ps], [to_torch(m) for m in ms], [to_torch(v) for v in vs]))
    return out


def distances(traj, ref):
    """largest absolute distance per state kind (p, m, v) over all steps and tensors"""
    return [max(float((a.double() - b).abs().max()) for s, r in zip(traj, ref) for a, b in zip(s[k], r[k])) for k in range(3)]


@pytest.mark.parametrize("kind", ["radam", "yogi"])
def test_descriptor_forms_f64(gpu, kind):
    ref = restated_trajectory(kind, torch.float64)
    got = kernel_trajectory(kind, torch.float64)
    print(f"{kind} f64: largest distances (p, m, v) {distances(got, ref)}")
    params0, _ = descriptor_inputs()
    for step, (s, r) in enumerate(zip(got, ref)):
        for k, what in enumerate("pmv"):
            for i, (a, b) in enumerate(zip(s[k], r[k])):
                np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-14, atol=1e-14 * float(b.abs().max()),
                                           err_msg=f"{what}[{i}] after step {step + 1}")
        assert torch.equal(bits(s[0][NONE_AT]), bits(params0[NONE_AT].double())), "a parameter without a gradient moved"
        assert not s[1][NONE_AT].any() and not s[2][NONE_AT].any(), "moments of a parameter without a gradient moved"


@pytest.mark.parametrize("kind", ["radam", "yogi"])
def test_descriptor_forms_f32(gpu, kind):
    """No number fixed in advance: the kernel may be at most twice as far from the f64 restatement as the f32 restatement (the chain of
    rounded ATen calls) is on the same inputs - the kernel rounds in fewer places, the factor 2 covers contraction going either way.
    So that a flipped Yogi sign in the yardstick cannot loosen the bound, the f32 restatement itself must stay within 2^-20 of each
    tensor's largest magnitude (measured: about 2^-22)."""
    ref = restated_trajectory(kind, torch.float64)
    chain = restated_trajectory(kind, torch.float32)
    for s, r in zip(chain, ref):
        for k in range(3):
            for a, b in zip(s[k], r[k]):
                assert float((a.double() - b).abs().max()) <= 2.0 ** -20 * float(b.abs().max()), "the f32 yardstick itself is off: choose another seed"
    got = kernel_trajectory(kind, torch.float32)
    d_kernel, d_chain = distances(got, ref), distances(chain, ref)
    print(f"{kind} f32: kernel distances (p, m, v) {d_kernel}, f32 restatement {d_chain}")
    for what, dk, dc in zip("pmv", d_kernel, d_chain):
        assert dk <= 2 * dc, f"{what}: kernel {dk:.3e} from the f64 restatement, the f32 chain {dc:.3e}"
    params0, _ = descriptor_inputs()
    for s in got:
        assert torch.equal(bits(s[0][NONE_AT]), bits(params0[NONE_AT]))
        assert not s[1][NONE_AT].any() and not s[2][NONE_AT].any()


# ---- 3. Yogi's discrete cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_yogi_discrete_cases(gpu, dt):
    n = 1025
    gen = torch.Generator().manual_seed(5)
    g0 = torch.randn(n, generator=gen, dtype=dt)
    v0 = torch.rand(n, generator=gen, dtype=dt) + 0.5           # (1-b2) g*g <= 0.001 * 25 is far below it
    half = torch.arange(n) < n // 2
    v0[half] = (g0 * g0)[half]                           # v == g*g as rounded by torch: the contracted form would see a non-zero difference
    zero = (torch.arange(n) >= 600) & (torch.arange(n) < 650)
    g0[zero] = 0.0
    v0[zero] = 0.0
    m0 = torch.randn(n, generator=gen, dtype=dt)
    p0 = torch.randn(n, generator=gen, dtype=dt)
    still = half | zero
    if dt == torch.float32:
        assert int((g0[half].double() ** 2 != (g0 * g0)[half].double()).sum()) > n // 4, "the squares must be inexact for the case to bite"
    hyper = dict(weightDecay=0.01, learningRate=0.01, beta1=0.9, beta2=0.999)
    pr, gr = p0.clone(), g0.clone()
    ropt = R.Yogi([pr], **hyper)
    ropt.load([torch.tensor(3.0, dtype=torch.float64), m0, v0])
    ropt.step([gr], 1.0)
    ph, gh = to_sten(p0), to_sten(g0)
    hopt = nn.Yogi([ph], **hyper)
    hopt.load([S.STen.scalarDouble(3.0), to_sten(m0), to_sten(v0)])
    hopt.step([gh], 1.0)
    (m,), (v,) = moments(hopt, 1)
    v, gn = to_torch(v), to_torch(gh)
    assert torch.equal(bits(v[still]), bits(v0[still])), "v moved where v == g*g (or g == 0 and v == 0)"
    assert torch.equal(bits(gn), bits(gr)), "the gradient must hold g*g*sign(v - g*g)"
    assert torch.equal(gn[still], torch.zeros_like(gn[still]))
    # elsewhere v = v - (1-b2)*gn is rounded once (fused) or twice (the chain): the product's rounding is far below a unit in the last
    # place of v, so the two results are the same or neighbouring values - at most eps * |v| apart; 2 eps is asserted
    eps = torch.finfo(dt).eps
    assert float(((v - ropt.vt[0]).abs() / ropt.vt[0].abs().clamp_min(1e-30)).max()) <= 2 * eps
    assert float((v[~still] != v0[~still]).float().mean()) > 0.9, "the control elements must move (all but those with a tiny g)"
    assert hopt.state[0].to_numpy() == 4.0


# ---- 4. bf16 and f16 storage -------------------------------------------------------------------------------------------------------
def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> int:
    """distance in units in the last place between two tensors of one 16-bit type (sign-magnitude bits mapped onto a line)"""
    def line(t):
        i = bits(t).to(torch.int32)
        return torch.where(i >= 0, i, -(i & 0x7FFF))
    return int((line(a) - line(b)).abs().max())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("kind,count", [("radam", 0), ("radam", 7), ("yogi", 3)], ids=["radam-plain", "radam-rectified", "yogi"])
def test_half_precision_storage_is_one_rounding(gpu, kind, count, dt):
    """One step from a loaded non-zero state: the kernel computes in f32 and rounds each stored value once, so against the restatement
    run in f32 on the same (representable) inputs and rounded once, every element is within one unit in the last place - an f32 result
    whose own error (a few 2^-24) is far below the spacing (2^-8 / 2^-11) can only land on a neighbouring value."""
    sizes = [7, 1025]
    gen = torch.Generator().manual_seed(11)
    mk = lambda f: [f(n).to(dt) for n in sizes]
    p0 = mk(lambda n: torch.randn(n, generator=gen))
    g0 = mk(lambda n: torch.randn(n, generator=gen))
    m0 = mk(lambda n: torch.randn(n, generator=gen) * 0.5)
    v0 = mk(lambda n: torch.rand(n, generator=gen) + 0.25)
    hyper = dict(weightDecay=0.05, learningRate=0.01, beta1=0.9, beta2=0.999)
    assert kind != "radam" or R.radam_is_rectified(0.999, count + 1) == (count == 7)
    pr, gr = [p.float() for p in p0], [g.float() for g in g0]
    ropt = KINDS[kind][1](pr, **hyper)
    ropt.load([torch.tensor(float(count), dtype=torch.float64)] + [t.float() for t in m0 + v0])
    ropt.step(gr, 1.0)
    ph, gh = [to_sten(p) for p in p0], [to_sten(g) for g in g0]
    hopt = KINDS[kind][0](ph, **hyper)
    hopt.load([S.STen.scalarDouble(float(count))] + [to_sten(t) for t in m0 + v0])
    hopt.step(gh, 1.0)
    ms, vs = moments(hopt, len(sizes))
    assert ms[0].dtype == ph[0].dtype == to_sten(p0[0]).dtype, "no mixed-precision mode: the moments have the parameter's dtype"
    for what, got, ref in (("p", ph, pr), ("m", ms, ropt.mt), ("v", vs, ropt.vt), ("g", gh, gr)):
        for i, (a, b) in enumerate(zip(got, ref)):
            d = ulp_distance(to_torch(a).to(dt), b.to(dt))
            assert d <= 1, f"{what}[{i}]: {d} units in the last place"
    if kind == "radam":
        assert all(torch.equal(to_torch(a).to(dt), b) for a, b in zip(gh, g0))


# ---- 5. clip -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["radam", "yogi"])
def test_clip_is_clipping_then_the_plain_step(gpu, kind):
    sizes = [7, 1025, 2049]
    gen = torch.Generator().manual_seed(3)
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    g0 = [torch.randn(n, generator=gen) for n in sizes]
    assert float(sum((g * g).sum() for g in g0)) > 1.0
    hyper = dict(weightDecay=0.05, learningRate=0.01, beta1=0.9, beta2=0.999)
    pa, ga = [to_sten(p) for p in p0], [to_sten(g) for g in g0]
    pb, gb = [to_sten(p) for p in p0], [to_sten(g) for g in g0]
    oa = KINDS[kind][0](pa, clip=1.0, **hyper)
    ob = KINDS[kind][0](pb, **hyper)
    oa.step(ga, 1.0)
    nn.gradientClippingInPlace(gb, 1.0)
    ob.step(gb, 1.0)
    for a, b in zip(pa + oa.state + ga, pb + ob.state + gb):
        assert torch.equal(bits(to_torch(a)), bits(to_torch(b)))
    assert not torch.equal(to_torch(ga[1]), g0[1]), "the gradients are clipped in place"


# ---- 6. state round trip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["radam", "yogi"])
def test_state_round_trip(gpu, kind):
    """3 steps, state -> a fresh optimiser's load, 3 more == 6 steps straight, bitwise.  RAdam changes branch at step 5: a step count
    lost in the round trip would leave the second half unrectified."""
    sizes = [7, 1025]
    gen = torch.Generator().manual_seed(9)
    p0 = [torch.randn(n, generator=gen, dtype=torch.float64) for n in sizes]
    gs = [[torch.randn(n, generator=gen, dtype=torch.float64) for n in sizes] for _ in range(6)]
    hyper = dict(weightDecay=0.05, learningRate=0.01, beta1=0.9, beta2=0.999)
    make = KINDS[kind][0]
    pa = [to_sten(p) for p in p0]
    oa = make(pa, **hyper)
    for g in gs:
        oa.step([to_sten(x) for x in g], 1.0)
    pb = [to_sten(p) for p in p0]
    ob = make(pb, **hyper)
    ob.step([to_sten(x) for x in gs[0]], 1.0)
    # the order is [count] + m... + v...: after one step from zero moments m = (1-b1) g and v = (1-b2) g*g for both optimisers
    st = ob.state
    assert len(st) == 1 + 2 * len(sizes) and st[0].dtype == S.F64 and st[0].to_numpy() == 1.0
    for i, g in enumerate(gs[0]):
        np.testing.assert_allclose(to_torch(st[1 + i]).numpy(), ((1 - 0.9) * g).numpy(), rtol=1e-12)
        np.testing.assert_allclose(to_torch(st[1 + len(sizes) + i]).numpy(), ((1 - 0.999) * g * g).numpy(), rtol=1e-12)
    for g in gs[1:3]:
        ob.step([to_sten(x) for x in g], 1.0)
    saved = [t.clone() for t in ob.state]
    assert saved[0].to_numpy() == 3.0
    pc = [p.clone() for p in pb]
    oc = make(pc, **hyper)
    oc.load(saved)
    for g in gs[3:]:
        oc.step([to_sten(x) for x in g], 1.0)
    assert oc.state[0].to_numpy() == 6.0
    for a, c in zip(pa + oa.state, pc + oc.state):
        assert torch.equal(bits(to_torch(a)), bits(to_torch(c)))


# ---- 7. rejected arguments -------------------------------------------------------------------------------------------------------------
def _raw_step(kind, p, g, m, v):
    n = len(p)
    arr = lambda x: f64_array([x] * n)
    args = [handle_array([t.h for t in ts]) for ts in (p, g, m, v)] + [n, arr(0.01), arr(0.05), arr(0.9), arr(0.999), 1e-8, 1.0, 1]
    if kind == "radam":
        lib.lamp_radam_step_(*args)
    else:
        lib.lamp_yogi_step_(*args, 1)


@pytest.mark.parametrize("kind", ["radam", "yogi"])
def test_bad_arguments_raise_and_write_nothing(gpu, kind):
    gen = torch.Generator().manual_seed(1)
    mk = lambda n, dt=torch.float32: torch.randn(n, generator=gen).to(dt)
    good = lambda: [to_sten(mk(1025)), to_sten(mk(7))]
    wrong = {
        "gradient dtype": lambda p, g, m, v: g.__setitem__(1, to_sten(mk(7, torch.float64))),
        "gradient size": lambda p, g, m, v: g.__setitem__(1, to_sten(mk(8))),
        "moment dtype": lambda p, g, m, v: m.__setitem__(1, to_sten(mk(7, torch.float64))),
        "moment size": lambda p, g, m, v: v.__setitem__(1, to_sten(mk(6))),
        "non-contiguous parameter": lambda p, g, m, v: p.__setitem__(1, to_sten(mk(14)).view(7, 2).select(1, 0)),
    }
    for what, spoil in wrong.items():
        p, g, m, v = good(), good(), good(), good()
        spoil(p, g, m, v)
        assert what != "non-contiguous parameter" or not p[1].is_contiguous()
        before = [to_torch(t).clone() for t in p + g + m + v]
        with pytest.raises(LampError):
            _raw_step(kind, p, g, m, v)
        for t, b in zip(p + g + m + v, before):
            assert torch.equal(bits(to_torch(t)), bits(b)), f"{what}: a rejected call wrote a tensor"
    # and through the optimiser: a gradient of another dtype or size
    p = good()
    opt = KINDS[kind][0](p, weightDecay=0.05)
    before = [to_torch(t).clone() for t in p]
    for bad in (to_sten(mk(7, torch.float64)), to_sten(mk(8))):
        with pytest.raises(LampError):
            opt.step([to_sten(mk(1025)), bad], 1.0)
    for t, b in zip(p + opt.state[1:], before + [torch.zeros_like(x) for x in before + before]):
        assert torch.equal(bits(to_torch(t)), bits(b))
    _raw_step(kind, good(), good(), good(), [to_sten(mk(1025).abs()), to_sten(mk(7).abs())])    # the well-formed call passes


# ---- 8. the re-pack hook ---------------------------------------------------------------------------------------------------------------
def _pack_counts():
    """{entries, pinned, hits, packs, repacked} of the packed-filter caches, summed over the backends (a debug export, not in the header)"""
    buf = (C.c_uint64 * 5)()
    lib.lamp_debug_pack_cache_counts(buf)
    return dict(zip(("entries", "pinned", "hits", "packs", "repacked"), (int(v) for v in buf)))


@pytest.mark.parametrize("kind", ["radam", "yogi"])
def test_replayed_resnet_step_tracks_the_weights(gpu, kind):
    """tests/test_autograd_gpu.py's test of the same name with RAdam / Yogi at f32, B = 8: forward + backprop captured once and replayed
    while the optimiser updates the weights eagerly between replays.  The convolutions' packed filter images follow an update only
    through the optimisers' re-pack hook, which writes them in place: the capture finds them current in the cache and records no pack
    launch, so a step that skipped the hook would leave the replayed graph reading stale filters."""
    from oracle import lamp_oracle as O
    B, ldt = 8, S.F32
    lib.lamp_manual_seed(77)
    em = nn.resnet(100, 0.0, ldt)
    gm = nn.resnet(100, 0.0, ldt)
    gm.load([v.value for v in em.state])
    cw = S.STen.ones([100], ldt)
    x = to_sten(O.closed_form(B * 3 * 32 * 32, 5, 1.0, torch.float32).reshape(B, 3, 32, 32))
    t = to_sten((torch.arange(B) * 7) % 100)
    emodel, gmodel = nn.SupervisedModel(em, nn.SupervisedModel.NLL, cw), nn.SupervisedModel(gm, nn.SupervisedModel.NLL, cw)
    factory = {"radam": nn.RAdam_factory, "yogi": nn.Yogi_factory}[kind](weightDecay=0.0, learningRate=1e-2)
    eopt, gopt = factory([p.value for p in em.parameters]), factory([p.value for p in gm.parameters])
    st = C.c_void_p(); lib.lamp_stream_get_from_pool(0, 0, C.byref(st)); lib.lamp_stream_set_current(st)
    try:
        for model, opt in ((emodel, eopt), (gmodel, gopt)):
            n, g1 = model.addTotalLossAndReturnGradientsAndNumExamples(x, t, None)
            opt.step(g1, 1.0)
        for _ in range(3):
            n, ge = emodel.addTotalLossAndReturnGradientsAndNumExamples(x, t, None)
            eopt.step(ge, 1.0)
        lib.lamp_device_synchronize()
        lib.lamp_graph_begin_capture()
        n, grads = gmodel.addTotalLossAndReturnGradientsAndNumExamples(x, t, None)
        g = C.c_void_p(); lib.lamp_graph_end_capture(C.byref(g))
        before = _pack_counts()
        for _ in range(3):
            lib.lamp_graph_launch(g)
            gopt.step(grads, 1.0)
        lib.lamp_device_synchronize()
        after = _pack_counts()
        assert after["packs"] == before["packs"], "a replay packs nothing: the capture found every image in its cache"
        assert after["repacked"] > before["repacked"], "the step must bring the cached images up to date (conv_repack_cached)"
        for i, (a, b) in enumerate(zip(gm.state, em.state)):
            assert_close(to_torch(a.value), to_torch(b.value).double(), 1e-6, f"state {i} after three replayed steps")
        lib.lamp_graph_release(g)
    finally:
        d = C.c_void_p(); lib.lamp_stream_get_default(0, C.byref(d)); lib.lamp_stream_set_current(d)
        lib.lamp_stream_release(st); lib.lamp_stream_release(d)
