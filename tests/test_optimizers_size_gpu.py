"""AdamW, SGDW, gradientClippingInPlace and the flat gradient bucket at size, on the pattern of tests/test_optimizers_gpu.py: 46 tensors
(two groups of the multi-tensor descriptor), chunk edges inside tensors, tails shorter than a 16-byte packet, one gradient None, per-tensor
hyperparameters, and every case in two layouts - each tensor its own allocation, or a contiguous view at an odd element offset of one
flat tensor (what a gradient is when it is a view of a bucket), with the flat tensor's elements outside the views checked bit for bit.
The references are the restatements of tests/optim_ref.py (f64, and f32 as the yardstick), math.fsum for the clipping norm, and torch's
IEEE f32 multiply and divide for the bucket.

What each mistake in optim.hip would turn red (read against the code, one per kernel form):
  `end = begin + MT_CHUNK - 1` in adamw_kernel or sgdw_kernel   element 1023 of every full chunk keeps its old value: the sentinel there
                                                                leaves m, v or the velocity at 0 - every *_descriptor_forms_* test
  no element loop after the packets in mt_update_chunk          nothing of a misaligned tensor moves - test_radam_yogi_misaligned_*
  `hi = a.n - 2` in mt_find                                     the last tensor of each group of 40 is never touched: every descriptor
                                                                test, the clipping sum (its two sentinels are 1.3 % of it), the bucket
  no `t++` walk in mt_sumsq_kernel or mt_clip_scale_kernel      only per_wg > 1 walks: tensor 1 and tensor 3's first chunk drop out of the sum
                                                                (1e-5 of the norm, bound 3e-6) - test_clipping_walks_several_chunks_per_workgroup
  the model copy written from the value before the update,      test_adamw_mixed_precision's bit-for-bit cast, after the first step
  or truncated instead of rounded to nearest even
  weight decay after the gradient step in sgdw_kernel           p differs by lr * wd * g, 1e-5 relative - test_sgdw_descriptor_forms_f64
  `sc < 1 ? sc : 1` alone for the clipping factor               a NaN norm clips by 1 - test_clipping_propagates_a_nan (what the file did before)
  `src[i] * (1 / div)` in mt_unflatten_kernel                   not the rounded quotient by 7 - test_bucket_flatten_and_unflatten_are_exactly_rounded"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from lamp_amd import nn
from lamp_amd import sten as S
from lamp_amd._capi import LampError, f64_array, handle_array, lib
from tests import optim_ref as R
from tests.test_optimizers_gpu import HYPER, KINDS, NONE_AT, SIZES, STEPS, bits, moments, ulp_distance
from tests.util import TORCH2LAMP, to_sten, to_torch

pytestmark = pytest.mark.gpu

N = len(SIZES)
SEED = 4                                               # chosen on the CPU: tests/test_optimizers.py checks what it has to satisfy
FILL = -77.0                                             # exact in f64, f32, f16 and bf16: what the flat tensor holds outside the views
FACTORS = [1.0, 1.0, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0]      # scheduleFactor per step
# the three large tensors differ from the rest in one hyperparameter each: a chunk handed to the wrong tensor's values shows
ADAMW_HYPER = dict(weightDecay=[0.0 if i in (2, 11) else 0.05 for i in range(N)], learningRate=[0.02 if i == 4 else 0.01 for i in range(N)],
                   beta1=0.9, beta2=[0.998 if i in (3, 10) else 0.999 for i in range(N)])
LAYOUTS = pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "misaligned"])
HALVES = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])


def sentinel_at(n):
    """a tensor's first and last element, and both sides of the first chunk edge where it has one"""
    return sorted({0, n - 1} | ({1023, 1024} & set(range(n))))


@functools.lru_cache(maxsize=None)
def size_inputs():
    """f32-representable parameters and per-step gradients: seeded normal, every 97th element zero, one tensor's gradient None, and sentinels
    at every tensor edge and chunk edge: magnitudes 7 .. 9 in steps of 1/16 (exact in bf16 and f16 too), so that a dropped or doubled edge
    element moves a sum or a moment by ~64.  A sentinel keeps its sign (its first moment does not cancel) and its magnitude varies by
    tensor, edge and step: the sentinels are the largest moments by far, and with ONE magnitude they would all walk one trajectory - the
    largest distance of a state kind, which the f32 rule compares, would be a sample of one."""
    gen = torch.Generator().manual_seed(SEED)
    params = [torch.randn(n, generator=gen, dtype=torch.float32) for n in SIZES]
    steps = []
    for s in range(STEPS):
        flat = torch.randn(sum(SIZES), generator=gen, dtype=torch.float32)
        flat[::97] = 0.0
        gs = [g.clone() for g in torch.split(flat, SIZES)]
        for i, g in enumerate(gs):
            for k, j in enumerate(sentinel_at(g.numel())):
                g[j] = (7.0 + (5 * i + 3 * k + 7 * s) % 33 / 16.0) * (1 if (i + k) % 2 == 0 else -1)
        gs[NONE_AT] = None
        steps.append(gs)
    return params, steps


# ---- the two layouts ------------------------------------------------------------------------------------------------------------------
def view_offsets(sizes, k):
    """element offsets [list][tensor] of k lists of tensors laid into one flat tensor as FILL t0 u0 FILL t1 u1 FILL ...: running offsets
    from element 1, one guard element after each of the first five tensors (the large ones), three at the end"""
    offs, off = [[] for _ in range(k)], 1
    for i, n in enumerate(sizes):
        for j in range(k):
            offs[j].append(off)
            off += n
        if i < 5:
            off += 1
    return offs, off + 3


class Layout:
    """k lists of same-sized device tensors of dtype dt.  aligned: each its own allocation.  misaligned: contiguous 1-d narrow views of
    ONE flat tensor, filled with FILL first; get() checks that everything outside the views that were written still holds FILL."""

    def __init__(self, sizes, k, dt, misaligned):
        self.sizes, self.k, self.dt, self.misaligned = list(sizes), k, dt, misaligned
        self.t = [[None] * len(self.sizes) for _ in range(k)]
        if misaligned:
            self.offs, total = view_offsets(self.sizes, k)
            self.flat = to_sten(torch.full((total,), FILL, dtype=dt))
            self.covered = torch.zeros(total, dtype=torch.bool)
            self.views = [[self.flat.narrow(0, o, n) for o, n in zip(self.offs[j], self.sizes)] for j in range(k)]

    def put(self, j, tensors):
        """write list j (a None entry stays unwritten); returns the device tensors, None where the entry is None"""
        if not self.misaligned:
            self.t[j] = [None if t is None else to_sten(t.to(self.dt)) for t in tensors]
            return self.t[j]
        src, o = to_sten(torch.cat([t for t in tensors if t is not None]).to(self.dt)), 0
        for i, t in enumerate(tensors):
            if t is None:
                self.t[j][i] = None
                continue
            n = self.sizes[i]
            self.views[j][i].copyFrom(src.narrow(0, o, n))
            self.covered[self.offs[j][i]:self.offs[j][i] + n] = True
            self.t[j][i] = self.views[j][i]
            o += n
        return self.t[j]

    def get(self, j):
        """list j on the host, in dt (None where nothing was put)"""
        if not self.misaligned:
            return [None if t is None else to_torch(t).to(self.dt) for t in self.t[j]]
        host = to_torch(self.flat).to(self.dt)
        outside = host[~self.covered]
        assert torch.equal(bits(outside), bits(torch.full_like(outside, FILL))), "an element outside the views was written"
        return [None if t is None else host[o:o + n].clone() for t, o, n in zip(self.t[j], self.offs[j], self.sizes)]

    def assert_misaligned(self, a=0, b=1):
        """from data_ptr(): the bases land on every residue of 16 bytes, and some tensor has list a aligned with list b misaligned"""
        if not self.misaligned:
            return
        isz = torch.empty(0, dtype=self.dt).element_size()
        res = [[v.data_ptr % 16 for v in self.views[j]] for j in range(self.k)]
        assert all(v.is_contiguous() for vs in self.views for v in vs)
        assert {r for rs in res for r in rs} == set(range(0, 16, isz)), "the bases must land on every residue of 16 bytes"
        if self.k > 1:
            assert any(ra == 0 and rb != 0 for ra, rb in zip(res[a], res[b])), "no tensor with an aligned parameter and a misaligned gradient"


def largest(traj, ref):
    """largest absolute distance per state kind over all steps and tensors"""
    return [max(float((a.double() - b.double()).abs().max()) for s, r in zip(traj, ref) for a, b in zip(s[k], r[k])) for k in range(len(ref[0]))]


def assert_f64(got, ref, names):
    for step, (s, r) in enumerate(zip(got, ref)):
        for k, what in enumerate(names):
            for i, (a, b) in enumerate(zip(s[k], r[k])):
                np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-14, atol=1e-14 * float(b.abs().max()), err_msg=f"{what}[{i}] after step {step + 1}")


def assert_f32_rule(label, got, ref, chain, names):
    """test_descriptor_forms_f32's rule: the kernel at most twice as far from the f64 restatement as the f32 restatement on the same inputs,
    per state kind, and that yardstick itself within 2^-20 of each tensor's largest magnitude"""
    for s, r in zip(chain, ref):
        for k in range(len(names)):
            for a, b in zip(s[k], r[k]):
                assert float((a.double() - b).abs().max()) <= 2.0 ** -20 * float(b.abs().max()), "the f32 yardstick itself is off: choose another seed"
    d_kernel, d_chain = largest(got, ref), largest(chain, ref)
    print(f"{label}: kernel distances {tuple(names)} {d_kernel}, f32 restatement {d_chain}")
    for what, dk, dc in zip(names, d_kernel, d_chain):
        assert dk <= 2 * dc, f"{label} {what}: kernel {dk:.3e} from the f64 restatement, the f32 chain {dc:.3e}"


def assert_none_tensor_untouched(got, dt, store=None):
    params0, _ = size_inputs()
    p0 = params0[NONE_AT] if store is None else params0[NONE_AT].to(store)
    for s in got:
        assert torch.equal(bits(s[0][NONE_AT]), bits(p0.to(dt))), "a parameter without a gradient moved"
        assert not s[1][NONE_AT].any() and not s[2][NONE_AT].any(), "moments of a parameter without a gradient moved"


# ---- AdamW ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adamw_restated(dt, store=None, debias=True):
    """[(p, m, v) after each step] of R.AdamW in dtype dt; store: the 16-bit type the parameters and gradients are rounded to first (what a
    mixed-precision run is fed, widened)"""
    params0, steps = size_inputs()
    q = (lambda t: t.to(dt)) if store is None else (lambda t: t.to(store).to(dt))
    ps = [q(p).clone() for p in params0]
    opt = R.AdamW(ps, debias=debias, **ADAMW_HYPER)
    out = []
    for gs, f in zip(steps, FACTORS):
        opt.step([None if g is None else q(g).clone() for g in gs], f)
        out.append(([p.clone() for p in ps], [m.clone() for m in opt.mt], [v.clone() for v in opt.vt]))
    return out


def adamw_kernel(dt, misaligned, mixed=False, debias=True):
    """[(p, m, v, working copies) after each step] of nn.AdamW_tagged on the device"""
    params0, steps = size_inputs()
    lay = Layout(SIZES, 2, dt, misaligned)
    ps = lay.put(0, params0)
    lay.assert_misaligned()
    opt = nn.AdamW_tagged(ps, debias=debias, mixedPrecision=mixed, **ADAMW_HYPER)
    out = []
    for gs, f in zip(steps, FACTORS):
        opt.step(lay.put(1, gs), f)
        st = [to_torch(t) for t in opt.state]
        assert len(st) == 1 + (3 if mixed else 2) * N and st[0].item() == len(out) + 1
        out.append((lay.get(0), st[1:1 + N], st[1 + N:1 + 2 * N], st[1 + 2 * N:]))
    return out


@pytest.mark.parametrize("misaligned,debias", [(False, True), (True, True), (False, False)], ids=["aligned", "misaligned", "aligned-no-debias"])
def test_adamw_descriptor_forms_f64(gpu, misaligned, debias):
    ref = adamw_restated(torch.float64, None, debias)
    got = adamw_kernel(torch.float64, misaligned, debias=debias)
    print(f"adamw f64 {'misaligned' if misaligned else 'aligned'} debias={debias}: largest distances (p, m, v) {largest(got, ref)}")
    assert_f64(got, ref, "pmv")
    assert_none_tensor_untouched(got, torch.float64)


@LAYOUTS
def test_adamw_descriptor_forms_f32(gpu, misaligned):
    ref, chain = adamw_restated(torch.float64), adamw_restated(torch.float32)
    got = adamw_kernel(torch.float32, misaligned)
    assert_f32_rule(f"adamw f32 {'misaligned' if misaligned else 'aligned'}", got, ref, chain, "pmv")
    assert_none_tensor_untouched(got, torch.float32)


@LAYOUTS
@HALVES
def test_adamw_half_precision_storage_is_one_rounding(gpu, dt, misaligned):
    """test_half_precision_storage_is_one_rounding's argument for AdamW without mixed precision: parameter and moments are stored in the
    16-bit type, the kernel computes in f32 and rounds each stored value once."""
    sizes = [7, 1025]
    gen = torch.Generator().manual_seed(11)
    mk = lambda f: [f(n).to(dt) for n in sizes]
    p0 = mk(lambda n: torch.randn(n, generator=gen))
    g0 = mk(lambda n: torch.randn(n, generator=gen))
    m0 = mk(lambda n: torch.randn(n, generator=gen) * 0.5)
    v0 = mk(lambda n: torch.rand(n, generator=gen) + 0.25)
    hyper = dict(weightDecay=0.05, learningRate=0.01, beta1=0.9, beta2=0.999)
    pr, gr = [p.float() for p in p0], [g.float() for g in g0]
    ropt = R.AdamW(pr, **hyper)
    ropt.load([torch.tensor(3.0, dtype=torch.float64)] + [t.float() for t in m0 + v0])
    ropt.step(gr, 1.0)
    lay = Layout(sizes, 2, dt, misaligned)
    ph, gh = lay.put(0, p0), lay.put(1, g0)
    hopt = nn.AdamW(ph, **hyper)
    hopt.load([S.STen.scalarDouble(3.0)] + [to_sten(t) for t in m0 + v0])
    hopt.step(gh, 1.0)
    ms, vs = moments(hopt, len(sizes))
    assert ms[0].dtype == vs[0].dtype == TORCH2LAMP[dt], "without mixed precision the moments have the parameter's dtype"
    for what, got, ref in (("p", lay.get(0), pr), ("m", [to_torch(t) for t in ms], ropt.mt), ("v", [to_torch(t) for t in vs], ropt.vt)):
        for i, (a, b) in enumerate(zip(got, ref)):
            d = ulp_distance(a.to(dt), b.to(dt))
            assert d <= 1, f"{what}[{i}]: {d} units in the last place"
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(lay.get(1), g0)), "AdamW only reads its gradients"
    assert hopt.state[0].to_numpy() == 4.0


@LAYOUTS
@HALVES
def test_adamw_mixed_precision(gpu, dt, misaligned):
    """The benchmark's form: 16-bit parameters and gradients, f32 working copies and moments.  The f32 state obeys the f32 rule against the
    f64 restatement fed the same 16-bit values widened, and after EVERY step each model parameter is bit for bit the round-to-nearest-even
    cast of the kernel's own working copy."""
    ref, chain = adamw_restated(torch.float64, dt), adamw_restated(torch.float32, dt)
    got = adamw_kernel(dt, misaligned, mixed=True)
    for step, (p, m, v, w) in enumerate(got):
        assert all(t.dtype == torch.float32 for t in m + v + w) and len(w) == N
        for i, (a, b) in enumerate(zip(p, w)):
            assert torch.equal(bits(a), bits(b.to(dt))), f"model parameter {i} after step {step + 1} is not the cast of its working copy"
    assert_f32_rule(f"adamw mixed {dt} {'misaligned' if misaligned else 'aligned'}", [(w, m, v) for p, m, v, w in got], ref, chain, "wmv")
    assert_none_tensor_untouched(got, dt, dt)
    params0, _ = size_inputs()
    assert all(torch.equal(bits(s[3][NONE_AT]), bits(params0[NONE_AT].to(dt).float())) for s in got), "a working copy without a gradient moved"


@HALVES
def test_adamw_mixed_precision_with_an_f32_tensor_takes_both_passes(gpu, dt):
    """One call over a 16-bit tensor with a working copy AND an f32 tensor without one: lamp_adamw_step_ runs the (f32 state, 16-bit
    gradient) pass and the (f32, f32) pass.  Both against R.AdamW(mixedPrecision=True), which widens only the 16-bit tensor."""
    sizes, kinds = [1025, 7, 2049], [dt, torch.float32, dt]
    gen = torch.Generator().manual_seed(21)
    p0 = [torch.randn(n, generator=gen).to(k) for n, k in zip(sizes, kinds)]
    gs = [[torch.randn(n, generator=gen).to(k) for n, k in zip(sizes, kinds)] for _ in range(3)]
    hyper = dict(weightDecay=0.05, learningRate=0.01, beta1=0.9, beta2=0.999)

    def restated(cdt):
        ps = [p.clone() if cdt == torch.float32 else p.to(cdt) for p in p0]
        opt = R.AdamW(ps, mixedPrecision=cdt == torch.float32, **hyper)
        out = []
        for g in gs:
            opt.step([x.clone() if cdt == torch.float32 else x.to(cdt) for x in g], 1.0)
            work = [p if w is None else w for p, w in zip(ps, opt.workingCopy)]
            out.append(([t.clone() for t in work], [t.clone() for t in opt.mt], [t.clone() for t in opt.vt]))
        return out
    ref, chain = restated(torch.float64), restated(torch.float32)
    ph = [to_sten(p) for p in p0]
    hopt = nn.AdamW(ph, mixedPrecision=True, **hyper)
    got = []
    for g in gs:
        hopt.step([to_sten(x) for x in g], 1.0)
        st = [to_torch(t) for t in hopt.state]
        assert len(st) == 1 + 2 * 3 + 2, "two working copies, after the moments"
        p, w = [to_torch(t) for t in ph], st[7:]
        assert all(t.dtype == torch.float32 for t in st[1:])
        assert torch.equal(bits(p[0].to(dt)), bits(w[0].to(dt))) and torch.equal(bits(p[2].to(dt)), bits(w[1].to(dt)))
        got.append(([w[0], p[1], w[1]], st[1:4], st[4:7]))
    assert_f32_rule(f"adamw mixed {dt} + f32", got, ref, chain, "wmv")


# ---- SGDW -----------------------------------------------------------------------------------------------------------------------------
SGDW_CASES = pytest.mark.parametrize("momentum,wd", [(None, 0.0), (None, 0.05), (0.9, 0.0), (0.9, 0.05)], ids=["plain", "wd", "mom", "mom-wd"])
SGDW_LR = 0.01


@functools.lru_cache(maxsize=None)
def sgdw_restated(dt, momentum, wd):
    """[(p, velocity) after each step] of R.SGDW in dtype dt (velocity: an empty list without momentum)"""
    params0, steps = size_inputs()
    ps = [p.to(dt).clone() for p in params0]
    opt = R.SGDW(ps, SGDW_LR, wd, momentum)
    out = []
    for gs, f in zip(steps, FACTORS):
        opt.step([None if g is None else g.to(dt).clone() for g in gs], f)
        out.append(([p.clone() for p in ps], [v.clone() for v in opt.state()]))
    return out


def sgdw_kernel(dt, misaligned, momentum, wd):
    params0, steps = size_inputs()
    lay = Layout(SIZES, 2, dt, misaligned)
    ps = lay.put(0, params0)
    lay.assert_misaligned()
    opt = nn.SGDW(ps, SGDW_LR, wd, momentum)
    out = []
    for gs, f in zip(steps, FACTORS):
        opt.step(lay.put(1, gs), f)
        st = [to_torch(t) for t in opt.state]
        assert len(st) == (0 if momentum is None else N)
        out.append((lay.get(0), st))
    return out


def assert_sgdw_none_tensor_untouched(got, dt):
    params0, _ = size_inputs()
    for p, vel in got:
        assert torch.equal(bits(p[NONE_AT]), bits(params0[NONE_AT].to(dt))), "a parameter without a gradient moved"
        assert not vel or not vel[NONE_AT].any(), "the velocity of a parameter without a gradient moved"


@LAYOUTS
@SGDW_CASES
def test_sgdw_descriptor_forms_f64(gpu, momentum, wd, misaligned):
    names = ["p"] if momentum is None else ["p", "velocity"]
    ref, got = sgdw_restated(torch.float64, momentum, wd), sgdw_kernel(torch.float64, misaligned, momentum, wd)
    print(f"sgdw f64 momentum={momentum} wd={wd}: largest distances {largest([s[:len(names)] for s in got], [r[:len(names)] for r in ref])}")
    assert_f64(got, ref, names)
    assert_sgdw_none_tensor_untouched(got, torch.float64)


@LAYOUTS
@SGDW_CASES
def test_sgdw_descriptor_forms_f32(gpu, momentum, wd, misaligned):
    names = ["p"] if momentum is None else ["p", "velocity"]
    cut = lambda traj: [s[:len(names)] for s in traj]
    ref, chain = sgdw_restated(torch.float64, momentum, wd), sgdw_restated(torch.float32, momentum, wd)
    got = sgdw_kernel(torch.float32, misaligned, momentum, wd)
    assert_f32_rule(f"sgdw f32 momentum={momentum} wd={wd} {'misaligned' if misaligned else 'aligned'}", cut(got), cut(ref), cut(chain), names)
    assert_sgdw_none_tensor_untouched(got, torch.float32)


@LAYOUTS
@pytest.mark.parametrize("momentum", [None, 0.9], ids=["plain", "mom"])
def test_sgdw_bf16_storage_is_one_rounding(gpu, momentum, misaligned):
    """one step on the descriptor inputs from a loaded non-zero velocity: parameter and velocity within one unit in the last place of the
    f32 restatement rounded once"""
    dt = torch.bfloat16
    params0, steps = size_inputs()
    p0, g0 = [p.to(dt) for p in params0], [None if g is None else g.to(dt) for g in steps[0]]
    gen = torch.Generator().manual_seed(12)
    v0 = [torch.randn(n, generator=gen).to(dt) * 0.1 for n in SIZES]
    pr = [p.float() for p in p0]
    ropt = R.SGDW(pr, SGDW_LR, 0.05, momentum)
    ropt.load([v.float() for v in v0])
    ropt.step([None if g is None else g.float() for g in g0], 1.0)
    lay = Layout(SIZES, 2, dt, misaligned)
    ph = lay.put(0, p0)
    hopt = nn.SGDW(ph, SGDW_LR, 0.05, momentum)
    if momentum is not None:
        hopt.load([to_sten(v) for v in v0])
    hopt.step(lay.put(1, g0), 1.0)
    for what, got, ref in (("p", lay.get(0), pr), ("velocity", [to_torch(t) for t in hopt.state], ropt.state())):
        for i, (a, b) in enumerate(zip(got, ref)):
            d = ulp_distance(a.to(dt), b.to(dt))
            assert d <= 1, f"{what}[{i}]: {d} units in the last place"
    assert torch.equal(bits(lay.get(0)[NONE_AT]), bits(p0[NONE_AT]))


def test_sgdw_entry_point_takes_per_tensor_hyperparameters(gpu):
    """nn.SGDW takes scalars; lamp_sgdw_step_ takes one learning rate, weight decay and momentum per tensor: two f64 steps of the 45
    tensors with a gradient, every array varying, against R.SGDW with the same arrays"""
    params0, steps = size_inputs()
    keep = [i for i in range(N) if i != NONE_AT]
    n = len(keep)
    lr = [0.01 * (1 + i % 3) for i in range(n)]
    wd = [0.0 if i % 4 == 1 else 0.02 * (1 + i % 2) for i in range(n)]
    mom = [0.5 + 0.1 * (i % 5) for i in range(n)]
    ps = [params0[i].double() for i in keep]
    ropt = R.SGDW(ps, lr, wd, mom)
    ph = [to_sten(params0[i].double()) for i in keep]
    vh = [S.STen.zeros([params0[i].numel()], S.F64) for i in keep]
    for s, f in ((0, 1.0), (1, 0.5)):
        gs = [steps[s][i].double() for i in keep]
        ropt.step([g.clone() for g in gs], f)
        gh = [to_sten(g) for g in gs]
        lib.lamp_sgdw_step_(handle_array([t.h for t in ph]), handle_array([t.h for t in gh]), handle_array([t.h for t in vh]), n,
                            f64_array(lr), f64_array(wd), f64_array(mom), f)
    assert_f64([([to_torch(t) for t in ph], [to_torch(t) for t in vh])], [(ps, ropt.state())], ["p", "velocity"])


# ---- RAdam and Yogi at misaligned bases: the element loop of mt_update_chunk -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def moment_restated(kind, dt, store=None):
    params0, steps = size_inputs()
    q = (lambda t: t.to(dt)) if store is None else (lambda t: t.to(store).to(dt))
    ps = [q(p).clone() for p in params0]
    opt = KINDS[kind][1](ps, **HYPER)
    out = []
    for gs in steps:
        opt.step([None if g is None else q(g).clone() for g in gs], 1.0)
        out.append(([p.clone() for p in ps], [m.clone() for m in opt.mt], [v.clone() for v in opt.vt]))
    return out


@pytest.mark.parametrize("kind", ["radam", "yogi"])
def test_radam_yogi_misaligned_f32(gpu, kind):
    """test_descriptor_forms_f32 with parameters and gradients at odd element offsets: the moments are the optimiser's own aligned
    allocations, so a chunk takes the packet path only where parameter AND gradient happen to sit on 16 bytes, the element loop elsewhere"""
    params0, steps = size_inputs()
    lay = Layout(SIZES, 2, torch.float32, True)
    ps = lay.put(0, params0)
    lay.assert_misaligned()
    opt = KINDS[kind][0](ps, **HYPER)
    got = []
    for gs in steps:
        opt.step(lay.put(1, gs), 1.0)
        ms, vs = moments(opt, N)
        got.append((lay.get(0), [to_torch(m) for m in ms], [to_torch(v) for v in vs]))
    assert_f32_rule(f"{kind} f32 misaligned", got, moment_restated(kind, torch.float64), moment_restated(kind, torch.float32), "pmv")
    assert_none_tensor_untouched(got, torch.float32)


@pytest.mark.parametrize("kind", ["radam", "yogi"])
def test_radam_yogi_misaligned_bf16(gpu, kind):
    """one step of the descriptor inputs in bf16 at odd element offsets (bases on every residue of 16 bytes in steps of 2): every stored
    value - Yogi's written-back gradient included - within one unit in the last place of the f32 restatement rounded once"""
    dt = torch.bfloat16
    params0, steps = size_inputs()
    p0, g0 = [p.to(dt) for p in params0], [None if g is None else g.to(dt) for g in steps[0]]
    pr, gr = [p.float() for p in p0], [None if g is None else g.float() for g in g0]
    ropt = KINDS[kind][1](pr, **HYPER)
    ropt.step(gr, 1.0)
    lay = Layout(SIZES, 2, dt, True)
    ps = lay.put(0, p0)
    lay.assert_misaligned()
    hopt = KINDS[kind][0](ps, **HYPER)
    hopt.step(lay.put(1, g0), 1.0)
    ms, vs = moments(hopt, N)
    for what, got, ref in (("p", lay.get(0), pr), ("m", [to_torch(t) for t in ms], ropt.mt), ("v", [to_torch(t) for t in vs], ropt.vt),
                           ("g", lay.get(1), gr)):
        for i, (a, b) in enumerate(zip(got, ref)):
            if b is not None:
                d = ulp_distance(a.to(dt), b.to(dt))
                assert d <= 1, f"{what}[{i}]: {d} units in the last place"
    assert torch.equal(bits(lay.get(0)[NONE_AT]), bits(p0[NONE_AT]))


# ---- clipping on its own ------------------------------------------------------------------------------------------------------------------
# The longest chain of additions a squared element passes through on its way into the total, counted from optim.hip:
#   1               the product x*x, rounded where the compiler does not contract it into the addition (exact in f64 for these inputs)
#   per_thread      mt_sumsq_kernel's serial `acc += x*x`: a chunk of MT_CHUNK = 1024 elements over 256 threads is 4 per thread on the
#                   element loop and on the packet path for f32 and f64 (256 or 512 packets of 4 or 2), 8 for 16-bit packets (128 packets
#                   of 8, one per thread), times the per_wg chunks a workgroup walks
#   8               block_sum: wave_sum's 6 butterfly levels, then 2 levels over the 4 wave sums (the other levels add exact zeros)
#   ceil(wgs / 256) mt_accumulate_kernel's serial adds over the partial sums of a group
#   8               its block_sum
#   1               total[0] + acc of a further group
def addition_depth(dt, per_wg, wgs):
    per_thread = (8 if dt in (torch.bfloat16, torch.float16) else 4) * per_wg
    return 1 + per_thread + 8 + (wgs + 255) // 256 + 8 + 1


def acc_eps(dt):
    return torch.finfo(torch.float64 if dt == torch.float64 else torch.float32).eps


def exact_norm(gs):
    """sqrt of the exact sum of squares: the square of an f32-representable value is exact in f64, math.fsum adds without error"""
    return math.sqrt(math.fsum(x for g in gs for x in (g.double() * g.double()).tolist()))


def midpoint_margin(r, dt):
    """relative distance of r from the nearest midpoint between two neighbouring values of dt"""
    b = torch.tensor([r], dtype=torch.float64).to(dt)
    ints = {2: torch.int16, 4: torch.int32}[b.element_size()]
    mids = [(float(b) + float((b.view(ints) + step).view(dt))) / 2 for step in (1, -1)]      # positive values: both neighbours of round(r)
    return min(abs(r - m) for m in mids) / r


def largest_group(sizes):
    """chunks (= workgroups at per_wg = 1) of the largest group of MT_MAX = 40 tensors"""
    return max(sum((n + 1023) // 1024 for n in sizes[b:b + 40]) for b in range(0, len(sizes), 40))


def check_clipped(label, dt, got, gs, theta, d):
    """every clipped element against the exact factor: (d / 2 + 4) eps relative - d eps on the sum is d / 2 on its root, then the square
    root, the division, the product, the store and a margin.  bf16: the norm is rounded to bf16 before the division (the same value here
    and there, because the exact norm is asserted to lie 4 d eps away from a bf16 rounding midpoint), and the stored value is one more
    rounding: one unit in the last place.  f32: neighbouring f32 values are 2^-23 to 2^-24 apart relative, so NO value lies 4 d eps =
    92 * 2^-23 away from their midpoints; the condition cannot be met and is not needed - the kernel's rounding of the norm to f32 is
    the half eps the bound already counts for the square root, against the UNROUNDED exact norm."""
    eps = acc_eps(dt)
    norm = exact_norm(gs)
    if dt == torch.bfloat16:
        margin = midpoint_margin(norm, dt)
        assert margin >= 4 * d * eps, f"the norm {norm!r} is {margin:.3e} from a bf16 rounding midpoint: choose another seed"
        norm = float(torch.tensor([norm], dtype=torch.float64).to(dt))
    factor = min(1.0, theta / norm)
    assert factor < 1.0, "theta must clip"
    worst = 0.0
    for i, (a, g) in enumerate(zip(got, gs)):
        want = g.double() * factor
        if dt == torch.bfloat16:
            u = ulp_distance(a.to(dt), want.to(dt))
            assert u <= 1, f"{label} g[{i}]: {u} units in the last place"
        else:
            err = (a.double() - want).abs()
            worst = max(worst, float((err / want.abs().clamp_min(1e-300)).max()))
            assert bool((err <= (d / 2 + 4) * eps * want.abs()).all()), f"{label} g[{i}]: {float((err / want.abs().clamp_min(1e-300)).max()):.3e} relative, bound {(d / 2 + 4) * eps:.3e}"
    print(f"{label}: d = {d}, bound {(d / 2 + 4) * eps:.3e}, largest relative error {worst:.3e}, norm {norm!r}")


def clip_inputs(dt):
    """the 45 descriptor gradients (step 0) as values of dt (f64: the f32 values widened, so that their squares are exact)"""
    _, steps = size_inputs()
    return [g.to(torch.bfloat16 if dt == torch.bfloat16 else torch.float32).to(dt) for g in steps[0] if g is not None]


@LAYOUTS
@pytest.mark.parametrize("dt", [torch.float32, torch.float64, torch.bfloat16], ids=["f32", "f64", "bf16"])
def test_clipping_against_the_exact_norm(gpu, dt, misaligned):
    gs = clip_inputs(dt)
    sizes = [g.numel() for g in gs]
    lay = Layout(sizes, 1, dt, misaligned)
    hs = lay.put(0, gs)
    lay.assert_misaligned()
    # per_wg = 1: 43 and 5 chunks in the two groups, far below 8 chunks per compute unit; one workgroup per chunk
    d = addition_depth(dt, 1, largest_group(sizes))
    nn.gradientClippingInPlace(hs, 1.0)
    check_clipped(f"clip {dt} {'misaligned' if misaligned else 'aligned'}", dt, lay.get(0), gs, 1.0, d)


@LAYOUTS
def test_clipping_above_the_norm_leaves_the_gradients_untouched(gpu, misaligned):
    gs = clip_inputs(torch.float32)
    lay = Layout([g.numel() for g in gs], 1, torch.float32, misaligned)
    hs = lay.put(0, gs)
    theta = 2.0 * exact_norm(gs)
    nn.gradientClippingInPlace(hs, theta)
    for a, g in zip(lay.get(0), gs):
        assert torch.equal(bits(a), bits(g))


def num_cus():
    """the library's own compute-unit count, the very number its launch rule reads (256 on an MI355X; hipDeviceProp's multiProcessorCount,
    what torch.cuda.get_device_properties(0).multi_processor_count reports - asked of the library so that the test process does not
    initialise a second HIP runtime through torch)"""
    n = C.c_int(0)
    lib.lamp_device_num_cus(C.byref(n))
    return n.value


@functools.lru_cache(maxsize=None)
def per_wg_inputs(cus):
    """[1025, 3, big, 2049, 1] with big sized so that the list makes 24 * cus + 3 chunks: this mirrors the rule at the launch site in
    lamp_gradient_clipping_, per_wg = min(16, max(1, chunks / (8 * cus))) - the form with per_wg > 1 exists from 16 * cus chunks on, and at
    least 3 * 8 * cus make per_wg = 3.  big's chunks are 3 .. 24 cus - 2 of the group: workgroup 0 walks chunks of tensors 0, 0 and 1, the
    workgroup that holds big's last chunk goes on into tensor 3.  Values are multiples of 2^-10 below 16 in magnitude, sentinels +-8 at
    every tensor edge and at big's chunk edges 1024 k - 1, 1024 k."""
    sizes = [1025, 3, (24 * cus - 5) * 1024 + 5, 2049, 1]
    gen = torch.Generator().manual_seed(41)
    gs = [(torch.randn(n, generator=gen) * 1024).round().clamp(-15 * 1024, 15 * 1024) / 1024 for n in sizes]
    for i, g in enumerate(gs):
        g[::97] = 0.0
        for k, j in enumerate(sentinel_at(g.numel())):
            g[j] = 8.0 if (i + k) % 2 == 0 else -8.0
    nb = sizes[2] // 1024
    for k in (1, 2, 3, 7, 4096 % nb, nb - 1, nb):
        gs[2][1024 * k - 1], gs[2][1024 * k] = 8.0, -8.0
    chunks = sum((n + 1023) // 1024 for n in sizes)
    per_wg = min(16, max(1, chunks // (8 * cus)))
    assert chunks >= 3 * 8 * cus and per_wg == 3
    return sizes, gs, exact_norm(gs), per_wg, (chunks + per_wg - 1) // per_wg


@pytest.mark.parametrize("dt,misaligned", [(torch.float32, False), (torch.float64, False), (torch.float32, True)],
                         ids=["f32", "f64", "f32-misaligned"])
def test_clipping_walks_several_chunks_per_workgroup(gpu, dt, misaligned):
    sizes, gs, norm, per_wg, wgs = per_wg_inputs(num_cus())
    d = addition_depth(dt, per_wg, wgs)
    eps = acc_eps(dt)
    if misaligned:                                       # big is a view at element offset 1 of a flat tensor, guarded by FILL on both sides
        flat = to_sten(torch.cat([torch.full((1,), FILL), gs[2], torch.full((3,), FILL)]))
        big = flat.narrow(0, 1, sizes[2])
        assert big.data_ptr % 16 == 4 and big.is_contiguous()
    else:
        big = to_sten(gs[2].to(dt))
    hs = [to_sten(g.to(dt)) for g in gs[:2]] + [big] + [to_sten(g.to(dt)) for g in gs[3:]]
    nn.gradientClippingInPlace(hs, 1.0)
    factor = 1.0 / norm
    worst = 0.0
    for i, (h, g) in enumerate(zip(hs, gs)):
        want = g.double() * factor
        err = (to_torch(h).double() - want).abs()
        worst = max(worst, float((err / want.abs().clamp_min(1e-300)).max()))
        assert bool((err <= (d / 2 + 4) * eps * want.abs()).all()), f"g[{i}]: {float((err / want.abs().clamp_min(1e-300)).max()):.3e} relative, bound {(d / 2 + 4) * eps:.3e}"
    if misaligned:
        host = to_torch(flat)
        assert torch.equal(bits(host[:1]), bits(torch.full((1,), FILL))) and torch.equal(bits(host[-3:]), bits(torch.full((3,), FILL)))
    print(f"clip per_wg = {per_wg} {dt}{' misaligned' if misaligned else ''}: {wgs} workgroups, d = {d}, bound {(d / 2 + 4) * eps:.3e}, largest relative error {worst:.3e}")


def test_clipping_propagates_a_nan(gpu):
    """one NaN element: the norm is NaN, ATen's minimum(theta / norm, 1) is NaN, and every gradient of both groups becomes NaN"""
    gs = [g.clone() for g in clip_inputs(torch.float32)]
    gs[3][1024] = float("nan")
    hs = [to_sten(g) for g in gs]
    nn.gradientClippingInPlace(hs, 1.0)
    for i, h in enumerate(hs):
        assert bool(torch.isnan(to_torch(h)).all()), f"g[{i}] is not all NaN"


def test_clipping_rejects_mixed_dtypes_and_writes_nothing(gpu):
    """The reference promotes (nn/package.scala:72-100 sums the norms in the first gradient's type); lamp_gradient_clipping_ insists on one
    dtype.  What it does today: a LampError before the first launch - gradients, parameters and state bit for bit as before."""
    gen = torch.Generator().manual_seed(6)
    p0 = [torch.randn(1025, generator=gen), torch.randn(7, generator=gen).to(torch.bfloat16)]
    g0 = [torch.randn(1025, generator=gen), torch.randn(7, generator=gen).to(torch.bfloat16)]
    ph, gh = [to_sten(p) for p in p0], [to_sten(g) for g in g0]
    opt = nn.AdamW(ph, weightDecay=0.05, clip=1.0)
    with pytest.raises(LampError):
        opt.step(gh, 1.0)
    for t, b in zip(ph + gh, p0 + g0):
        assert torch.equal(bits(to_torch(t).to(b.dtype)), bits(b)), "a rejected step wrote a tensor"
    st = opt.state
    assert st[0].to_numpy() == 0.0 and all(not to_torch(t).any() for t in st[1:])
    nn.AdamW(ph, weightDecay=0.05).step(gh, 1.0)         # without clip the same lists pass: one (state, gradient) pass per dtype


@pytest.mark.parametrize("kind", ["adamw", "sgdw", "sgdw-mom"])
def test_adamw_sgdw_clip_is_clipping_then_the_plain_step(gpu, kind):
    sizes = [7, 1025, 2049]
    gen = torch.Generator().manual_seed(3)
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    g0 = [torch.randn(n, generator=gen) for n in sizes]
    assert float(sum((g * g).sum() for g in g0)) > 1.0
    make = {"adamw": lambda p, **kw: nn.AdamW(p, weightDecay=0.05, learningRate=0.01, **kw),
            "sgdw": lambda p, **kw: nn.SGDW(p, 0.01, 0.05, **kw),
            "sgdw-mom": lambda p, **kw: nn.SGDW(p, 0.01, 0.05, momentum=0.9, **kw)}[kind]
    pa, ga = [to_sten(p) for p in p0], [to_sten(g) for g in g0]
    pb, gb = [to_sten(p) for p in p0], [to_sten(g) for g in g0]
    oa, ob = make(pa, clip=1.0), make(pb)
    for _ in range(2):
        oa.step(ga, 1.0)
        nn.gradientClippingInPlace(gb, 1.0)
        ob.step(gb, 1.0)
    for a, b in zip(pa + oa.state + ga, pb + ob.state + gb):
        assert torch.equal(bits(to_torch(a)), bits(to_torch(b)))
    assert not torch.equal(to_torch(ga[1]), g0[1]), "the gradients are clipped in place"


# ---- the bucket on the device ---------------------------------------------------------------------------------------------------------------
BUCKET_DTYPES = pytest.mark.parametrize("dt", [torch.float32, torch.float64, torch.bfloat16, torch.float16], ids=["f32", "f64", "bf16", "f16"])
SCALE, COUNT = 3.0, 7.0


def bucket_inputs(dt):
    _, steps = size_inputs()
    return [g.to(dt) for g in steps[1] if g is not None]


def flatten_on(device, ts, total):
    bucket = S.STen.full([total + 1], COUNT, S.F32, device)
    lib.lamp_flatten_into_(bucket, handle_array([t.h for t in ts]), len(ts), SCALE)
    return bucket


@LAYOUTS
@BUCKET_DTYPES
@pytest.mark.parametrize("divide", [1, 0], ids=["divide", "plain"])
def test_bucket_flatten_and_unflatten_are_exactly_rounded(gpu, dt, misaligned, divide):
    """The library is built without fast-math, so one f32 multiply and one IEEE f32 division are exactly rounded: bit for bit
    bucket[off + i] == f32(scale) * f32(g[i]) and out[i] == cast(bucket[off + i] / bucket[-1]) as torch computes them on the CPU, and as
    the library's own host path computes them on host copies; the bucket's last element, the count, is left alone by flatten."""
    gs = bucket_inputs(dt)
    sizes = [g.numel() for g in gs]
    total = sum(sizes)
    lay = Layout(sizes, 2, dt, misaligned)
    hs = lay.put(0, gs)
    lay.assert_misaligned()
    bucket = flatten_on(0, hs, total)
    want = torch.cat([torch.tensor(SCALE, dtype=torch.float32) * g.to(torch.float32) for g in gs] + [torch.tensor([COUNT])])
    got = to_torch(bucket)
    assert torch.equal(bits(got), bits(want)), "the bucket is not scale * g rounded once to f32 (or its count moved)"
    host_ts = [to_sten(g, S.CPU) for g in gs]
    host_bucket = flatten_on(S.CPU, host_ts, total)
    assert host_bucket.device == S.CPU and torch.equal(bits(to_torch(host_bucket)), bits(got)), "host and device buckets differ"
    assert all(torch.equal(bits(a), bits(g)) for a, g in zip(lay.get(0), gs)), "flatten only reads its tensors"

    outs = lay.put(1, [torch.full_like(g, 5.0) for g in gs])
    lib.lamp_unflatten_from_(handle_array([t.h for t in outs]), len(outs), bucket, divide)
    quotient = want / want[-1] if divide else want
    o = 0
    for i, (a, n) in enumerate(zip(lay.get(1), sizes)):
        assert torch.equal(bits(a), bits(quotient[o:o + n].to(dt))), f"out[{i}] is not cast(bucket / count)"
        o += n
    host_outs = [to_sten(torch.full_like(g, 5.0), S.CPU) for g in gs]
    lib.lamp_unflatten_from_(handle_array([t.h for t in host_outs]), len(host_outs), host_bucket, divide)
    for a, b in zip(lay.get(1), host_outs):
        assert torch.equal(bits(a), bits(to_torch(b).to(dt))), "host and device unflatten differ"
    assert torch.equal(bits(to_torch(bucket)), bits(want)), "unflatten only reads the bucket"


def test_bucket_rejections_write_nothing(gpu):
    gs = bucket_inputs(torch.float32)[:6]
    total = sum(g.numel() for g in gs)
    hs = [to_sten(g) for g in gs]
    odd = hs[:3] + [to_sten(gs[3].double())] + hs[4:]
    small, full = S.STen.full([total - 1], COUNT, S.F32), S.STen.full([total + 1], COUNT, S.F32)
    for bucket, ts in ((small, hs), (full, odd)):
        before = to_torch(bucket).clone()
        with pytest.raises(LampError):
            lib.lamp_flatten_into_(bucket, handle_array([t.h for t in ts]), len(ts), SCALE)
        assert torch.equal(bits(to_torch(bucket)), bits(before)), "a rejected flatten wrote the bucket"
        with pytest.raises(LampError):
            lib.lamp_unflatten_from_(handle_array([t.h for t in ts]), len(ts), bucket, 1)
        for t, g in zip(ts, gs):
            assert torch.equal(bits(to_torch(t).float()), bits(g)), "a rejected unflatten wrote a tensor"
    lib.lamp_flatten_into_(full, handle_array([t.h for t in hs]), len(hs), SCALE)      # the well-formed call passes
