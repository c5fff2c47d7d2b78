"""Shampoo and the batched Jacobi eigensolver through the public interface on the GPU (and, staged, on the CPU device) against the
restatement of tests/shampoo_ref.py and torch.linalg.svd in f64 on the CPU: the reference's known answer, every form and edge of the
eigensolver, trajectories in both preconditioner modes, the preconditioner schedule, the state round trip, rejected arguments and the
convolutions' re-pack hook."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from lamp_amd import nn
from lamp_amd import sten as S
from lamp_amd._capi import LampError, f64_array, handle_array, i64_array, lib
from tests import shampoo_ref as R
from tests.util import assert_close, to_sten, to_torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -52
SWEEP_CAP = 30


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


# ---- 1. the reference's known answer ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [0, S.CPU], ids=["gpu", "cpu-device"])
def test_shampoo_kat(gpu, device):
    k = R.KATS["matrix"]
    p = S.STen.from_numpy(np.array([k["init"]]), device, S.F64)
    g = S.STen.from_numpy(np.array([k["gradients"]]), device, S.F64)
    opt = nn.Shampoo([p], learningRate=k["learningRate"])
    for step in ("step1", "step2"):
        opt.step([g], 1.0)
        assert p.device == device
        assert np.round(p.to_numpy()[0], 4).tolist() == k[step]
    assert g.to_numpy()[0].tolist() == k["gradients"], "without momentum Shampoo only reads its gradients"
    assert opt.state[0].to_numpy() == 2.0


@pytest.mark.parametrize("device", [0, S.CPU], ids=["gpu", "cpu-device"])
def test_shampoo_kat_diagonal_side(gpu, device):
    k = R.KATS["diagonal"]
    gen = torch.Generator().manual_seed(3)
    g0 = torch.rand(k["shape"], generator=gen, dtype=torch.float64)
    pr = torch.ones(k["shape"], dtype=torch.float64)
    ref = R.Shampoo([pr], learningRate=k["learningRate"])
    p = to_sten(torch.ones(k["shape"], dtype=torch.float64), device)
    g = to_sten(g0, device)
    opt = nn.Shampoo([p], learningRate=k["learningRate"])
    assert opt.state[3].shape == [513] and opt.state[1].shape == [1, 1]
    for _ in range(2):
        opt.step([g], 1.0)
        ref.step([g0], 1.0)
    assert torch.isfinite(to_torch(p)).all()
    assert_close(to_torch(p), pr, 1e-12, "two steps with a vector right side")


# ---- 2. the eigensolver --------------------------------------------------------------------------------------------------------------
# 1, 2 and 3 (a bye); 5; 64 and 65 (a second row per lane); 127 and 128 (the last side that lives in LDS); 129 (the first in the global
# workspace); 512 (the limit) - in ONE call, so that both forms and mixed sizes share a launch
SIDES = [1, 2, 3, 5, 64, 65, 127, 128, 129, 512]
EPS = 1e-4
EIG_KINDS = ["eps_identity", "ascending_diagonal", "full_rank", "rank_n_over_8", "f32_not_bit_symmetric"]


@functools.lru_cache(maxsize=None)
def eig_case(kind):
    """(matrices, [(u, s) of torch.linalg.svd on the f64 copy]) per side; computed once"""
    gen = torch.Generator().manual_seed(EIG_KINDS.index(kind) + 11)
    mats = []
    for n in SIDES:
        eye = EPS * torch.eye(n, dtype=torch.float64)
        if kind == "eps_identity":
            a = eye
        elif kind == "ascending_diagonal":
            a = torch.diag(0.5 + torch.arange(n, dtype=torch.float64))
        elif kind == "full_rank":
            g = torch.randn(n, 2 * n, generator=gen, dtype=torch.float64) * 0.05
            a = eye + g.mm(g.t())
        elif kind == "rank_n_over_8":
            g = torch.randn(n, max(1, n // 8), generator=gen, dtype=torch.float64) * 0.05
            a = eye + g.mm(g.t())
        else:
            g = torch.randn(n, 2 * n, generator=gen, dtype=torch.float32) * 0.05
            a = (EPS * torch.eye(n, dtype=torch.float32) + g.mm(g.t()))
            up = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
            a = torch.where(up, torch.nextafter(a, torch.full_like(a, 1e9)), a)          # the upper triangle one ulp up
            assert n == 1 or not torch.equal(a, a.t())
        mats.append(a)
    refs = []
    for a in mats:
        u, s, _ = torch.linalg.svd(a.double())
        refs.append((u, s))
    return mats, refs


@pytest.mark.parametrize("kind", EIG_KINDS)
def test_symmetric_eig_against_cpu_svd(gpu, kind):
    """Both methods are backward stable with error <= c n 2^-52 s_max, so with kappa = s_max / s_min of the CPU result:
    values |ds| / s <= 4 n 2^-52 kappa; U^T U - I and (A U - U diag(s)) / s_max <= 4 n 2^-52 in max-norm;
    U diag(s^-1/4) U^T within 4 n 2^-52 kappa of the CPU's, relative to its largest entry.
    The f32 matrix is not symmetric, so A U = U diag(s) holds only to its asymmetry (2^-24); what IS defined for left singular vectors is
    A A^T U = U diag(s^2): a backward error dA gives 2 |dA| s_max there and the f64 product A A^T of the check adds n 2^-52 s_max^2,
    hence 3 x the bound, relative to s_max^2."""
    mats, refs = eig_case(kind)
    vals, vecs, status = S.symmetricEig([to_sten(a) for a in mats], vectors=True)
    only_vals, none, status2 = S.symmetricEig([to_sten(a) for a in mats])
    assert none is None and status2 == status
    print(f"{kind}: sweeps {dict(zip(SIDES, status))}")
    assert all(1 <= s < SWEEP_CAP for s in status), status
    for n, a, (ur, sr), v, ov, u in zip(SIDES, mats, refs, vals, only_vals, vecs):
        a = a.double()
        s, uu = to_torch(v), to_torch(u)
        assert s.dtype == torch.float64 and list(s.shape) == [n] and list(uu.shape) == [n, n]
        assert torch.equal(bits(s), bits(to_torch(ov))), "the values do not depend on whether the vectors are asked for"
        assert torch.equal(s, torch.sort(s, descending=True).values), "descending order"
        kappa = float(sr.max() / sr.min())
        bound = 4 * n * U
        e_val = float(((s - sr).abs() / sr).max())
        e_orth = float((uu.t().mm(uu) - torch.eye(n, dtype=torch.float64)).abs().max())
        if kind == "f32_not_bit_symmetric":
            e_res = float((a.mm(a.t()).mm(uu) - uu * (s * s).view(1, -1)).abs().max() / float(sr.max()) ** 2) / 3
        else:
            e_res = float((a.mm(uu) - uu * s.view(1, -1)).abs().max() / float(sr.max()))
        root = (uu * s.pow(-0.25).view(1, -1)).mm(uu.t())
        root_ref = (ur * sr.pow(-0.25).view(1, -1)).mm(ur.t())
        e_root = float((root - root_ref).abs().max() / root_ref.abs().max())
        print(f"  n={n}: kappa {kappa:.2e}  values {e_val:.2e} (<= {bound * kappa:.2e})  orth {e_orth:.2e}  residual {e_res:.2e} (<= {bound:.2e})  "
              f"root {e_root:.2e} (<= {bound * kappa:.2e})")
        assert e_val <= bound * kappa, (n, e_val)
        assert e_orth <= bound, (n, e_orth)
        assert e_res <= bound, (n, e_res)
        assert e_root <= bound * kappa, (n, e_root)


def _raw_eig(mats, vals, vecs, status):
    lib.lamp_symmetric_eig(handle_array([t.h for t in mats]), len(mats), handle_array([t.h for t in vals]),
                           handle_array([t.h for t in vecs]) if vecs is not None else None, status.h if status is not None else None)


def test_symmetric_eig_rejections_write_nothing(gpu):
    with pytest.raises(LampError, match="513"):
        S.symmetricEig([S.STen.zeros([513, 513], S.F64)])
    with pytest.raises(LampError):
        S.symmetricEig([S.STen.zeros([4, 5], S.F64)])
    with pytest.raises(LampError):
        S.symmetricEig([S.STen.zeros([4, 4], S.BF16)])
    # a NaN in ONE matrix of the call: an error, and no output of ANY matrix is written (an LDS-form and a global-form neighbour)
    good = [torch.eye(5, dtype=torch.float64) * 2, torch.eye(130, dtype=torch.float64) * 3]
    bad = torch.eye(7, dtype=torch.float32)
    bad[3, 5] = float("nan")
    mats = [to_sten(good[0]), to_sten(bad), to_sten(good[1])]
    vals = [S.STen.full([n], -1.0, S.F64) for n in (5, 7, 130)]
    vecs = [S.STen.full([n, n], -1.0, S.F64) for n in (5, 7, 130)]
    with pytest.raises(LampError, match="NaN"):
        _raw_eig(mats, vals, vecs, None)
    for t in vals + vecs:
        assert bool((to_torch(t) == -1.0).all()), "a rejected call wrote an output"
    mats[1] = to_sten(torch.eye(7, dtype=torch.float32))
    _raw_eig(mats, vals, vecs, None)                                  # the well-formed call passes
    assert to_torch(vals[2]).tolist() == [3.0] * 130
    # a singular matrix is not an error: its zero columns stay zero
    z = torch.zeros(4, 4, dtype=torch.float64)
    z[1, 1] = 2.0
    v, u, st = S.symmetricEig([to_sten(z)], vectors=True)
    assert to_torch(v[0]).tolist() == [2.0, 0.0, 0.0, 0.0] and torch.isfinite(to_torch(u[0])).all()


# ---- 3. trajectories -------------------------------------------------------------------------------------------------------------------
def _hyper(mom, clip):
    return dict(learningRate=R.TRAJ_LR, momentum=[mom] * len(R.TRAJ_SHAPES), clip=R.TRAJ_CLIP if clip else None)


@functools.lru_cache(maxsize=None)
def restated_trajectory(dt, paper, mom, clip):
    """after every step of the restatement in dtype dt: (parameters, state, gradients as the step left them)"""
    params0, steps = R.trajectory_inputs()
    ps = [p.to(dt).clone() for p in params0]
    opt = R.Shampoo(ps, paper=paper, **_hyper(mom, clip))
    out = []
    for gs in steps:
        g = [None if x is None else x.to(dt).clone() for x in gs]
        opt.step(g, 1.0)
        out.append(([p.clone() for p in ps], [t.clone() for t in opt.state], g))
    return out


def kernel_trajectory(dt, paper, mom, clip):
    params0, steps = R.trajectory_inputs()
    ps = [to_sten(p.to(dt)) for p in params0]
    opt = nn.Shampoo(ps, paperPreconditioner=paper, **_hyper(mom, clip))
    out = []
    for gs in steps:
        g = [None if x is None else to_sten(x.to(dt)) for x in gs]
        opt.step(g, 1.0)
        out.append(([to_torch(p) for p in ps], [to_torch(t) for t in opt.state], [None if x is None else to_torch(x) for x in g]))
    return out


MODES = pytest.mark.parametrize("paper", [False, True], ids=["reference", "paper"])
MOMS = pytest.mark.parametrize("mom", [0.0, 0.5], ids=["mom0", "mom0.5"])
CLIPS = pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])


@MODES
@MOMS
@CLIPS
def test_trajectory_f64(gpu, paper, mom, clip):
    """1e-9 per element: the dominant term is the eigensolver's 4 n 2^-52 kappa through s^-1/4, 144 * 4 * 2.2e-16 * 2.1e3 / 4 = 7e-11 for the
    inverse roots at the sizes and the conditioning of this case (kappa <= 2.1e3, tests/test_shampoo.py), times lr * |G| in a parameter"""
    ref = restated_trajectory(torch.float64, paper, mom, clip)
    got = kernel_trajectory(torch.float64, paper, mom, clip)
    _, steps = R.trajectory_inputs()
    n = len(R.TRAJ_SHAPES)
    for t, ((gp, gs, gg), (rp, rs, rg)) in enumerate(zip(got, ref)):
        assert len(gs) == len(rs) == 1 + 5 * n and float(gs[0]) == t + 1
        for i, (a, b) in enumerate(zip(gp, rp)):
            assert_close(a, b, 1e-9, f"step {t + 1}: parameter {i}")
        for i, (a, b) in enumerate(zip(gs[1:], rs[1:])):
            assert list(a.shape) == list(b.shape)
            assert_close(a, b, 1e-9, f"step {t + 1}: state {i + 1}", scale="max")
        for i, (a, b, g0) in enumerate(zip(gg, rg, steps[t])):
            if a is None:
                assert b is None
            elif mom == 0 and not clip:
                assert torch.equal(bits(a), bits(g0.double())), "without momentum the gradients are only read"
            else:
                assert_close(a, b, 1e-12, f"step {t + 1}: gradient {i} after the step")
                assert mom == 0 or clip or not torch.equal(a, g0.double()) or t == 0
    # the parameter without a gradient and its state never moved
    params0, _ = R.trajectory_inputs()
    assert torch.equal(got[-1][0][R.TRAJ_NONE_AT], params0[R.TRAJ_NONE_AT].double())
    assert torch.equal(got[-1][1][1 + 2 * R.TRAJ_NONE_AT], 1e-4 * torch.eye(R.TRAJ_SHAPES[R.TRAJ_NONE_AT][0], dtype=torch.float64))


@MODES
@MOMS
@CLIPS
def test_trajectory_f32(gpu, paper, mom, clip):
    """the yardstick is the restatement in f32 against the restatement in f64: the GPU's f32 parameters must be within 4 x that distance
    of the f64 restatement, per tensor, in max-norm (only the GEMMs' summation order differs; the sensitivity of the small eigenvalues
    to f32 statistics is in the yardstick itself)"""
    ref64 = restated_trajectory(torch.float64, paper, mom, clip)
    ref32 = restated_trajectory(torch.float32, paper, mom, clip)
    got = kernel_trajectory(torch.float32, paper, mom, clip)
    for t in range(len(got)):
        for i, (a, r32, r64) in enumerate(zip(got[t][0], ref32[t][0], ref64[t][0])):
            assert a.dtype == torch.float32
            yard = float((r32.double() - r64).abs().max())
            dist = float((a.double() - r64).abs().max())
            if t == len(got) - 1:
                print(f"parameter {i} after step {t + 1}: GPU f32 {dist:.3e} from the f64 restatement, restated f32 {yard:.3e}")
            assert dist <= 4 * yard, f"step {t + 1}: parameter {i}: {dist:.3e} > 4 x {yard:.3e}"
    if mom > 0:
        for a, b in zip(got[-1][2], ref32[-1][2]):
            if a is not None:
                assert_close(a, b.double(), 1e-6, "the blended gradient is written back")


# ---- 4. the schedule ---------------------------------------------------------------------------------------------------------------------
def test_preconditioner_schedule(gpu):
    """103 steps with updatePreconditionerEveryNIterations = 3: the roots are recomputed on every step up to 100, then at 102 only"""
    shapes = [[4, 3], [3]]
    gen = torch.Generator().manual_seed(4)
    p0 = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    rp = [p.clone() for p in p0]
    ref = R.Shampoo(rp, learningRate=0.01, updatePreconditionerEveryNIterations=3)
    ps = [to_sten(p) for p in p0]
    opt = nn.Shampoo(ps, learningRate=0.01, updatePreconditionerEveryNIterations=3)
    ltinv = {}
    for t in range(1, 104):
        gs = [torch.randn(s, generator=gen, dtype=torch.float64) * 0.1 for s in shapes]
        ref.step([g.clone() for g in gs], 1.0)
        opt.step([to_sten(g) for g in gs], 1.0)
        if t >= 99:
            for i, (a, b) in enumerate(zip(ps, rp)):
                assert_close(to_torch(a), b, 1e-9, f"step {t}: parameter {i}")
            ltinv[t] = to_torch(opt.state[2])
    assert not torch.equal(ltinv[99], ltinv[100])
    assert torch.equal(bits(ltinv[100]), bits(ltinv[101])), "step 101 keeps the stored roots"
    assert not torch.equal(ltinv[101], ltinv[102]), "step 102 is a multiple of 3"
    assert torch.equal(bits(ltinv[102]), bits(ltinv[103]))
    assert opt.state[0].to_numpy() == 103.0


# ---- 5. the state ------------------------------------------------------------------------------------------------------------------------
def test_state_layout_and_round_trip(gpu):
    """[count] ++ (lt, ltinv)* ++ (rt, rtinv)* ++ lastGradient; 99 steps, state -> a fresh optimiser's load, 4 more == 103 steps straight,
    bitwise: with N = 3 a step count lost in the round trip would recompute the roots at 101 and 103"""
    shapes = [[4, 3], [3], [2, 513]]
    gen = torch.Generator().manual_seed(8)
    p0 = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    gs = [[torch.randn(s, generator=gen, dtype=torch.float64) * 0.1 for s in shapes] for _ in range(103)]
    hyper = dict(learningRate=0.01, updatePreconditionerEveryNIterations=3, momentum=0.5)
    pa = [to_sten(p) for p in p0]
    oa = nn.Shampoo(pa, **hyper)
    st = oa.state
    assert [t.shape for t in st] == [[], [4, 4], [4, 4], [3, 3], [3, 3], [2, 2], [2, 2], [3, 3], [3, 3], [1, 1], [1, 1], [513], [513], [4, 3], [3], [2, 513]]
    assert st[0].dtype == S.F64 and st[0].to_numpy() == 0.0
    assert torch.equal(to_torch(st[1]), 1e-4 * torch.eye(4, dtype=torch.float64)) and torch.equal(to_torch(st[12]), 1e-4 * torch.ones(513, dtype=torch.float64))
    for g in gs:
        oa.step([to_sten(x) for x in g], 1.0)
    pb = [to_sten(p) for p in p0]
    ob = nn.Shampoo(pb, **hyper)
    for g in gs[:99]:
        ob.step([to_sten(x) for x in g], 1.0)
    saved = [t.clone() for t in ob.state]
    assert saved[0].to_numpy() == 99.0
    pc = [p.clone() for p in pb]
    oc = nn.Shampoo(pc, **hyper)
    oc.load(saved)
    for g in gs[99:]:
        oc.step([to_sten(x) for x in g], 1.0)
    assert oc.state[0].to_numpy() == 103.0
    for a, c in zip(pa + oa.state, pc + oc.state):
        assert torch.equal(bits(to_torch(a)), bits(to_torch(c)))


# ---- 6. rejected arguments ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_write_nothing(gpu):
    gen = torch.Generator().manual_seed(1)
    with pytest.raises(LampError, match="f32 or f64"):
        nn.Shampoo([S.STen.from_numpy(np.ones((4, 3), dtype=np.float32), 0, S.BF16)])
    with pytest.raises(LampError, match="0-d"):
        nn.Shampoo([S.STen.scalarDouble(1.0)])
    p0 = [torch.randn(4, 3, generator=gen, dtype=torch.float32), torch.randn(7, generator=gen, dtype=torch.float32)]
    p = [to_sten(x) for x in p0]
    opt = nn.Shampoo(p, learningRate=0.1, clip=0.5, momentum=0.5)
    opt.step([to_sten(torch.randn(4, 3, generator=gen)), to_sten(torch.randn(7, generator=gen))], 1.0)
    before = [to_torch(t).clone() for t in p + opt.state]
    for bad in (to_sten(torch.randn(3, 4, generator=gen)), to_sten(torch.randn(4, 4, generator=gen)), to_sten(torch.randn(4, 3, generator=gen).double())):
        g1 = to_sten(torch.randn(7, generator=gen))
        g1_before = to_torch(g1).clone()
        with pytest.raises(LampError):
            opt.step([bad, g1], 1.0)
        assert torch.equal(bits(to_torch(g1)), bits(g1_before)), "a rejected step clipped or blended a gradient"
    for t, b in zip(p + opt.state, before):
        assert torch.equal(bits(to_torch(t)), bits(b)), "a rejected step wrote a parameter or the state"
    # the stateless entry point: half-precision tensors are rejected before anything is written
    h = lambda shape: S.STen.from_numpy(np.ones(shape, dtype=np.float32), 0, S.BF16)
    lists = [[h((4, 3))], [h((4, 3))], [h((4, 4))], [h((4, 4))], [h((3, 3))], [h((3, 3))], [h((4, 3))]]
    with pytest.raises(LampError, match="only f32 and f64"):
        lib.lamp_shampoo_step_(*[handle_array([t.h for t in ts]) for ts in lists], 1, f64_array([0.1]), f64_array([0.5]), 1, 100, 0)
    for ts in lists:
        assert bool((to_torch(ts[0].castToFloat()) == 1.0).all())


# ---- 7. the re-pack hook -------------------------------------------------------------------------------------------------------------------
def _pack_counts():
    """{entries, pinned, hits, packs, repacked} of the packed-filter caches, summed over the backends (a debug export, not in the header)"""
    buf = (C.c_uint64 * 5)()
    lib.lamp_debug_pack_cache_counts(buf)
    return dict(zip(("entries", "pinned", "hits", "packs", "repacked"), (int(v) for v in buf)))


def test_convolution_after_a_step_uses_the_new_filter(gpu):
    """a convolution whose filter Shampoo has updated computes with the new filter: the packed image the first call cached follows the
    update through the re-pack hook, or is packed again - never the stale one"""
    gen = torch.Generator().manual_seed(6)
    w0 = torch.randn(16, 16, 3, 3, generator=gen, dtype=torch.float32) * 0.1
    x0 = torch.randn(8, 16, 12, 12, generator=gen, dtype=torch.float32)
    g0 = torch.randn(16, 16, 3, 3, generator=gen, dtype=torch.float32) * 0.05
    w, x = to_sten(w0), to_sten(x0)
    one = i64_array([1, 1])

    def conv():
        o = C.c_void_p()
        lib.lamp_convolution(C.byref(o), x.h, w.h, None, one, one, one, 2, 0, i64_array([0, 0]), 1)
        return to_torch(S.STen(o))
    y0 = conv()
    conv()                                                        # (a second call: whatever the backend caches of the filter is cached now)
    opt = nn.Shampoo([w], learningRate=0.05)
    opt.step([to_sten(g0)], 1.0)
    y1 = conv()
    assert float((to_torch(w) - w0).abs().max()) > 1e-3, "the step moved the filter"
    want = torch.nn.functional.conv2d(x0.double(), to_torch(w).double(), padding=1)
    assert_close(y1, want, 1e-5, "the convolution after the step")
    assert float((y1.double() - y0.double()).abs().max()) > 1e-3


def test_replayed_resnet_step_tracks_the_weights(gpu):
    """tests/test_optimizers_gpu.py's test of the same name with Shampoo at f32, B = 8: forward + backprop captured once and replayed while
    the optimiser updates the weights eagerly between replays.  The convolutions' packed filter images follow an update only through the
    step's re-pack hook, which writes them in place: the capture finds them current in the cache and records no pack launch, so a step
    that skipped the hook would leave the replayed graph reading stale filters."""
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
    factory = nn.Shampoo_factory(learningRate=1e-4)
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
            assert torch.isfinite(to_torch(a.value)).all()
            assert_close(to_torch(a.value), to_torch(b.value).double(), 1e-6, f"state {i} after three replayed steps")
        lib.lamp_graph_release(g)
    finally:
        d = C.c_void_p(); lib.lamp_stream_get_default(0, C.byref(d)); lib.lamp_stream_set_current(d)
        lib.lamp_stream_release(st); lib.lamp_stream_release(d)
