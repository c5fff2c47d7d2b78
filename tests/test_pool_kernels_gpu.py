"""Every kernel of kernels/pool.hip against ATen's float64 operators on the inputs AFTER rounding to the dtype under test.

  global average (kernel == the whole square plane, stride 1, no padding; the kernel size is ONE integer, so a 2 x 4 plane cannot be
  pooled globally and the 16-byte plane is f32's 2 x 2)
      avg_pool_global_vec(_bwd)   planes of lpp = 1, 2, 4 .. 64 packets of 16 bytes, lpp lanes per plane: 2 x 2, 4 x 4, 8 x 8, 16 x 16
                                  give 1, 4, 16, 64 (f32), 2, 8, 32 (bf16 from 4 x 4 on; f64 up to 8 x 8)
      avg_pool_global(_bwd)       a wave per plane: everything else - 7 x 7, 12 x 12, f64's 16 x 16 (128 packets), bf16's 2 x 2
                                  (8 bytes), a misaligned input
  avg_pool(_bwd), max_pool(_bwd)  a thread per output (backward: per input, gathering): non-square maps, stride > kernel, padding,
                                  ceil_mode, count_include_pad, dilation
  max_pool1d(_bwd)                the same over [N, C, L]
Each test asserts the tag of the form it was written for through the kernel timers.  Tolerances are test_pooling's
(tests/test_ops_gpu.py): FWD_TOL * 2 for averages and gradients, indices and maxima bit-exact (first maximum in row-major order, NaN wins,
a window of -inf keeps its first element).  Probes: a plane whose only non-zero element is H * W averages to exactly 1, so a lane that
reads another plane's packet (a wrong t / lpp) shows as a 0 or a 2; integer gradients make the max-pool backward exact."""
import ctypes as C

import pytest
import torch

from lamp_amd import sten as S
from lamp_amd._capi import lib
from tests.form_ref import ITEM, aligned, dtid, equal_bits, launched, misaligned, small_ints
from tests.util import DTYPES, FWD_TOL, assert_close, closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu
aten = torch.ops.aten
F64 = torch.float64


def _avg(X, k, s, p, ceil, cip):
    o = C.c_void_p()
    lib.lamp_avg_pool2d(C.byref(o), X, k, s, p, ceil, cip)
    return to_torch(S.STen(o))


def _avg_bwd(G, X, k, s, p, ceil, cip):
    o = C.c_void_p()
    lib.lamp_avg_pool2d_backward(C.byref(o), G, X, k, s, p, ceil, cip)
    return to_torch(S.STen(o))


def _lanes(side, dt):
    """lanes per plane of the packet forms, 0: the wave-per-plane forms (global_pool_lanes in kernels/pool.hip)"""
    nbytes = side * side * ITEM[dt]
    lpp = nbytes // 16
    return lpp if nbytes % 16 == 0 and 1 <= lpp <= 64 and lpp & (lpp - 1) == 0 else 0


def _one_tag(L, tag, family):
    ran = {t: L.count(t) for t in L if t.startswith(family)}
    assert ran == {tag: 1}, f"launched {ran}, written for {tag}"


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("side", [2, 4, 8, 16, 7, 12])
def test_global_average_pool_forms(gpu, dt, side):
    """plane counts: 1, 37 (a partly filled workgroup of any lpp <= 4, several for the others), one that fills a workgroup exactly (256 /
    lpp planes, 4 for the wave-per-plane form) and that plus one"""
    lpp, hw = _lanes(side, dt), side * side
    per_group = 256 // lpp if lpp else 4
    fwd, bwd = ("avg_pool_global_vec", "avg_pool_global_vec_bwd") if lpp else ("avg_pool_global", "avg_pool_global_bwd")
    tol = FWD_TOL[dt] * 2
    for planes in sorted({1, 37, per_group, per_group + 1}):
        shape = (1, planes, side, side)
        x = closed_form(shape, 3, 2.0, dt)
        X = aligned(x)
        with launched() as L:
            got = _avg(X, side, 1, 0, 0, 1)
        _one_tag(L, fwd, "avg_pool")
        assert_close(got, aten.avg_pool2d(x.double(), [side], [1], [0], False, True, None), tol, f"{planes} planes: average")
        gy = closed_form((1, planes, 1, 1), 9, 1.0, dt)
        with launched() as L:
            got = _avg_bwd(to_sten(gy), X, side, 1, 0, 0, 1)
        _one_tag(L, bwd, "avg_pool")
        assert_close(got, aten.avg_pool2d_backward(gy.double(), x.double(), [side], [1], [0], False, True, None), tol, f"{planes} planes: backward")
        # probes: one element of value H * W per plane, each plane at another position: every average is exactly 1 ...
        hot = torch.zeros(planes, hw, dtype=dt)
        hot[torch.arange(planes), (torch.arange(planes) * 7) % hw] = float(hw)
        got = _avg(aligned(hot.reshape(shape)), side, 1, 0, 0, 1)
        assert torch.equal(got.double(), torch.ones(1, planes, 1, 1, dtype=F64)), f"{planes} planes: averages {got.reshape(-1).tolist()}"
        # ... and with only the first, the middle and the last plane non-zero the result is exactly one-hot there, forward and backward
        keep = torch.zeros(planes, 1, dtype=dt)
        keep[[0, planes // 2, planes - 1]] = 1.0
        got = _avg(aligned((hot * keep).reshape(shape)), side, 1, 0, 0, 1)
        assert torch.equal(got.reshape(-1).double(), keep.reshape(-1).double()), f"{planes} planes: averages {got.reshape(-1).tolist()}"
        got = _avg_bwd(to_sten((keep * hw).reshape(1, planes, 1, 1)), X, side, 1, 0, 0, 1)
        assert torch.equal(got.reshape(planes, hw).double(), keep.double().expand(planes, hw)), f"{planes} planes: backward of a one-hot gradient"


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("side", [4, 8])
def test_global_average_pool_misaligned(gpu, dt, side):
    """a contiguous input one element past a 16-byte boundary takes the wave-per-plane form; a misaligned gradient does not matter to the
    backward, whose packets are stores into a fresh tensor"""
    assert _lanes(side, dt) > 0
    shape = (3, 5, side, side)
    x = closed_form(shape, 3, 2.0, dt)
    ref = aten.avg_pool2d(x.double(), [side], [1], [0], False, True, None)
    for put, tag in ((aligned, "avg_pool_global_vec"), (misaligned, "avg_pool_global")):
        with launched() as L:
            got = _avg(put(x), side, 1, 0, 0, 1)
        _one_tag(L, tag, "avg_pool")
        assert_close(got, ref, FWD_TOL[dt] * 2, tag)
    gy = closed_form((3, 5, 1, 1), 9, 1.0, dt)
    with launched() as L:
        got = _avg_bwd(misaligned(gy), aligned(x), side, 1, 0, 0, 1)
    _one_tag(L, "avg_pool_global_vec_bwd", "avg_pool")
    assert_close(got, aten.avg_pool2d_backward(gy.double(), x.double(), [side], [1], [0], False, True, None), FWD_TOL[dt] * 2, "backward")


SHAPES = [(2, 3, 9, 14), (1, 2, 7, 5)]
KSP = [(2, 2, 0), (3, 2, 1), (3, 1, 1), (2, 3, 0), (5, 2, 2), (1, 1, 0)]


def _ksp_id(v):
    return "k%d-s%d-p%d" % v


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("shape", SHAPES, ids=["9x14", "7x5"])
@pytest.mark.parametrize("ksp", KSP, ids=_ksp_id)
def test_windowed_average_pool(gpu, dt, shape, ksp):
    k, s, p = ksp
    x = closed_form(shape, 3, 2.0, dt)
    X, xd = to_sten(x), x.double()
    tol = FWD_TOL[dt] * 2
    for ceil in (0, 1):
        for cip in (0, 1):
            what = f"ceil_mode={ceil} count_include_pad={cip}"
            ref = aten.avg_pool2d(xd, [k], [s], [p], bool(ceil), bool(cip), None)
            with launched() as L:
                got = _avg(X, k, s, p, ceil, cip)
            _one_tag(L, "avg_pool", "avg_pool")
            assert_close(got, ref, tol, f"{what}: average")
            gy = closed_form(tuple(ref.shape), 9, 1.0, dt) + 1.0            # positive: a covered input's gradient cannot cancel to 0
            refb = aten.avg_pool2d_backward(gy.double(), xd, [k], [s], [p], bool(ceil), bool(cip), None)
            with launched() as L:
                got = _avg_bwd(to_sten(gy), X, k, s, p, ceil, cip)
            _one_tag(L, "avg_pool_bwd", "avg_pool")
            assert_close(got, refb, tol, f"{what}: backward")
            assert torch.equal(got == 0, refb == 0), f"{what}: the inputs no window covers must get exactly 0"
            if s > k and not ceil:
                assert int((refb == 0).sum()) > 0


def _special(shape, dt):
    """quarter steps in [-1, 1] (every window holds tied maxima), one NaN, a 6 x 6 corner (6 wide in 1-D) of -inf: every window of up
    to 3 x 3 that lies in it is all -inf"""
    x = (closed_form(shape, 3, 2.0, F64) * 4).round() / 4
    if len(shape) == 4:
        x[..., :6, :6] = float("-inf")
    else:
        x[..., :6] = float("-inf")
    x.reshape(-1)[x.numel() - 11] = float("nan")
    return x.to(dt)


DIL = [1, 2]


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("shape", SHAPES, ids=["9x14", "7x5"])
@pytest.mark.parametrize("ksp", KSP, ids=_ksp_id)
def test_max_pool(gpu, dt, shape, ksp):
    k, s, p = ksp
    for x in (closed_form(shape, 3, 2.0, dt), _special(shape, dt)):
        X, xd = to_sten(x), x.double()
        for d in DIL:
            for ceil in (0, 1):
                what = f"dilation={d} ceil_mode={ceil}"
                ref, idx = aten.max_pool2d_with_indices(xd, [k], [s], [p], [d], bool(ceil))
                o, i = C.c_void_p(), C.c_void_p()
                with launched() as L:
                    lib.lamp_max_pool2d_with_indices(C.byref(o), C.byref(i), X, k, s, p, d, ceil)
                _one_tag(L, "max_pool", "max_pool")
                O, I = S.STen(o), S.STen(i)
                assert torch.equal(to_torch(I), idx), f"{what}: indices"
                assert equal_bits(to_torch(O), ref), f"{what}: maxima"
                # integers 1 .. 7: at most k * k of them meet in one input, so every sum is exact in every dtype
                for exact, gy in ((True, small_ints(tuple(ref.shape), 9, dt) + 4.0), (False, closed_form(tuple(ref.shape), 9, 1.0, dt))):
                    refb = aten.max_pool2d_with_indices_backward(gy.double(), xd, [k], [s], [p], [d], bool(ceil), idx)
                    o = C.c_void_p()
                    with launched() as L:
                        lib.lamp_max_pool2d_with_indices_backward(C.byref(o), to_sten(gy), X, k, s, p, d, ceil, I)
                    _one_tag(L, "max_pool_bwd", "max_pool")
                    got = to_torch(S.STen(o))
                    assert_close(got, refb, FWD_TOL[dt] * 2, f"{what}: backward")
                    if exact:
                        assert torch.equal(got.double(), refb), f"{what}: backward of an integer gradient"
                        assert torch.equal(got == 0, refb == 0), f"{what}: only the maxima receive a gradient"


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("ksp", KSP, ids=_ksp_id)
def test_max_pool1d(gpu, dt, ksp):
    k, s, p = ksp
    shape = (2, 3, 37)
    for x in (closed_form(shape, 3, 2.0, dt), _special(shape, dt)):
        X, xd = to_sten(x), x.double()
        for d in DIL:
            for ceil in (0, 1):
                what = f"dilation={d} ceil_mode={ceil}"
                ref, idx = aten.max_pool1d_with_indices(xd, [k], [s], [p], [d], bool(ceil))
                o, i = C.c_void_p(), C.c_void_p()
                with launched() as L:
                    lib.lamp_max_pool1d_with_indices(C.byref(o), C.byref(i), X, k, s, p, d, ceil)
                _one_tag(L, "max_pool1d", "max_pool")
                O, I = S.STen(o), S.STen(i)
                assert torch.equal(to_torch(I), idx), f"{what}: indices"
                assert equal_bits(to_torch(O), ref), f"{what}: maxima"
                gy = small_ints(tuple(ref.shape), 9, dt) + 4.0
                # ATen's own backward of the 1-D pool is the 2-D one over [N, C, 1, L]
                refb = aten.max_pool2d_with_indices_backward(gy.double().unsqueeze(2), xd.unsqueeze(2), [1, k], [1, s], [0, p], [1, d], bool(ceil),
                                                             idx.unsqueeze(2)).squeeze(2)
                o = C.c_void_p()
                with launched() as L:
                    lib.lamp_max_pool1d_with_indices_backward(C.byref(o), to_sten(gy), X, k, s, p, d, ceil, I)
                _one_tag(L, "max_pool1d_bwd", "max_pool")
                assert torch.equal(to_torch(S.STen(o)).double(), refb), f"{what}: backward"
