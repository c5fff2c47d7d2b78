"""Every kernel form of layer norm, softmax / log-softmax and the row-broadcast elementwise launcher against plain float64 formulas.

The host picks a form from the row width D, the element size and the pointer alignment (W = 16 / sizeof(T) elements per 16-byte packet,
npk = D / W packets per row):
  layer norm   ln_fwd_vec_kernel / ln_bwd_dx_vec_kernel<MAXP 1, 2, 4, 8> for npk <= 64, 128, 256, 512; the scalar Welford kernels when
               D % W != 0, npk > 512 or a pointer is not 16-byte aligned; ln_bwd_dwdb_vec_kernel / ln_bwd_dwdb_kernel on alignment and
               D % W alone, rows split nsplit <= 256 ways
  softmax      softmax_fwd_vec_kernel<MAXP 1, 2, 4, 8> in registers, <0> streaming for npk > 512; the strided softmax_fwd_kernel when
               inner != 1, D % W != 0, D < 32 W or misaligned; log_softmax_bwd_vec_kernel / log_softmax_bwd_kernel on the same condition
  elementwise  ew_rowvec_kernel (dense / row vector / one element inputs over [R, N], N % W == 0), ew_vec_kernel (flat), ew_strided_kernel
The reference (tests/row_ref.py, verified on the CPU by tests/test_row_ref.py) is evaluated in float64 on the inputs AFTER rounding to the
dtype under test, so the tolerances only have to cover the kernel's own arithmetic: they are the ones of test_layer_norm,
test_log_softmax_and_nll and test_binary_broadcast_and_inplace.  Those are relative to the mean magnitude of a tensor, which hides a
reduction that loses one packet of a long row; the one-hot probes put the whole weight of a row on one position at a time instead."""
import ctypes as C
import math

import pytest
import torch

from lamp_amd import sten as S
from lamp_amd._capi import lib, i64_array
from tests import row_ref as R
from tests.util import DTYPES, FWD_TOL, assert_close, closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
ITEM = {F64: 8, F32: 4, BF16: 2}
EPS = 1e-5
LN_BWD_TOL = {F64: 1e-10, F32: 2e-4, BF16: 4e-2}      # test_layer_norm's


def _dtid(dt):
    return str(dt).replace("torch.", "")


def _W(dt):
    return 16 // ITEM[dt]


def _width(dt, spec):
    """spec = (npk, plus): D = npk * W + plus"""
    return spec[0] * _W(dt) + spec[1]


def _wid(spec):
    return f"{spec[0]}W+{spec[1]}" if spec[1] else f"{spec[0]}W"


def _misaligned(t):
    """t's values as a CONTIGUOUS device view whose data pointer is one element past a 16-byte boundary: element 1.. of a 1-D tensor of
    numel + 1 elements.  Every vector form has to decline it."""
    base = to_sten(torch.cat([t.new_zeros(1), t.reshape(-1)]))
    v = base.narrow(0, 1, t.numel()).view(*t.shape)
    assert base.data_ptr % 16 == 0 and v.data_ptr % 16 == ITEM[t.dtype] and v.is_contiguous()
    return v


def _aligned(t):
    a = to_sten(t)
    assert a.data_ptr % 16 == 0
    return a


def _positions(D, W):
    """first / last element of the first packet, of lane 63's and lane 0's second packet, of the last register-resident packet and the
    first streamed one, and of the row's last packet"""
    return [p for p in sorted({0, W - 1, W, 64 * W - 1, 64 * W, 512 * W - 1, 512 * W, D - W, D - 1}) if 0 <= p < D]


def _one_hot(pos, D, dt, value=1.0):
    x = torch.zeros(len(pos), D, dtype=dt)
    x[torch.arange(len(pos)), torch.tensor(pos)] = value
    return x


# ---- layer norm ---------------------------------------------------------------------------------------------------------------------------
def _ln_fwd(X, norm, Wt, Bt):
    out = (C.c_void_p * 3)()
    lib.lamp_native_layer_norm(out, X, i64_array(norm), len(norm), Wt, Bt, EPS)
    return [to_torch(S.STen(out[i])) for i in range(3)]


def _ln_bwd(G, X, norm, Mean, Rstd, Wt, Bt):
    out = (C.c_void_p * 3)()
    lib.lamp_native_layer_norm_backward(out, G, X, i64_array(norm), len(norm), Mean, Rstd, Wt, Bt,
                                        (C.c_uint8 * 3)(1, int(Wt is not None), int(Bt is not None)))
    return [to_torch(S.STen(out[i])) if out[i] else None for i in range(3)]


def _ln_inputs(M, D, dt, affine=True):
    """x: closed form in [-2, 2] plus 3 + row % 5 (a row mean of 3 .. 7 against a deviation of 1.15: a variance computed as
    E[x^2] - mean^2 would show), rounded to dt; w, b, gy as in test_layer_norm"""
    x = (closed_form((M, D), 3, 4.0, F64) + 3.0 + (torch.arange(M, dtype=F64) % 5)[:, None]).to(dt)
    w = closed_form((D,), 1, 1.0, dt) + 1.0 if affine else None
    b = closed_form((D,), 5, 1.0, dt) if affine else None
    gy = closed_form((M, D), 13, 2.0, dt)
    return x, gy, w, b


def _check_ln(dt, x, gy, w, b, X=None, G=None, what=""):
    """forward and backward of one input against the reference.  x, gy, w, b are CPU tensors in dt and may have any leading shape; w's
    shape is normalized_shape.  X / G: the device tensors to hand over when they are not plain copies of x / gy."""
    norm = list(w.shape) if w is not None else [x.shape[-1]]
    X = X if X is not None else to_sten(x)
    G = G if G is not None else to_sten(gy)
    Wt = to_sten(w) if w is not None else None
    Bt = to_sten(b) if b is not None else None
    y, mean, rstd = _ln_fwd(X, norm, Wt, Bt)
    ry, rmean, rrstd = R.layer_norm(x, w, b, EPS, len(norm))
    tol = FWD_TOL[dt] * 4
    assert_close(y, ry, tol, f"{what} ln y")
    assert_close(mean, rmean, tol, f"{what} ln mean")
    assert_close(rstd, rrstd, tol, f"{what} ln rstd")
    # the backward is handed the reference's statistics rounded to dt, and the reference formula takes the same rounded values
    m_dt, r_dt = rmean.to(dt), rrstd.to(dt)
    dx, dw, db = _ln_bwd(G, X, norm, to_sten(m_dt), to_sten(r_dt), Wt, Bt)
    rdx, rdw, rdb = R.layer_norm_backward(gy, x, m_dt, r_dt, w, len(norm))
    btol = LN_BWD_TOL[dt]
    assert_close(dx, rdx, btol, f"{what} ln dx")
    if w is not None:
        assert_close(dw, rdw, btol, f"{what} ln dweight")
        assert_close(db, rdb, btol, f"{what} ln dbias")
    else:
        assert dw is None and db is None
    return {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dw": dw, "db": db}


# every MAXP boundary (64, 128, 256, 512 packets) from both sides, the too-long scalar fallback (513), D % W != 0 next to MAXP 1, 2 and
# the fallback, and the two tiny rows of the known-answer tests
LN_WIDTHS = [(n, 0) for n in (1, 63, 64, 65, 128, 129, 256, 257, 511, 512, 513)] + [(1, 1), (64, 1), (512, 1), (0, 1), (0, 3)]


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("width", LN_WIDTHS, ids=_wid)
def test_layer_norm_forms(gpu, dt, affine, width):
    """M = 5: the second four-row workgroup holds one row"""
    x, gy, w, b = _ln_inputs(5, _width(dt, width), dt, affine)
    _check_ln(dt, x, gy, w, b)


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("npk", [64, 512], ids=["maxp1", "maxp8"])
def test_layer_norm_misaligned_rows_take_the_scalar_form(gpu, dt, npk):
    x, gy, w, b = _ln_inputs(5, npk * _W(dt), dt)
    _check_ln(dt, x, gy, w, b, X=_aligned(x), G=_aligned(gy), what="aligned")
    _check_ln(dt, x, gy, w, b, X=_misaligned(x), G=_misaligned(gy), what="misaligned")


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
def test_layer_norm_two_normalized_dims(gpu, dt):
    x, gy, w, b = _ln_inputs(3, 96, dt)
    out = _check_ln(dt, x.reshape(3, 4, 24), gy.reshape(3, 4, 24), w.reshape(4, 24), b.reshape(4, 24))
    assert list(out["dw"].shape) == [4, 24] and list(out["db"].shape) == [4, 24] and list(out["mean"].shape) == [3, 1, 1]


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
def test_layer_norm_non_contiguous_input(gpu, dt):
    x, gy, w, b = _ln_inputs(5, 65 * _W(dt), dt)
    X = to_sten(x.t().contiguous()).transpose(0, 1)
    G = to_sten(gy.t().contiguous()).transpose(0, 1)
    assert not X.is_contiguous() and X.shape == list(x.shape)
    _check_ln(dt, x, gy, w, b, X=X, G=G)


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("M,plus", [(300, 0), (259, 1)], ids=["vec", "scalar"])
def test_layer_norm_row_split(gpu, dt, M, plus):
    """D = 3 W (+ 1): one block of columns, so the dweight / dbias pass splits the rows as many ways as it may (256 on an MI355X, where
    splits 0 .. 43, or 0 .. 2, then take two rows).  Nothing here depends on that number: any split of the rows has the same sums.
    Second input: gy is zero except rows 0, 255, 256 and M - 1 (the first and the last row of the first trip and of the second one with
    256 splits), each with ones in a band of columns of its own: dbias is exactly 1 inside a band and 0 outside, so a row that is
    skipped, or added twice, shows as a 0 or a 2."""
    D = 3 * _W(dt) + plus
    x, gy, w, b = _ln_inputs(M, D, dt)
    _check_ln(dt, x, gy, w, b)
    band = torch.zeros(M, D, dtype=dt)
    expect = torch.zeros(D, dtype=F64)
    for k, r in enumerate((0, 255, 256, M - 1)):
        lo, hi = k * D // 5, (k + 1) * D // 5
        assert hi > lo
        band[r, lo:hi] = 1.0
        expect[lo:hi] = 1.0
    assert expect[4 * D // 5:].sum().item() == 0.0
    out = _check_ln(dt, x, band, w, b, what="banded")
    assert torch.equal(out["db"].double(), expect), f"dbias {out['db'].tolist()}"


# npk, plus: full register files of each MAXP (the last `lane + 64 * i` of every lane is in use), a ragged MAXP 8, both scalar forms
LN_PROBES = {"maxp1": (64, 0), "maxp2": (128, 0), "maxp4": (256, 0), "maxp8": (512, 0), "maxp8-ragged": (257, 0), "scalar-long": (513, 0),
             "scalar-odd": (64, 1)}


@pytest.mark.parametrize("dt", [BF16, F32], ids=_dtid)
@pytest.mark.parametrize("form", list(LN_PROBES))
def test_layer_norm_every_position_counts(gpu, dt, form):
    """Row i is zero but for a 1 at position p_i.  As x: a reduction that misses p_i sees a constant row and answers mean 0 and
    rstd 1 / sqrt(eps) = 316 instead of 1 / D and about sqrt(D).  As gy (x from the main case): the two row sums of dx are w[p] / D and
    w[p] xhat[p] / D or, when p_i is missed, 0, which moves every other element of dx by its own size; dweight and dbias have one
    non-zero row per probed column."""
    W = _W(dt)
    D = _width(dt, LN_PROBES[form])
    pos = _positions(D, W)
    hot = _one_hot(pos, D, dt)
    x, gy, w, b = _ln_inputs(len(pos), D, dt)
    out = _check_ln(dt, hot, gy, w, b, what="one-hot x")
    assert out["rstd"].max().item() < 0.5 / math.sqrt(EPS)
    out = _check_ln(dt, x, hot, w, b, what="one-hot gy")
    assert torch.equal(out["db"].double(), hot.double().sum(0))


# ---- softmax, log-softmax, log-softmax backward ------------------------------------------------------------------------------------------------
def _lsm_bwd(G, O, dim):
    o = C.c_void_p()
    lib.lamp_log_softmax_backward_data(C.byref(o), G, O, dim)
    return to_torch(S.STen(o))


def _check_softmax(dt, x, dim, X=None, what=""):
    X = X if X is not None else to_sten(x)
    tol = FWD_TOL[dt]
    assert_close(to_torch(X.logSoftMax(dim)), R.log_softmax(x, dim), tol * (2 if dt == BF16 else 1), f"{what} log_softmax")
    assert_close(to_torch(X.softmax(dim)), R.softmax(x, dim), tol, f"{what} softmax")


def _check_lsm_bwd(dt, g, out, dim, G=None, O=None, what=""):
    got = _lsm_bwd(G if G is not None else to_sten(g), O if O is not None else to_sten(out), dim)
    assert_close(got, R.log_softmax_backward(g, out, dim), FWD_TOL[dt] * 4, f"{what} log_softmax backward")


def _sm_inputs(shape, dim, dt):
    """x, g, and out = the reference log-softmax rounded to dt (what the backward is handed in training)"""
    x = closed_form(shape, 3, 8.0, dt)
    return x, closed_form(shape, 8, 1.0, dt), R.log_softmax(x, dim).to(dt)


# 31: below D >= 32 W, scalar; 32 .. 512: MAXP 1, 2, 4, 8 from both sides of each boundary; 513: streaming with one lane on a ninth trip;
# 1500: streaming, 23.4 trips; 1500 W + 1: long and scalar
SM_WIDTHS = [(n, 0) for n in (31, 32, 64, 65, 128, 129, 256, 257, 512, 513, 1500)] + [(1500, 1)]


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("width", SM_WIDTHS, ids=_wid)
def test_softmax_forms(gpu, dt, width):
    x, g, out = _sm_inputs((5, _width(dt, width)), 1, dt)
    _check_softmax(dt, x, 1)
    _check_lsm_bwd(dt, g, out, 1)


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("shape,dim", [((70, 65), 0), ((3, 200, 67), 1), ((3, 200, 67), -1)], ids=["dim0", "middle", "last"])
def test_softmax_strided_form(gpu, dt, shape, dim):
    """outer > 1, inner > 64 (more than one wave of rows per outer index), D > 64 (a second trip of the lanes); dim = -1 of an odd width"""
    x, g, out = _sm_inputs(shape, dim, dt)
    _check_softmax(dt, x, dim)
    _check_lsm_bwd(dt, g, out, dim)


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("npk", [64, 513], ids=["maxp1", "streaming"])
def test_softmax_misaligned_rows_take_the_scalar_form(gpu, dt, npk):
    x, g, out = _sm_inputs((5, npk * _W(dt)), 1, dt)
    _check_softmax(dt, x, 1, X=_aligned(x), what="aligned")
    _check_softmax(dt, x, 1, X=_misaligned(x), what="misaligned")
    _check_lsm_bwd(dt, g, out, 1, G=_aligned(g), O=_aligned(out), what="aligned")
    _check_lsm_bwd(dt, g, out, 1, G=_misaligned(g), O=_misaligned(out), what="misaligned")


SM_FORMS = {"scalar": (31, 0), "maxp1": (64, 0), "maxp8": (512, 0), "streaming": (513, 0)}


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("form", list(SM_FORMS))
def test_softmax_special_values(gpu, dt, form):
    """one entry of 60 (everything else underflows against it unless the maximum is subtracted), every third entry -inf (log-softmax -inf,
    softmax 0 there), equal entries, all -inf (NaN, as ATen).  assert_close compares the non-finite pattern before the values; that the
    reference's pattern is ATen's is also pinned on the CPU (tests/test_row_ref.py)."""
    x = R.special_rows(_width(dt, SM_FORMS[form]), dt)
    for mine, theirs in ((R.log_softmax, torch.ops.aten._log_softmax), (R.softmax, torch.ops.aten._softmax)):
        ref, own = mine(x, 1), theirs(x, 1, False).double()
        assert torch.equal(torch.isnan(own), torch.isnan(ref)) and torch.equal(torch.isinf(own), torch.isinf(ref))
    _check_softmax(dt, x, 1)


SM_PROBES = {"scalar": (31, 0), "maxp1": (64, 0), "maxp2": (128, 0), "maxp4": (256, 0), "maxp8": (512, 0), "streaming-ragged": (513, 0),
             "streaming": (1500, 0), "scalar-long": (1500, 1)}


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("form", list(SM_PROBES))
def test_softmax_every_position_counts(gpu, dt, form):
    """Forward: row i is 0 but for 20 at p_i, so softmax is 1 - (D - 1) e^-20 there and e^-20 elsewhere; with p_i missed by the maximum or
    by the sum it is 1 / D everywhere else.  Backward: g is one-hot at p_i against the uniform out = -log D: -1 / D off the position and
    0 when the sum misses it."""
    D = _width(dt, SM_PROBES[form])
    pos = _positions(D, _W(dt))
    _check_softmax(dt, _one_hot(pos, D, dt, 20.0), 1)
    out = torch.full((len(pos), D), -math.log(D), dtype=F64).to(dt)
    _check_lsm_bwd(dt, _one_hot(pos, D, dt), out, 1)


# ---- elementwise: row vector, flat and strided forms ----------------------------------------------------------------------------------------------
def _check_row_broadcast(dt, N, dense):
    """the expressions of a bias / scale over a token batch [7, N]; dense(t) puts the dense operand on the device"""
    Rn = 7
    tol = FWD_TOL[dt]
    x = closed_form((Rn, N), 1, 4.0, dt)
    bias = closed_form((N,), 50, 3.0, dt) + 1.6
    scale = closed_form((1, N), 9, 2.0, dt)
    one = torch.tensor([1.75], dtype=dt)
    xd, bd, sd, od = x.double(), bias.double(), scale.double(), one.double()
    Bi, Sc, One = to_sten(bias), to_sten(scale), to_sten(one)
    assert_close(to_torch(dense(x) + Bi), xd + bd, tol, "x + bias[N]")
    assert_close(to_torch(Bi + dense(x)), bd + xd, tol, "bias[N] + x")
    assert_close(to_torch(dense(x) * Sc), xd * sd, tol, "x * scale[1, N]")
    O = dense(x)
    S.STen.addcmulOut(O, O, Bi, One, 0.3)
    assert_close(to_torch(O), xd + 0.3 * bd * od, tol, "addcmul(dense, row, one)")
    O = dense(x)
    S.STen.addcdivOut(O, O, Bi, One, -0.7)
    assert_close(to_torch(O), xd - 0.7 * bd / od, tol, "addcdiv(dense, row, one)")
    O = dense(torch.zeros_like(x))
    S.STen.addcmulOut(O, Bi, One, dense(x), 0.3)
    assert_close(to_torch(O), bd + 0.3 * od * xd, tol, "addcmul(row, one, dense)")
    xb = x + 1.0 + x.abs()                              # a divisor away from zero
    O = dense(torch.zeros_like(x))
    S.STen.addcdivOut(O, One, Bi, dense(xb), -0.7)
    assert_close(to_torch(O), od - 0.7 * bd / xb.double(), tol, "addcdiv(one, row, dense)")
    X = dense(x)
    X += Bi
    assert_close(to_torch(X), xd + bd, tol, "x += bias")


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
@pytest.mark.parametrize("config", ["rowvec", "strided", "misaligned"])
def test_elementwise_row_broadcast(gpu, dt, config):
    """N = 12 W aligned: ew_rowvec_kernel.  N = 12 W + 1, and the aligned width behind a misaligned pointer: ew_strided_kernel, which has to
    agree."""
    N = 12 * _W(dt) + (1 if config == "strided" else 0)
    _check_row_broadcast(dt, N, _misaligned if config == "misaligned" else _aligned)


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
def test_elementwise_row_broadcast_second_grid_trip(gpu, dt):
    """[1027, 513 W] is 526 851 packets, just over the 2048 x 256 threads of the capped grid (8 blocks per CU, 256 CUs): the first 2 563
    threads take a second packet, whose column is no longer the thread's first one (513 does not divide the grid's stride)"""
    Rn, N = 1027, 513 * _W(dt)
    x = closed_form((Rn, N), 1, 4.0, dt)
    bias = closed_form((N,), 50, 3.0, dt) + 1.6
    assert_close(to_torch(_aligned(x) + to_sten(bias)), x.double() + bias.double(), FWD_TOL[dt], "x + bias[N]")


@pytest.mark.parametrize("dt", DTYPES, ids=_dtid)
def test_elementwise_flat_second_grid_trip_and_tail(gpu, dt):
    """2048 x 256 + 1 whole packets (a second trip for thread 0) and a scalar tail of 3 elements (1 for f64)"""
    W = _W(dt)
    n = 2048 * 256 * W + W + 3
    a = closed_form((n,), 1, 4.0, dt)
    b = closed_form((n,), 50, 3.0, dt)
    assert_close(to_torch(_aligned(a).add(_aligned(b), 0.25)), a.double() + 0.25 * b.double(), FWD_TOL[dt], "a + 0.25 b")
