"""The Cholesky family on the GPU (kernels/linalg.hip): lamp_linalg_cholesky, lamp_cholesky_solve, lamp_cholesky_inverse,
lamp_triangular_solve in f32 and f64, at every form boundary (sides 1, 2, 3, 31, 32, 33, S - 1, S, S + 1 and the blocked 2 NB + S + 1 with
its ragged last panel; S = the LDS side, NB = the block column, both read from the plan).

Inputs: A = M M^T / n + I (condition number about 5), triangles tril / triu(randn) + 3 I, from fixed seeds (tests/linalg_ref.py).

Backward error against the textbook bounds, which hold for any order of summation (Higham, Accuracy and Stability of Numerical
Algorithms, theorems 10.3 and 8.5), residuals evaluated in f64 on the host, the factor 2 for that evaluation's own rounding:
    |A - L L^T| <= 2 gamma(n + 1) |L| |L|^T        |T x - b| <= 2 gamma(n) |T| |x|        gamma(k) = k u / (1 - k u)
cholesky_solve and cholesky_inverse are forward results; they are held to 8 x the distance torch-CPU's own result in the same dtype
keeps from a result one precision up on the same inputs (the order of summation differs, the algorithm does not): f32 against
linalg_ref in f64 as the rule is stated; for f64 that distance would be zero by construction, so f64 is measured against the same two
substitutions in x87 extended precision (numpy longdouble).  With very few elements the measured distance is one draw of a rounding
error, so sides up to 3 are measured on a batch of 65.  Figures: BASELINE.md section 21; every case prints its own (-s).

Exact properties: the other triangle is bitwise 0, inputs are never written, two runs agree bitwise, a batch equals its matrices run
alone, the upper factor is the transposed lower one, garbage in a triangle that is not read changes nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from lamp_amd import sten as S
from lamp_amd._capi import LampError, lib
from tests import linalg_ref as R
from tests.util import to_sten, to_torch

pytestmark = pytest.mark.gpu

LDS_SIDE = R.linalg_plan("linalg_cholesky", torch.float64, [4, 4])["lds_side"]
NB = R.linalg_plan("linalg_cholesky", torch.float64, [LDS_SIDE + 1, LDS_SIDE + 1])["nb"]
BLOCKED = 2 * NB + LDS_SIDE + 1
SIDES = [1, 2, 3, 31, 32, 33, LDS_SIDE - 1, LDS_SIDE, LDS_SIDE + 1, BLOCKED]
DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]
CASES = [(n, b) for n in SIDES for b in (1, 3, 65) if b < 65 or n <= 33]
CASE_IDS = [f"n{n}-b{b}" for n, b in CASES]
FLAGS = [(u, t, d) for u in (0, 1) for t in (0, 1) for d in (0, 1)]


def bshape(batch):
    return () if batch == 1 else (batch,)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def chol(a, upper=0, device=0):
    h = to_sten(a, device)
    out = to_torch(h.cholesky(upper))
    assert same_bits(to_torch(h), a), "the input was written"
    return out


def tri_solve(b, a, upper, trans, unit, device=0):
    hb, ha = to_sten(b, device), to_sten(a, device)
    out = to_torch(S.STen.triangularSolve(hb, ha, upper, trans, unit))
    assert same_bits(to_torch(hb), b) and same_bits(to_torch(ha), a), "an input was written"
    return out


def chol_solve(b, f, upper, device=0):
    hb, hf = to_sten(b, device), to_sten(f, device)
    out = to_torch(hb.choleskySolve(hf, upper))
    assert same_bits(to_torch(hb), b) and same_bits(to_torch(hf), f), "an input was written"
    return out


def chol_inverse(f, upper, device=0):
    hf = to_sten(f, device)
    out = to_torch(hf.choleskyInverse(upper))
    assert same_bits(to_torch(hf), f), "the input was written"
    return out


def garbage(t, keep_upper):
    """t with the triangle that must not be read filled with NaN, infinities and huge numbers"""
    n = t.shape[-1]
    junk = torch.tensor([float("nan"), float("inf"), -1e30, 7.0], dtype=t.dtype).repeat(n * n // 4 + 1)[: n * n].reshape(n, n)
    mask = torch.ones(n, n, dtype=torch.bool).triu(1) if not keep_upper else torch.ones(n, n, dtype=torch.bool).tril(-1)
    return torch.where(mask, junk, t)


def op_of(tri, upper, trans, unit):
    """the matrix the solve works with, in f64: the named triangle only, a unit diagonal when asked, transposed when asked"""
    t = (tri.double().triu() if upper else tri.double().tril())
    if unit:
        n = t.shape[-1]
        t = t - torch.diag_embed(torch.diagonal(t, 0, -2, -1)) + torch.eye(n, dtype=torch.float64)
    return t.transpose(-1, -2) if trans else t


# ---- factorisation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n,batch", CASES, ids=CASE_IDS)
def test_cholesky_backward_error_and_exact_properties(gpu, dt, n, batch):
    a = R.spd(n, bshape(batch), dtype=dt)
    a64 = a.double()
    low = chol(a, 0)
    up = chol(a, 1)
    assert low.dtype == dt and low.shape == a.shape
    for name, f, fft, absfft in (("lower", low, low.double() @ low.double().transpose(-1, -2), low.double().abs() @ low.double().abs().transpose(-1, -2)),
                                 ("upper", up, up.double().transpose(-1, -2) @ up.double(), up.double().abs().transpose(-1, -2) @ up.double().abs())):
        excess = ((a64 - fft).abs() / (2 * R.gamma(n + 1, dt) * absfft)).max().item()
        print(f"cholesky {name} n={n} batch={batch} {dt}: residual / bound = {excess:.3f}")
        assert excess <= 1.0, (name, excess)
    # the other triangle is bitwise +0
    assert same_bits(low, low.tril()) and same_bits(up, up.triu())
    # the upper factor is the transposed lower one: the same arithmetic on the same triangle
    assert same_bits(up, low.transpose(-1, -2).contiguous())
    # two runs agree bitwise
    assert same_bits(chol(a, 0), low)
    # a batch equals its matrices run one at a time
    if batch == 3:
        for k in range(3):
            assert same_bits(chol(a[k], 0), low[k]) and same_bits(chol(a[k], 1), up[k])


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [3, 33, LDS_SIDE, BLOCKED])
def test_cholesky_reads_one_triangle(gpu, dt, n):
    a = R.spd(n, (3,), dtype=dt)
    assert same_bits(chol(garbage(a, keep_upper=False), 0), chol(a, 0))
    assert same_bits(chol(garbage(a, keep_upper=True), 1), chol(a, 1))


def test_cholesky_takes_strided_input(gpu):
    a = R.spd(33, (3,), dtype=torch.float64)
    h = to_sten(a.transpose(-1, -2).contiguous()).transpose(1, 2)        # a itself, as a view with a unit ROW stride
    assert same_bits(to_torch(h.choleskyLower()), chol(a, 0))


# ---- triangular solve --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n,batch", CASES, ids=CASE_IDS)
def test_triangular_solve_backward_error(gpu, dt, n, batch):
    worst = 0.0
    for nrhs in (1, 3, 65):
        b = R.rhs(n, nrhs, bshape(batch), dtype=dt)
        for upper, trans, unit in FLAGS:
            tri = R.triangle(n, bshape(batch), upper=bool(upper), dtype=dt)
            x = tri_solve(b, tri, upper, trans, unit)
            assert x.dtype == dt and x.shape == b.shape
            t = op_of(tri, upper, trans, unit)
            den = 2 * R.gamma(n, dt) * (t.abs() @ x.double().abs())
            res = (t @ x.double() - b.double()).abs()
            assert bool((res[den == 0] == 0).all())
            excess = (res[den > 0] / den[den > 0]).max().item() if bool((den > 0).any()) else 0.0
            worst = max(worst, excess)
            assert excess <= 1.0, (nrhs, upper, trans, unit, excess)
    print(f"triangular_solve n={n} batch={batch} {dt}: worst residual / bound over 3 widths x 8 flag sets = {worst:.3f}")


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [3, 33, LDS_SIDE, BLOCKED])
def test_triangular_solve_exact_properties(gpu, dt, n):
    b = R.rhs(n, 3, (3,), dtype=dt)
    for upper, trans, unit in FLAGS:
        tri = R.triangle(n, (3,), upper=bool(upper), dtype=dt)
        x = tri_solve(b, tri, upper, trans, unit)
        assert same_bits(tri_solve(b, tri, upper, trans, unit), x)                                    # two runs
        assert same_bits(tri_solve(b, garbage(tri, keep_upper=bool(upper)), upper, trans, unit), x)   # only the named triangle is read
        if unit:                                                                                      # ... and not its diagonal
            d = tri.clone()
            torch.diagonal(d, 0, -2, -1).fill_(float("nan"))
            assert same_bits(tri_solve(b, d, upper, trans, unit), x)
        for k in range(3):                                                                            # a batch equals its matrices alone
            assert same_bits(tri_solve(b[k], tri[k], upper, trans, unit), x[k])


def test_triangular_solve_broadcasts_strides_and_clones(gpu):
    tri = R.triangle(33, (), dtype=torch.float64)
    b = R.rhs(33, 5, (4,), dtype=torch.float64)
    x = tri_solve(b, tri, 0, 0, 0)                                        # one triangle over a batch of right-hand sides
    for k in range(4):
        assert same_bits(tri_solve(b[k], tri, 0, 0, 0), x[k])
    tris = R.triangle(33, (4,), dtype=torch.float64)
    x = tri_solve(b[0], tris, 0, 1, 0)                                    # one right-hand side over a batch of triangles
    for k in range(4):
        assert same_bits(tri_solve(b[0], tris[k], 0, 1, 0), x[k])
    hb = to_sten(b[0].t().contiguous()).t                                 # a column-major right-hand side
    assert same_bits(to_torch(S.STen.triangularSolve(hb, to_sten(tri), 0, 0, 0)), tri_solve(b[0], tri, 0, 0, 0))
    sol, cl = C.c_void_p(), C.c_void_p()
    ha, hb4 = to_sten(tri), to_sten(b)                                    # (named: a temporary's handle dies before the call)
    lib.lamp_triangular_solve(C.byref(sol), C.byref(cl), hb4.h, ha.h, 0, 0, 0)
    sol, cl = S.STen(sol), S.STen(cl)
    assert cl.shape == [4, 33, 33] and same_bits(to_torch(cl), tri.expand(4, 33, 33).contiguous())   # ATen's cloned coefficient


def test_singular_triangle_gives_non_finite_values_not_an_error(gpu):
    tri = R.triangle(5, (), dtype=torch.float32)
    tri[2, 2] = 0.0
    x = tri_solve(R.rhs(5, 2, (), dtype=torch.float32), tri, 0, 0, 0)
    assert bool(torch.isfinite(x[:2]).all()) and not bool(torch.isfinite(x[2:]).all())


# ---- cholesky_solve, cholesky_inverse -----------------------------------------------------------------------------------------------
def _substitute(lower, b):
    """L y = b then L^T x = y in numpy longdouble (x87 extended precision)"""
    n = lower.shape[0]
    y = np.zeros_like(b)
    for i in range(n):
        y[i] = (b[i] - lower[i, :i] @ y[:i]) / lower[i, i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - lower[i + 1:, i] @ x[i + 1:]) / lower[i, i]
    return x


def precise_solve(b, f, upper):
    """the solution from the factor as given, one precision above its dtype: f64 for f32, longdouble for f64"""
    if f.dtype == torch.float32:
        return R.cholesky_solve(b.double(), f.double(), upper).numpy().astype(np.longdouble)
    fl = f.numpy().astype(np.longdouble).reshape(-1, f.shape[-1], f.shape[-1])
    bl = b.numpy().astype(np.longdouble).reshape(-1, b.shape[-2], b.shape[-1])
    out = np.stack([_substitute(np.tril(m.T if upper else m), r) for m, r in zip(fl, bl)])
    return out.reshape(b.shape)


FORWARD_CASES = [(n, b) for n in (1, 2, 3) for b in (65,)] + [(n, b) for n in (31, 32, 33) for b in (1, 3, 65)]


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("upper", [0, 1], ids=["lower", "upper"])
@pytest.mark.parametrize("n,batch", FORWARD_CASES, ids=[f"n{n}-b{b}" for n, b in FORWARD_CASES])
def test_cholesky_solve_and_inverse_against_cpu_distance(gpu, dt, upper, n, batch):
    f = torch.linalg.cholesky(R.spd(n, bshape(batch)), upper=bool(upper)).to(dt)
    for nrhs in (1, 3, 65):
        b = R.rhs(n, nrhs, bshape(batch), dtype=dt)
        ref = precise_solve(b, f, upper)
        cpu = np.abs(R.cholesky_solve(b, f, upper).numpy().astype(np.longdouble) - ref).max()
        x = chol_solve(b, f, upper)
        assert x.dtype == dt and x.shape == b.shape
        got = np.abs(x.numpy().astype(np.longdouble) - ref).max()
        print(f"cholesky_solve n={n} batch={batch} nrhs={nrhs} upper={upper} {dt}: |gpu - ref| = {float(got):.3e}, |cpu - ref| = {float(cpu):.3e}, allowed {float(8 * cpu):.3e}")
        assert got <= 8 * cpu, (nrhs, float(got), float(cpu))
    eye = torch.eye(n, dtype=dt).expand(*bshape(batch), n, n).contiguous()
    ref = precise_solve(eye, f, upper)
    cpu = np.abs(R.cholesky_inverse(f, upper).numpy().astype(np.longdouble) - ref).max()
    inv = chol_inverse(f, upper)
    got = np.abs(inv.numpy().astype(np.longdouble) - ref).max()
    print(f"cholesky_inverse n={n} batch={batch} upper={upper} {dt}: |gpu - ref| = {float(got):.3e}, |cpu - ref| = {float(cpu):.3e}, allowed {float(8 * cpu):.3e}")
    assert got <= 8 * cpu, (float(got), float(cpu))


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [3, 33, LDS_SIDE, BLOCKED])
def test_cholesky_solve_and_inverse_exact_properties(gpu, dt, n):
    """at every form: the solves satisfy A x = b to the bound of two triangular solves, read one triangle, repeat bitwise, batch = alone"""
    a = R.spd(n, (3,))
    b = R.rhs(n, 3, (3,), dtype=dt)
    for upper in (0, 1):
        f = torch.linalg.cholesky(a, upper=bool(upper)).to(dt)
        x = chol_solve(b, f, upper)
        inv = chol_inverse(f, upper)
        f64 = f.double()
        tt = (f64.transpose(-1, -2).abs() @ f64.abs()) if upper else (f64.abs() @ f64.transpose(-1, -2).abs())
        full = (f64.transpose(-1, -2) @ f64) if upper else (f64 @ f64.transpose(-1, -2))
        # two substitutions, (F + dF1)(F^T + dF2) x = b with |dF| <= gamma(n) |F|: |F F^T x - b| <= (2 gamma(n) + gamma(n)^2) |F| |F^T| |x|
        # <= gamma(2 n) |F| |F^T| |x|; twice that for the f64 evaluation
        for name, sol, right in (("solve", x, b.double()), ("inverse", inv, torch.eye(n, dtype=torch.float64).expand(3, n, n))):
            excess = ((full @ sol.double() - right).abs() / (2 * R.gamma(2 * n, dt) * (tt @ sol.double().abs()))).max().item()
            print(f"cholesky_{name} n={n} upper={upper} {dt}: residual / bound = {excess:.3f}")
            assert excess <= 1.0, (name, upper, excess)
        assert same_bits(chol_solve(b, f, upper), x) and same_bits(chol_inverse(f, upper), inv)
        g = garbage(f, keep_upper=bool(upper))
        assert same_bits(chol_solve(b, g, upper), x) and same_bits(chol_inverse(g, upper), inv)
        for k in range(3):
            assert same_bits(chol_solve(b[k], f[k], upper), x[k]) and same_bits(chol_inverse(f[k], upper), inv[k])
    one = chol_solve(b, f[0], 1)                                           # a 2-D factor over a batch of right-hand sides
    assert all(same_bits(chol_solve(b[k], f[0], 1), one[k]) for k in range(3))


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def error_of(fn):
    with pytest.raises(LampError) as e:
        fn()
    assert str(e.value) == lib.load().lamp_last_error().decode()
    return str(e.value)


def cpu_error(a, upper=False):
    with pytest.raises(RuntimeError) as e:
        torch.linalg.cholesky(a, upper=upper)
    return str(e.value)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [1, 3, 33, LDS_SIDE, BLOCKED])
def test_not_positive_definite_is_atens_error(gpu, dt, n):
    a = R.spd(n, (), dtype=dt)
    good = chol(a)
    sentence = "linalg.cholesky: The factorization could not be completed because the input is not positive-definite (the leading minor of order %d is not positive-definite)."
    for upper in (0, 1):
        msg = error_of(lambda: chol(-a, upper))                           # the first pivot fails
        assert msg == sentence % 1 == cpu_error(-a, bool(upper))
        assert same_bits(chol(a), good)                                   # a good call after a failed one
        if n > 1:
            bad = a.clone()
            bad[n - 1, n - 1] = -1.0                                      # every leading minor but the last is A's own
            msg = error_of(lambda: chol(bad, upper))
            assert msg == sentence % n == cpu_error(bad, bool(upper))
            assert same_bits(chol(a), good)
    if n > 1:
        nan = a.clone()
        nan[1, 1] = float("nan")
        assert error_of(lambda: chol(nan)) == sentence % 2                # a NaN pivot is not > 0
        assert same_bits(chol(a), good)
        batch = torch.stack([a, -a, a])
        msg = error_of(lambda: chol(batch))
        assert msg == cpu_error(batch) and "(Batch element 1): " in msg and "order 1 " in msg
        both = torch.stack([a, bad, -a])                                  # the FIRST failing element and its order
        msg = error_of(lambda: chol(both))
        assert "(Batch element 1): " in msg and f"order {n} " in msg
        assert same_bits(chol(torch.stack([a, a, a])), torch.stack([good, good, good]))


def test_refusals_carry_a_reason(gpu):
    a = R.spd(4, ())
    bf = S.STen.from_numpy(a.float().numpy(), device=0, dtype=S.BF16)
    assert "f32 and f64" in error_of(lambda: bf.choleskyLower())
    assert "f32 and f64" in error_of(lambda: bf.choleskyInverse(False))
    assert "f32 and f64" in error_of(lambda: bf.choleskySolve(bf, False))
    assert "f32 and f64" in error_of(lambda: S.STen.triangularSolve(bf, bf, False, False, False))
    h = to_sten(a)
    assert "square" in error_of(lambda: h.narrow(0, 0, 3).choleskyLower())
    assert "mismatched sizes" in error_of(lambda: to_sten(R.rhs(5, 2)).choleskySolve(h, False))
    assert "batch shapes" in error_of(lambda: to_sten(R.rhs(4, 2, (3,))).choleskySolve(to_sten(R.spd(4, (2,))), False))
    assert " is " in error_of(lambda: to_sten(R.rhs(4, 2).float()).choleskySolve(h, False))          # f32 against f64
    assert same_bits(to_torch(h.choleskyLower()), chol(a))


# ---- host tensors: staged through the GPU, one case per call --------------------------------------------------------------------------
def test_host_tensors_are_staged(gpu):
    a = R.spd(5, (2,))
    b = R.rhs(5, 3, (2,))
    low = chol(a, 0, device=S.CPU)
    assert same_bits(low, chol(a, 0))
    assert to_sten(a, S.CPU).choleskyLower().device == S.CPU
    assert same_bits(chol_solve(b, low, 0, device=S.CPU), chol_solve(b, low, 0))
    assert same_bits(chol_inverse(low, 0, device=S.CPU), chol_inverse(low, 0))
    assert same_bits(tri_solve(b, low, 0, 1, 0, device=S.CPU), tri_solve(b, low, 0, 1, 0))
    msg = error_of(lambda: chol(-a, 0, device=S.CPU))
    assert "(Batch element 0): " in msg and "order 1 " in msg
