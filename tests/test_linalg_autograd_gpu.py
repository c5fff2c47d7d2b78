"""The autograd operators Cholesky and CholeskySolve (csrc/host/ops2.cpp over kernels/linalg.hip; ops.scala:2186-2285) on the GPU.

Reference: the closures as the reference writes them, restated on torch-CPU (tests/linalg_ref.py) - not torch.autograd, whose gradient
for CholeskySolve's factor lives in the factor's own triangle only while the reference mirrors it into both.
f64: rtol 1e-10, atol 1e-12, the tolerance tests/test_autograd_gpu.py holds its f64 oracle comparisons to.
f32: 8 x the distance the same closures evaluated on torch-CPU in f32 keep from their f64 evaluation on the same inputs (the order of
summation differs, nothing else); every case prints both distances (-s), BASELINE.md section 21 records them.
Finite differences: f64, n = 3, central differences of the GPU forward with step 1e-6, agreement to 4 decimals as the reference's own
gradient suite asks (autograd.test.scala:135), i.e. |gradient - difference| <= 5e-5."""
import numpy as np
import pytest
import torch

from lamp_amd import autograd as A
from tests import linalg_ref as R
from tests.util import to_sten, to_torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32]
DT_IDS = ["f64", "f32"]
P = [[52.0, 16.0], [16.0, 5.0]]                       # mat2x2PD, autograd.test.scala:27


def weights(shape, seed, dtype):
    g = torch.Generator().manual_seed(4000 + seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)


def weighted_sum(v, w):
    """sum(v * w): the partial derivative that reaches v's closure is w"""
    return (v * A.const(to_sten(w))).sum()


def compare(what, got, ref64, cpu, dt):
    """f64: the suite's oracle tolerance; f32: 8 x torch-CPU's own distance from the f64 result"""
    if dt == torch.float64:
        np.testing.assert_allclose(got.numpy(), ref64.numpy(), rtol=1e-10, atol=1e-12, err_msg=what)
        return
    d_gpu = (got.double() - ref64).abs().max().item()
    d_cpu = (cpu.double() - ref64).abs().max().item()
    print(f"{what}: |gpu - f64| = {d_gpu:.3e}, |cpu f32 - f64| = {d_cpu:.3e}, allowed {8 * d_cpu:.3e}")
    assert d_gpu <= 8 * d_cpu, (what, d_gpu, d_cpu)


def test_reference_known_answers(gpu):
    p = A.param(to_sten(torch.tensor(P, dtype=torch.float64)))
    low = p.choleskyLower()
    assert round(float(to_torch(low.sum().value)), 4) == 9.7073                       # autograd.test.scala:968
    b = A.param(to_sten(torch.tensor([[4.0, 1.0], [6.0, 2.0]], dtype=torch.float64)))
    x = b.choleskySolve(A.const(low.value))
    assert round(float(to_torch(x.sum().value)), 4) == 58.25                          # autograd.test.scala:981


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [3, 33])
@pytest.mark.parametrize("batch", [(), (3,)], ids=["2d", "3d"])
def test_cholesky_value_and_gradient(gpu, dt, n, batch):
    a = R.spd(n, batch, dtype=dt)
    w = weights((*batch, n, n), 1, dt)
    v = A.param(to_sten(a))
    low = v.choleskyLower()
    weighted_sum(low, w).backprop()
    l64 = R.cholesky(a.double())
    l32 = R.cholesky(a)
    compare(f"Cholesky value n={n} {batch}", to_torch(low.value), l64, l32, dt)
    compare(f"Cholesky gradient n={n} {batch}", to_torch(v.partialDerivative), R.cholesky_backward(l64, w.double()), R.cholesky_backward(l32, w), dt)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("upper", [0, 1], ids=["lower", "upper"])
@pytest.mark.parametrize("n", [3, 33])
@pytest.mark.parametrize("batch", [(), (3,)], ids=["2d", "3d"])
def test_cholesky_solve_value_and_gradients(gpu, dt, upper, n, batch):
    f = torch.linalg.cholesky(R.spd(n, batch), upper=bool(upper)).to(dt)
    b = R.rhs(n, 2, batch, dtype=dt)
    w = weights((*batch, n, 2), 2, dt)
    vb, vf = A.param(to_sten(b)), A.param(to_sten(f))
    x = vb.choleskySolve(vf, bool(upper))
    weighted_sum(x, w).backprop()
    tag = f"n={n} {batch} upper={upper}"
    x64 = R.cholesky_solve(b.double(), f.double(), upper)
    x32 = R.cholesky_solve(b, f, upper)
    compare(f"CholeskySolve value {tag}", to_torch(x.value), x64, x32, dt)
    compare(f"CholeskySolve gradient of b {tag}", to_torch(vb.partialDerivative), R.cholesky_solve_backward_b(w.double(), f.double(), upper),
            R.cholesky_solve_backward_b(w, f, upper), dt)
    compare(f"CholeskySolve gradient of the factor {tag}", to_torch(vf.partialDerivative),
            R.cholesky_solve_backward_factor(w.double(), x64, f.double(), upper), R.cholesky_solve_backward_factor(w, x32, f, upper), dt)


def test_gradients_accumulate_into_existing_buffers(gpu):
    """two consumers of one variable: the second closure adds to (Cholesky, b) or subtracts from (the factor) the buffer the first one left"""
    n = 3
    a = R.spd(n, (2,))
    w1, w2 = weights((2, n, n), 3, torch.float64), weights((2, n, n), 4, torch.float64)
    v = A.param(to_sten(a))
    (weighted_sum(v.choleskyLower(), w1) + weighted_sum(v.choleskyLower(), w2)).backprop()
    l64 = R.cholesky(a)
    np.testing.assert_allclose(to_torch(v.partialDerivative).numpy(), (R.cholesky_backward(l64, w1) + R.cholesky_backward(l64, w2)).numpy(), rtol=1e-10, atol=1e-12)
    b = R.rhs(n, 2, (2,))
    u1, u2 = weights((2, n, 2), 5, torch.float64), weights((2, n, 2), 6, torch.float64)
    vb, vf = A.param(to_sten(b)), A.param(to_sten(l64))
    (weighted_sum(vb.choleskySolve(vf), u1) + weighted_sum(vb.choleskySolve(vf), u2)).backprop()
    x64 = R.cholesky_solve(b, l64, False)
    np.testing.assert_allclose(to_torch(vb.partialDerivative).numpy(),
                               (R.cholesky_solve_backward_b(u1, l64, False) + R.cholesky_solve_backward_b(u2, l64, False)).numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(to_torch(vf.partialDerivative).numpy(),
                               (R.cholesky_solve_backward_factor(u1, x64, l64, False) + R.cholesky_solve_backward_factor(u2, x64, l64, False)).numpy(),
                               rtol=1e-10, atol=1e-12)


def _loss(fn, *tensors):
    return float(to_torch(fn(*[A.param(to_sten(t)) for t in tensors]).value))


def test_finite_differences(gpu):
    n, eps = 3, 1e-6
    a = R.spd(n, ())
    w = weights((n, n), 7, torch.float64)
    v = A.param(to_sten(a))
    weighted_sum(v.choleskyLower(), w).backprop()
    g = to_torch(v.partialDerivative)
    for i in range(n):
        for j in range(i + 1):                       # symmetric perturbations: the input is a symmetric matrix
            s = torch.zeros(n, n, dtype=torch.float64)
            s[i, j] = s[j, i] = 1.0
            fd = (_loss(lambda x: weighted_sum(x.choleskyLower(), w), a + eps * s) - _loss(lambda x: weighted_sum(x.choleskyLower(), w), a - eps * s)) / (2 * eps)
            assert abs((g * s).sum().item() - fd) <= 5e-5, ("Cholesky", i, j, (g * s).sum().item(), fd)
    low = R.cholesky(a)
    b = R.rhs(n, 2, ())
    u = weights((n, 2), 8, torch.float64)
    for upper in (False, True):
        f = low.t().contiguous() if upper else low
        vb, vf = A.param(to_sten(b)), A.param(to_sten(f))
        weighted_sum(vb.choleskySolve(vf, upper), u).backprop()
        gb, gf = to_torch(vb.partialDerivative), to_torch(vf.partialDerivative)
        solve = lambda bb, ff: weighted_sum(bb.choleskySolve(ff, upper), u)   # noqa: E731
        for i in range(n):
            for j in range(2):
                s = torch.zeros(n, 2, dtype=torch.float64)
                s[i, j] = 1.0
                fd = (_loss(solve, b + eps * s, f) - _loss(solve, b - eps * s, f)) / (2 * eps)
                assert abs(gb[i, j].item() - fd) <= 5e-5, ("CholeskySolve b", upper, i, j, gb[i, j].item(), fd)
        if upper:
            continue                                 # the reference's closure takes tril for either triangle: its lower-factor form is the one that is a gradient
        for i in range(n):
            for j in range(i + 1):                   # the factor's own triangle; the closure mirrors it into the other one
                s = torch.zeros(n, n, dtype=torch.float64)
                s[i, j] = 1.0
                fd = (_loss(solve, b, f + eps * s) - _loss(solve, b, f - eps * s)) / (2 * eps)
                assert abs(gf[i, j].item() - fd) <= 5e-5, ("CholeskySolve factor", i, j, gf[i, j].item(), fd)
                assert gf[j, i].item() == gf[i, j].item() or i == j
