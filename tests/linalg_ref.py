"""Torch-CPU restatements of the four symmetric positive-definite calls (ATen's linalg_cholesky, cholesky_solve, cholesky_inverse,
triangular_solve) and of the closures of lamp's Cholesky and CholeskySolve operators (ops.scala:2186-2285), line for line.  The closures
are the reference's own formulas, NOT torch.autograd: the factor gradient of CholeskySolve is mirrored into both triangles there.
Everything runs in the dtype it is given (the tests pass f64 for the reference and the working dtype to measure torch-CPU's own error)."""
import torch


def cholesky(a, upper=False):
    return torch.linalg.cholesky(a, upper=bool(upper))


def cholesky_solve(b, factor, upper=False):
    return torch.cholesky_solve(b, factor, upper=bool(upper))


def cholesky_inverse(factor, upper=False):
    return torch.cholesky_inverse(factor, upper=bool(upper))


def triangular_solve(b, a, upper, transpose, unitriangular):
    # linalg.solve_triangular has no transpose flag: op(a) = a^T is the other triangle of the transposed matrix
    t = a.transpose(-1, -2) if transpose else a
    return torch.linalg.solve_triangular(t, b, upper=bool(upper) != bool(transpose), unitriangular=bool(unitriangular))


def _mm(a, b):
    return a.bmm(b) if a.dim() == 3 else a.mm(b)


def _tril_half_diagonal(t):
    t = t.tril()
    d = torch.diagonal(t, 0, -2, -1)
    d *= 0.5
    return t


def cholesky_backward(l, g):
    """Cholesky's closure: l the lower factor, g the incoming partial derivative; returns what is added to the input's gradient"""
    size = l.shape[-2]
    linv = triangular_solve(torch.eye(size, dtype=l.dtype).expand(l.shape).contiguous() if l.dim() == 3 else torch.eye(size, dtype=l.dtype),
                            l, False, False, False)
    phi = _tril_half_diagonal(_mm(l.transpose(-1, -2), g))
    tmp = _mm(_mm(linv.transpose(-1, -2), phi), linv)
    return (tmp + tmp.transpose(-1, -2)) * 0.5


def cholesky_solve_backward_b(p, factor, upper):
    """CholeskySolve's closure for b: out += p.choleskySolve(factor, upper)"""
    return cholesky_solve(p, factor, upper)


def cholesky_solve_backward_factor(p, value, factor, upper):
    """CholeskySolve's closure for the factor, as a quantity ADDED to the gradient (the reference subtracts `symmetrized`)"""
    gb = cholesky_solve(p, factor, upper)
    tmp = _mm(gb, value.transpose(-2, -1))
    tmp2 = tmp + tmp.transpose(-2, -1)
    tmp4 = _mm(factor, tmp2) if upper else _mm(tmp2, factor)
    tmp4 = _tril_half_diagonal(tmp4)
    return -(tmp4 + tmp4.transpose(-2, -1))


def spd(n, batch=(), seed=0, dtype=torch.float64):
    """A = M M^T / n + I, M standard normal: condition number about 5"""
    g = torch.Generator().manual_seed(1000 * n + seed)
    m = torch.randn(*batch, n, n, generator=g, dtype=torch.float64)
    a = m @ m.transpose(-1, -2) / n + torch.eye(n, dtype=torch.float64)
    return ((a + a.transpose(-1, -2)) * 0.5).to(dtype)                      # bit-symmetric: a + a^T commutes


def triangle(n, batch=(), seed=0, upper=False, dtype=torch.float64):
    """tril / triu(randn) + 3 I"""
    g = torch.Generator().manual_seed(2000 * n + seed)
    m = torch.randn(*batch, n, n, generator=g, dtype=torch.float64)
    return ((m.triu() if upper else m.tril()) + 3.0 * torch.eye(n, dtype=torch.float64)).to(dtype)


def rhs(n, nrhs, batch=(), seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(3000 * n + 7 * nrhs + seed)
    return torch.randn(*batch, n, nrhs, generator=g, dtype=torch.float64).to(dtype)


def gamma(k, dtype):
    """gamma(k) = k u / (1 - k u), u the unit roundoff of dtype"""
    u = torch.finfo(dtype).eps / 2
    return k * u / (1 - k * u)


OPS = {"linalg_cholesky": 0, "cholesky_solve": 1, "cholesky_inverse": 2, "triangular_solve": 3}


def linalg_plan(op, dt, a_shape, b_shape=None, cus=256):
    """The plan the library makes for a call on operands of these shapes on a device of `cus` compute units (lamp_debug_linalg_plan: the
    functions the real path uses, no GPU needed), as a dict; numbers as ints."""
    import ctypes as C
    from lamp_amd._capi import lib, i64_array
    from tests.util import TORCH2LAMP
    buf = C.create_string_buffer(2048)
    lib.lamp_debug_linalg_plan(OPS[op], TORCH2LAMP[dt], i64_array(a_shape), len(a_shape), i64_array(b_shape) if b_shape is not None else None,
                               len(b_shape) if b_shape is not None else 0, int(cus), buf, len(buf))
    d = dict(line.split("=", 1) for line in buf.value.decode().splitlines())
    return {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in d.items()}
