"""Plain float64 formulas of the row operators (layer norm, softmax, log-softmax and their backward passes): the reference
tests/test_row_kernels_gpu.py compares every kernel form with.  Callers hand in the inputs as the kernel sees them (already rounded
to the dtype under test); everything here is computed in float64 and nothing is rounded on the way.  tests/test_row_ref.py pins these
formulas to ATen's float64 operators on a machine without a GPU."""
import math

import torch

F64 = torch.float64


def _norm_dims(x, nnorm):
    return tuple(range(x.dim() - nnorm, x.dim()))


def layer_norm(x, w=None, b=None, eps=1e-5, nnorm=1):
    """-> (y, mean, rstd) over the last `nnorm` dims; mean / rstd keep those dims with size 1 (native_layer_norm's shapes).
    rstd = 1 / sqrt(biased variance + eps)."""
    x = x.to(F64)
    dims = _norm_dims(x, nnorm)
    mean = x.mean(dims, keepdim=True)
    var = ((x - mean) ** 2).mean(dims, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * rstd
    if w is not None:
        y = y * w.to(F64)
    if b is not None:
        y = y + b.to(F64)
    return y, mean, rstd


def layer_norm_backward(g, x, mean, rstd, w=None, nnorm=1):
    """-> (dx, dw, db) from the GIVEN mean / rstd (the values the kernel is handed, rounded to its dtype):
    xh = (x - mean) rstd, gw = g w, dx = rstd (gw - mean_D(gw) - xh mean_D(gw xh)), dw = sum_rows(g xh), db = sum_rows(g)."""
    g, x, mean, rstd = g.to(F64), x.to(F64), mean.to(F64), rstd.to(F64)
    dims = _norm_dims(x, nnorm)
    rows = tuple(range(x.dim() - nnorm))
    xh = (x - mean) * rstd
    gw = g * w.to(F64) if w is not None else g
    dx = rstd * (gw - gw.mean(dims, keepdim=True) - xh * (gw * xh).mean(dims, keepdim=True))
    dw = (g * xh).sum(rows) if rows else g * xh
    db = g.sum(rows) if rows else g.clone()
    return dx, dw, db


def log_softmax(x, dim):
    """x - max - log(sum(exp(x - max))) along dim.  A row that is all -inf is NaN (-inf - -inf), as in ATen."""
    x = x.to(F64)
    z = x - x.max(dim, keepdim=True).values
    return z - torch.log(torch.exp(z).sum(dim, keepdim=True))


def softmax(x, dim):
    x = x.to(F64)
    e = torch.exp(x - x.max(dim, keepdim=True).values)
    return e / e.sum(dim, keepdim=True)


def log_softmax_backward(g, out, dim):
    """g - exp(out) sum(g), with `out` the log-softmax output as the kernel is handed it."""
    g, out = g.to(F64), out.to(F64)
    return g - torch.exp(out) * g.sum(dim, keepdim=True)


def special_rows(D, dtype):
    """the four rows softmax kernels get wrong first: one entry of 60 among ordinary ones, every third entry -inf, all entries equal,
    all entries -inf."""
    i = torch.arange(D, dtype=torch.int64)
    base = (((i * 7919) % 1009).to(F64) / 1009.0 - 0.5) * 8.0
    r0 = base.clone(); r0[D // 2] = 60.0
    r1 = base.clone(); r1[::3] = -math.inf
    r2 = torch.full((D,), 1.5, dtype=F64)
    r3 = torch.full((D,), -math.inf, dtype=F64)
    return torch.stack([r0, r1, r2, r3]).to(dtype)
