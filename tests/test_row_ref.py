"""tests/row_ref.py against ATen's float64 operators, to 1e-12: the reference of the row-kernel GPU tests, verified without a GPU."""
import pytest
import torch

from tests import row_ref as R
from tests.util import assert_close, closed_form

F64 = torch.float64
aten = torch.ops.aten
TOL = 1e-12


def _ln_inputs(shape, nnorm):
    norm = list(shape[len(shape) - nnorm:])
    rows = 1
    for s in shape[:len(shape) - nnorm]:
        rows *= s
    x = closed_form(shape, 3, 4.0, F64) + 3.0
    x = x + torch.arange(rows, dtype=F64).reshape(list(shape[:len(shape) - nnorm]) + [1] * nnorm)
    return x, closed_form(norm, 1, 1.0, F64) + 1.0, closed_form(norm, 5, 1.0, F64), closed_form(shape, 13, 2.0, F64), norm


@pytest.mark.parametrize("shape,nnorm", [((5, 1), 1), ((5, 3), 1), ((5, 96), 1), ((7, 1025), 1), ((3, 4, 24), 2), ((2, 3, 17), 1), ((2, 4105), 1)])
@pytest.mark.parametrize("affine", [True, False])
def test_layer_norm_reference(shape, nnorm, affine):
    x, w, b, g, norm = _ln_inputs(shape, nnorm)
    if not affine:
        w = b = None
    ref = aten.native_layer_norm(x, norm, w, b, 1e-5)
    y, mean, rstd = R.layer_norm(x, w, b, 1e-5, nnorm)
    assert_close(y, ref[0], TOL, "y")
    assert_close(mean, ref[1], TOL, "mean")
    assert_close(rstd, ref[2], TOL, "rstd")
    # the backward takes mean / rstd as given: hand both sides the same perturbed (as if rounded) values
    m2 = (ref[1] * (1 + 2.0 ** -9)).contiguous()
    r2 = (ref[2] * (1 - 2.0 ** -9)).contiguous()
    for mm, rr in ((ref[1], ref[2]), (m2, r2)):
        refb = aten.native_layer_norm_backward(g, x, norm, mm, rr, w, b, [True, affine, affine])
        dx, dw, db = R.layer_norm_backward(g, x, mm, rr, w, nnorm)
        if shape[-1] == 1 and nnorm == 1:
            # D = 1: gw - mean(gw) is exactly 0 and dx is what is left of terms of the size of rstd * gw: that size is the yardstick
            terms = (rr * g * (w if affine else 1.0)).abs().max().item()
            assert (dx - refb[0]).abs().max().item() <= TOL * terms
        else:
            assert_close(dx, refb[0], TOL, "dx")
        if affine and shape[-1] == 1 and nnorm == 1:
            # likewise: x - mean is exactly 0 here, ATen sums products of the size of g x rstd
            assert (dw - refb[1]).abs().max().item() <= TOL * (g.abs() * (x.abs() + mm.abs()) * rr).sum().item()
            assert_close(db, refb[2], TOL, "db")
        elif affine:
            assert_close(dw, refb[1], TOL, "dw")
            assert_close(db, refb[2], TOL, "db")
        else:
            assert list(dw.shape) == norm and list(db.shape) == norm


@pytest.mark.parametrize("shape,dim", [((5, 100), 1), ((5, 4104), 1), ((2, 12001), 1), ((70, 65), 0), ((3, 200, 67), 1), ((3, 200, 67), -1)])
def test_softmax_reference(shape, dim):
    x = closed_form(shape, 3, 8.0, F64)
    ls = R.log_softmax(x, dim)
    assert_close(ls, aten._log_softmax(x, dim, False), TOL, "log_softmax")
    assert_close(R.softmax(x, dim), aten._softmax(x, dim, False), TOL, "softmax")
    g = closed_form(shape, 8, 1.0, F64)
    out = ls.to(torch.bfloat16).to(F64)           # an `out` that is not exactly normalised, as the kernel gets it
    for o in (ls, out):
        assert_close(R.log_softmax_backward(g, o, dim), aten._log_softmax_backward_data(g, o, dim, F64), TOL, "log_softmax backward")


@pytest.mark.parametrize("dt", [torch.float64, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [31, 256, 4104])
def test_special_rows_have_atens_pattern(dt, D):
    """one entry of 60, every third entry -inf, equal entries, all -inf: the float64 formulas give ATen's values in float64 and, in the
    dtype under test, ATen's pattern of NaN / infinities (assert_close compares that pattern before the values)."""
    x = R.special_rows(D, dt)
    assert torch.isinf(x[1, ::3]).all() and torch.isinf(x[3]).all() and x[0].max().item() == 60.0
    for name, mine, theirs in (("log_softmax", R.log_softmax, aten._log_softmax), ("softmax", R.softmax, aten._softmax)):
        ref = mine(x, 1)
        assert_close(ref, theirs(x.to(F64), 1, False), TOL, name)
        own = theirs(x, 1, False).double()
        assert torch.equal(torch.isnan(own), torch.isnan(ref)), name
        assert torch.equal(torch.isinf(own), torch.isinf(ref)), name
        assert torch.isnan(ref[3]).all() and torch.isfinite(ref[0]).all() and torch.isfinite(ref[2]).all()
