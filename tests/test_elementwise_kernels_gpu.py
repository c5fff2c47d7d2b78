"""Every functor of kernels/elementwise.hip in every dtype it is dispatched for, through the launch forms of launch_ew, and every (D, S)
pair of the converting copy kernels of core/tensor.hip, against the references of tests/elementwise_ref.py (verified on the CPU by
tests/test_elementwise_ref.py, which also runs the same registry on host tensors).

The launch form cannot be read from the kernel timers - ew_vec_kernel, ew_rowvec_kernel and ew_strided_kernel share the tag
`elementwise` - so the tests assert the preconditions launch_ew chooses by instead: the number of dimensions after collapsing, the strides
and the alignment of every operand.
  flat      1-D contiguous operands of n_for(dt) elements on 16-byte boundaries (n > 1): ew_vec_kernel - two full blocks of packets, one
            packet in a third block, a scalar tail.  A one-element operand of a binary functor: its bcast_mask branch.
  strided   the same values one element past a 16-byte boundary (contiguous, 1-D: no packet form takes it) and as a stride-2 slice of a
            [2 n] tensor: ew_strided_kernel.  Bit for bit the flat form's result.
The second grid trip, the row-vector form and the large tensors are tests/test_row_kernels_gpu.py's.  where_kernel, masked_fill_kernel and
add_scaled_mixed_kernel have one form each; copy_contig_kernel and copy_strided_kernel are chosen by `all_contiguous`."""
import pytest
import torch

from lamp_amd import sten as S
from tests import elementwise_ref as E
from tests.elementwise_ref import BOOL, F64, FLOATS
from tests.util import assert_close, to_sten, to_torch

pytestmark = pytest.mark.gpu


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
def flat(x):
    a = to_sten(x)
    assert a.data_ptr % 16 == 0 and a.is_contiguous() and len(a.shape) <= 1
    return a


class Views:
    """operands as views into larger zero-filled tensors; untouched() afterwards: no launch wrote outside a view"""

    def __init__(self, how):
        self.how, self.bases = how, []

    def __call__(self, x):
        n = x.numel()
        if self.how == "misaligned":                    # contiguous, one element past a 16-byte boundary
            base = to_sten(torch.cat([x.new_zeros(1), x.reshape(-1)]))
            v = base.narrow(0, 1, n)
            assert base.data_ptr % 16 == 0 and v.data_ptr % 16 == E.ITEM[x.dtype] and v.is_contiguous() and v.shape == [n]
            self.bases.append((base, [0]))
        else:                                           # every second element of a [2 n] tensor
            base = to_sten(torch.stack([x.reshape(-1), torch.zeros_like(x.reshape(-1))], 1).reshape(-1))
            v = base.slice(0, 0, 2 * n, 2)
            assert v.shape == [n] and v.strides == [2] and v.data_ptr == base.data_ptr
            self.bases.append((base, list(range(1, 2 * n, 2))))
        return v

    def untouched(self):
        for base, idx in self.bases:
            assert bool((E.bits(to_torch(base))[torch.tensor(idx)].double() == 0).all()), f"{self.how}: a launch wrote outside its view"


# ---- the registry through the launch forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", E.grid(), ids=E.grid_id)
def test_functor(gpu, p):
    e, dt = p
    for scalars in e.cases(dt):
        what = f"{e.name}{scalars} {E.dtid(dt)}"
        xs = E.operands(e, dt)
        assert all(x.numel() == E.n_for(dt) > 1 and x.dim() == 1 for x in xs)
        got = E.run_and_check(e, dt, scalars, flat, what + " flat")
        for how in ("misaligned", "stride2"):
            views = Views(how)
            g = E.run_and_check(e, dt, scalars, views, f"{what} {how}")
            views.untouched()
            assert E.equal_bits(E.bits(g), E.bits(got)), f"{what}: the {how} form differs from the flat one"
        if e.arity == 2:
            # one element (an ordinary value of the sweep) on either side; an in-place form can only take it on the right
            for side in ((1,) if e.kind == "inplace" else (0, 1)):
                ys = list(xs)
                ys[side] = xs[side][30:31].clone()
                assert bool(torch.isfinite(ys[side].double()).all())
                E.run_and_check(e, dt, scalars, flat, f"{what} one element on side {side}", xs=ys)


# ---- where / masked_fill ------------------------------------------------------------------------------------------------------------------
R = 37


def _rn(dt, salt):
    n = E.n_for(dt) // R
    return E.table((-6.0, 6.0), dt, salt, R * n).reshape(R, n)


def _transposed(x):
    """x's values as the transposed view of a dense [N, R] tensor"""
    v = to_sten(x.t().contiguous()).t
    assert v.shape == list(x.shape) and v.strides == [1, x.shape[0]]
    return v


@pytest.mark.parametrize("dt", E.ALL_BOOL, ids=E.dtid)
def test_where(gpu, dt):
    a, b = _rn(dt, 1), _rn(dt, 12)
    n = a.shape[1]
    cond = (torch.arange(R * n).reshape(R, n) * 7919 % 1009 % 3 == 0)
    z = a[5, 7].clone()                                                   # 0-dim
    cases = [("[R, 1] condition, [1, N] other", cond[:, :1], to_sten(cond[:, :1].contiguous()), a, to_sten(a), b[:1], to_sten(b[:1])),
             ("dense condition, transposed self, 0-dim other", cond, to_sten(cond), a, _transposed(a), z, to_sten(z)),
             ("0-dim self, transposed other", cond, to_sten(cond), z, to_sten(z), b, _transposed(b)),
             ("[1, N] condition as uint8", cond[:1], to_sten(cond[:1].to(torch.uint8)), a, to_sten(a), b, to_sten(b))]
    for what, c, C_, x, X, y, Y in cases:
        got = to_torch(S.STen.where(C_, X, Y))
        ref = torch.where(c, x, y)
        assert got.dtype == (torch.float32 if dt == torch.bfloat16 else dt)
        assert E.equal_bits(E.bits(got), E.bits(ref)), f"where {E.dtid(dt)} {what}"


@pytest.mark.parametrize("dt", E.ALL_BOOL, ids=E.dtid)
def test_masked_fill(gpu, dt):
    a = _rn(dt, 1)
    n = a.shape[1]
    mask = (torch.arange(R * n).reshape(R, n) * 7919 % 1009 % 3 == 0)
    values = (2.5, -0.0, float("inf"), float("nan")) if dt in FLOATS else ((7.0, -3.0) if dt in (torch.int64, torch.int32) else ((7.0,) if dt == torch.uint8 else (1.0, 0.0)))
    for v in values:
        fill = v if dt in FLOATS else (bool(v) if dt == BOOL else int(v))
        for what, X, m in (("dense mask", to_sten(a), mask), ("[R, 1] mask", to_sten(a), mask[:, :1].contiguous()), ("[1, N] mask", to_sten(a), mask[:1].contiguous()),
                           ("0-dim mask", to_sten(a), torch.tensor(True)), ("transposed self", _transposed(a), mask)):
            got = to_torch(X.maskedFill(to_sten(m), v))
            assert E.equal_bits(E.bits(got), E.bits(a.masked_fill(m, fill))), f"masked_fill {E.dtid(dt)} {v} {what}"


# ---- add_scaled_mixed_ --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dx", FLOATS, ids=E.dtid)
@pytest.mark.parametrize("da", FLOATS, ids=E.dtid)
def test_add_scaled_mixed(gpu, da, dx):
    """acc += scale * x in f64, one rounding to acc's dtype.  FWD_TOL of the accumulator, not bit-exact: the f64 multiply-add may contract"""
    from lamp_amd._capi import lib
    n = max(E.n_for(da), E.n_for(dx))                                      # n_for of the smaller item size
    acc, x = E.float_table(-6.0, 6.0, da, 1, n), E.float_table(-6.0, 6.0, dx, 12, n)
    for scale in (0.75, -3.0):
        A, X = flat(acc), flat(x)
        ptr = A.data_ptr
        lib.lamp_add_scaled_mixed_(A, X, scale)
        assert A.data_ptr == ptr
        assert_close(to_torch(A), (acc.double() + scale * x.double()).to(da).double(), E.TOL[da], f"add_scaled_mixed {E.dtid(da)} += {scale} * {E.dtid(dx)}")
    if da == F64:
        # the epoch-loss accumulator of the training loops: an f64 scalar, the batch loss in the model's dtype
        A, X = S.STen.scalarDouble(1.25, S.F64), to_sten(torch.tensor(0.3, dtype=dx))
        lib.lamp_add_scaled_mixed_(A, X, 128.0)
        assert_close(to_torch(A), torch.tensor(1.25 + 128.0 * torch.tensor(0.3, dtype=dx).double().item(), dtype=F64), E.TOL[F64], f"scalar accumulator, {E.dtid(dx)} loss")


# ---- converting copies ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", E.CAST_PAIRS, ids=E.cast_id)
def test_cast(gpu, p):
    """lamp_cast, lamp_to and lamp_copy_ for one (source, destination) pair: copy_contig_kernel<D, S> on contiguous tensors,
    copy_strided_kernel<D, S> through a transposed view and a broadcast [1, N] source; bit-exact against torch's .to() on the CPU"""
    E.check_cast(p[0], p[1], 0)
