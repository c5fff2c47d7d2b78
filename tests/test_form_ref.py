"""What the kernel-form GPU tests of the reductions, the pooling and the index kernels take for granted, checked without a GPU: the table
of forms against the mirror of the reduction's chooser, the exactness of the integer probes in f32 / bf16 arithmetic, and the top-k
reference against ATen."""
import pytest
import torch

from tests import form_ref as FR
from tests import test_index_kernels_gpu as TI
from tests import test_pool_kernels_gpu as TP
from tests import test_reduce_kernels_gpu as TR
from tests.form_ref import BF16, F32, F64, I64, ITEM, small_ints, topk_ref
from tests.util import DTYPES


@pytest.mark.parametrize("dt,name,x2", TR.PARAMS)
def test_reduction_table_is_the_choosers(dt, name, x2):
    """on 256 compute units; the f32 / bf16 entries are the forms the cases were written for"""
    shape, (_, dims, narrow, wide, mis) = TR.case_shape(name, dt, x2), TR.CASES[name]
    assert FR.reduce_plan(shape, dims, ITEM[dt], 256, on_packet=not mis) == TR.case_expect(name, dt, x2)
    if ITEM[dt] < 8 or x2:
        assert TR.case_expect(name, dt, x2) == narrow
    if name.startswith("vec-"):
        assert narrow[0] == TR.CV
    if name == "vec-split-256-empty" and TR.case_expect(name, dt, x2)[0] == TR.CV:
        edges, empty = FR.split_rows(shape[0], 256)
        assert empty == 3 and edges[-1] == (252 * 65, 16384)


def test_every_reduction_tag_is_asserted():
    seen = {t for k in TR.CASES for dt in DTYPES for t in TR.case_expect(k, dt) if isinstance(t, str)}
    assert seen == {"reduce_block", "reduce_column", "reduce_column_vec", "reduce_generic", "reduce_finalize", "reduce_finalize_wide"}


def test_split_rows():
    assert FR.split_rows(10, 4) == ([(0, 2), (3, 5), (6, 8), (9, 9)], 0)
    assert FR.split_rows(9, 4) == ([(0, 2), (3, 5), (6, 8)], 1)
    assert FR.split_rows(7, 1) == ([(0, 6)], 0)


@pytest.mark.parametrize("dt,name,x2", [p for p in TR.PARAMS if p.values[0] != I64])
def test_integer_probes_are_exact(dt, name, x2):
    """the values are exact in bf16; the sums of the magnitudes and of the squares stay below 2^24, so every partial sum in every order
    is an integer f32 holds; summing in f32 in two different orders gives the float64 sum; rounding the float64 results to the dtype
    rounds once (torch goes through float32 for bfloat16: no float32 value may sit on a bfloat16 midpoint)"""
    shape, dims = TR.case_shape(name, dt, x2), TR.CASES[name][1]
    rdims = dims or list(range(len(shape)))
    x = small_ints(shape, 11, dt)
    xd = x.double()
    assert torch.equal(xd, small_ints(shape, 11, F64)) and xd.abs().max().item() == 3.0
    assert xd.abs().sum().item() < 2 ** 24 and (xd * xd).sum().item() < 2 ** 24
    for v in (xd, xd * xd):
        flat = v.float().reshape(-1)
        assert flat.cumsum(0)[-1].double().item() == flat.flip(0).cumsum(0)[-1].double().item() == v.sum().item()
    TR._rounded_once(xd.sum(rdims), dt)
    TR._rounded_once((xd * xd).sum(rdims).sqrt(), dt)


def test_rounded_once_sees_a_midpoint():
    with pytest.raises(AssertionError):
        TR._rounded_once(torch.tensor([1.00390625 + 2.0 ** -40], dtype=F64), BF16)      # float32 rounds it onto 1 + 2^-8
    assert TR._rounded_once(torch.tensor([1.00390625], dtype=F64), BF16).item() == 1.0   # the midpoint itself: one rounding, to even


def test_global_pool_sides_cover_every_lane_count():
    assert sorted({TP._lanes(s, dt) for s in (2, 4, 8, 16) for dt in DTYPES}) == [0, 1, 2, 4, 8, 16, 32, 64]
    assert TP._lanes(16, F64) == 0 and TP._lanes(7, F32) == 0 and TP._lanes(12, BF16) == 0 and TP._lanes(2, BF16) == 0


def test_special_pool_input():
    x = TP._special((2, 3, 9, 14), F32)
    assert int(torch.isnan(x).sum()) == 1 and bool(torch.isinf(x[..., :6, :6]).all()) and x[torch.isfinite(x)].unique().numel() <= 9
    x = TP._special((2, 3, 37), BF16)
    assert int(torch.isnan(x).sum()) == 1 and bool(torch.isinf(x[..., :6]).all())


@pytest.mark.parametrize("dt", DTYPES, ids=FR.dtid)
@pytest.mark.parametrize("largest", [False, True])
def test_topk_reference(dt, largest):
    """topk_ref is (value, index)-lexicographic; on rows without NaN it is the stable sort of v (of -v for `largest`); its values are
    ATen's topk values, NaN rows included (ATen: NaN is the greatest value)"""
    for x, k in ((TI._tie_rows(1000, dt), 64), (TI._nan_rows(1001, dt), 10), (TI._nan_rows(5, dt), 5), (TI._nan_rows(300, dt), 300)):
        v, i = topk_ref(x, k, 1, largest)
        assert FR.equal_bits(torch.gather(x, 1, i), v)
        av = torch.topk(x.double(), k, 1, largest, True)[0]
        assert torch.equal(torch.isnan(av), torch.isnan(v)) and torch.equal(av.nan_to_num(0.0), v.double().nan_to_num(0.0))
        vd = v.double()
        nan_a, nan_b = torch.isnan(vd[:, :-1]), torch.isnan(vd[:, 1:])
        lt = (vd[:, :-1] > vd[:, 1:]) if largest else (vd[:, :-1] < vd[:, 1:])
        eq = (vd[:, :-1] == vd[:, 1:]) | (nan_a & nan_b)
        first = (nan_a & ~nan_b) if largest else (~nan_a & nan_b)
        assert bool((lt | first | (eq & (i[:, :-1] < i[:, 1:]))).all())
        clean = ~torch.isnan(x.double()).any(1)
        s = torch.sort(-x.double() if largest else x.double(), dim=1, stable=True)[1][:, :k]
        assert torch.equal(s[clean], i[clean])


def test_index_data():
    idx = TI._indices(257, 500)
    assert idx.min().item() < 0 and idx.max().item() < 500 and idx.min().item() >= -500 and (idx == idx[0]).sum().item() > 30
    for N, nw in ((1, 11), (255, 50), (700, 1000)):
        t = TI._tokens(N, nw)
        assert 0 <= t.min().item() and t.max().item() == nw - 1 and t.numel() == N
    t = TI._tokens(700, 1000)
    assert t[0].item() == 0 and not bool(((t % 3 == 1) & (t != 999)).any())
