"""Every form of top-k, the row gather, the embedding gradient and the atomic scatters of kernels/index.hip, bit-exact against plain
torch expressions on the inputs AFTER rounding to the dtype under test.

  top-k       topk_wave (k <= 64: a wave per row, four rows per workgroup): the 4-element scan (D % 4 == 0, aligned rows) or the scalar one;
              the threshold + compaction path, the k-rounds path inside the wave when fewer than k lanes saw an element (short rows),
              more than 64 candidates pass the threshold (ties) or the row holds a NaN; topk_rounds (k > 64: a workgroup per row, k
              rounds).  The reference is the first k of a stable sort - lexicographic (value, index), NaN the greatest value and equal to every NaN, -0.0 == 0.0 - which
              is the order the kernels promise; ATen's own topk picks the same values and leaves the order of ties open.
  gather      index_select_rows_vec (dim 0, rows a multiple of 16 bytes, aligned) against index_select
  embedding   embedding_bwd_scan (num_weights * N <= 2^28: no atomics, rounds once) against zero fill + index_add
  atomics     index_add, scatter_add: f64 / f32 / int64 hardware atomics, bf16 by compare-and-swap on the 32-bit word that holds the element
Each test asserts the tag of the form it was written for through the kernel timers.  Gradients and sources are small integers wherever
the order of the additions is not fixed (|sum| <= 256, exact in bf16), so every comparison but the closed-form embedding gradients (one
rounding of an f32 / f64 sum: FWD_TOL) is an equality."""
import ctypes as C

import pytest
import torch

from lamp_amd import sten as S
from lamp_amd._capi import lib
from tests.form_ref import BF16, F32, F64, I64, W, aligned, dtid, equal_bits, launched, misaligned, small_ints, topk_ref
from tests.util import DTYPES, FWD_TOL, assert_close, closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu
ALL = DTYPES + [I64]
NAN, INF = float("nan"), float("inf")


def _data(shape, salt, dt):
    return small_ints(shape, salt, I64, 1000) if dt == I64 else closed_form(shape, salt, 2.0, dt)


# ---- top-k ---------------------------------------------------------------------------------------------------------------------------
def _check_topk(x, k, dim, largest, tag, what=""):
    with launched() as L:
        v, ix = to_sten(x).topk(k, dim, largest, True)
    ran = {t: L.count(t) for t in L if t.startswith("topk_")}
    assert ran == {tag: 1}, f"launched {ran}, written for {tag}"
    rv, rix = topk_ref(x, k, dim, largest)
    got_v, got_i = to_torch(v), to_torch(ix)
    bad = (got_i != rix).reshape(-1).nonzero().reshape(-1).tolist()[:6]
    assert not bad, f"{what} k={k} largest={largest}: indices differ at {bad}: got {got_i.reshape(-1)[bad].tolist()} for {rix.reshape(-1)[bad].tolist()}"
    assert equal_bits(got_v, rv), f"{what} k={k} largest={largest}: values differ"


# rows, D, k, tag: D % 4 == 0 and != 0, neither row count a multiple of 4; k = 30 of 100: 25 lanes see elements in the 4-element scan;
# k = D; k = 64, the widest wave form; k = 65 and k = D through the k-rounds kernel
TOPK = [(7, 1000, 10, "topk_wave"), (5, 1001, 10, "topk_wave"), (3, 100, 10, "topk_wave"), (3, 100, 30, "topk_wave"), (2, 5, 5, "topk_wave"),
        (4, 2048, 64, "topk_wave"), (3, 300, 65, "topk_rounds"), (3, 300, 300, "topk_rounds")]


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("rows,D,k,tag", TOPK, ids=[f"{r}x{d}-k{k}" for r, d, k, _ in TOPK])
def test_topk_forms(gpu, dt, largest, rows, D, k, tag):
    """closed-form values (period 1009, and 8 bits of mantissa in bf16: the long rows hold ties)"""
    _check_topk(closed_form((rows, D), 5, 2.0, dt), k, 1, largest, tag)


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
def test_topk_along_dim_0(gpu, dt, largest):
    x = closed_form((1000, 6), 5, 2.0, dt)
    _check_topk(x, 10, 0, largest, "topk_wave")
    _check_topk(x.reshape(10, 100, 6), 7, 1, largest, "topk_wave", "middle dim")


def _tie_rows(D, dt):
    """one repeated value; 200 copies of the minimum and 200 of the maximum (more than 64 candidates pass the threshold); zeros of both
    signs among a few numbers; three +inf and three -inf; all +inf; all -inf"""
    x = closed_form((6, D), 5, 2.0, F64)
    x[0] = 1.5
    x[1, (torch.arange(200) * 5 + 1) % D] = -3.0
    x[1, (torch.arange(200) * 5 + 3) % D] = 3.0
    x[2] = 0.0
    x[2, 1::2] = -0.0
    x[2, 7::50] = 1.0
    x[2, 9::50] = -1.0
    x[3, [5, 64, D - 1]] = INF
    x[3, [0, D // 3, D - 2]] = -INF
    x[4] = INF
    x[5] = -INF
    return x.to(dt)


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("D,k,tag", [(1000, 10, "topk_wave"), (1001, 10, "topk_wave"), (1000, 64, "topk_wave"), (300, 65, "topk_rounds")],
                         ids=["vec", "scalar", "k64", "rounds"])
def test_topk_ties_zeros_infinities(gpu, dt, largest, D, k, tag):
    _check_topk(_tie_rows(D, dt), k, 1, largest, tag)


def _nan_rows(D, dt):
    """one NaN: at 0; at 37 (a lane's first element in the scalar scan, inside a lane's first four in the other); at 40 (the first of a
    lane's four); at 700 (past every lane's first trip); at D - 1.  All NaN; 70 NaN (for `largest` more than 64 tie at the threshold);
    none.  In a row shorter than a position the position wraps."""
    x = closed_form((8, D), 5, 2.0, F64)
    for r, p in enumerate((0, 37, 40, 700, D - 1)):
        x[r, p % D] = NAN
    x[5] = NAN
    x[6, (torch.arange(70) * 3 + 2) % D] = NAN
    return x.to(dt)


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("largest", [False, True], ids=["smallest", "largest"])
@pytest.mark.parametrize("D,k,tag", [(1000, 10, "topk_wave"), (1001, 10, "topk_wave"), (100, 30, "topk_wave"), (5, 5, "topk_wave"), (1000, 64, "topk_wave"),
                                     (300, 65, "topk_rounds"), (300, 300, "topk_rounds")],
                         ids=["vec", "scalar", "short-rows", "k-is-D", "k64", "rounds", "rounds-k-is-D"])
def test_topk_nan_is_the_greatest_value(gpu, dt, largest, D, k, tag):
    """ATen's order: `largest` returns the NaN first, the smallest k skip them unless the row runs out of numbers.  Before this test
    the kernels compared with < and == alone: a lane whose first element was NaN kept it as its minimum, the threshold could become NaN
    and the row came back as zeros with index -1; a NaN elsewhere was never selected."""
    _check_topk(_nan_rows(D, dt), k, 1, largest, tag)


# ---- row gather ----------------------------------------------------------------------------------------------------------------------------
def _indices(J, D):
    """J indices into D rows: repeats (every fifth is the first) and negative ones (every third counts from the end)"""
    idx = (torch.arange(J) * 37 + 11) % D
    idx[1::5] = idx[0]
    idx[2::3] -= D
    return idx


@pytest.mark.parametrize("dt", ALL, ids=dtid)
@pytest.mark.parametrize("J", [1, 255, 257])
def test_index_select_forms(gpu, dt, J):
    w = W(dt)
    idx = _indices(J, 500)
    for what, width, put, dim, tag in (("rows of 4 packets", 4 * w, aligned, 0, "index_select_rows_vec"),
                                       ("rows off a packet", 4 * w + 1, aligned, 0, "index_select"),
                                       ("misaligned table", 4 * w, misaligned, 0, "index_select"),
                                       ("dim 1", 4 * w, aligned, 1, "index_select")):
        x = _data((500, width) if dim == 0 else (width, 500), 3, dt)
        with launched() as L:
            got = to_torch(put(x).indexSelect(dim, to_sten(idx)))
        ran = {t: L.count(t) for t in L if t.startswith("index_select")}
        assert ran == {tag: 1}, f"{what}: launched {ran}, written for {tag}"
        assert torch.equal(got.double(), x.index_select(dim, idx % 500).double()), what


# ---- embedding -----------------------------------------------------------------------------------------------------------------------------
def _emb_bwd(g, idx, num_weights, padding_idx):
    o = C.c_void_p()
    lib.lamp_embedding_backward(C.byref(o), to_sten(g), to_sten(idx), num_weights, padding_idx)
    return to_torch(S.STen(o))


def _emb_ref(g, idx, num_weights, padding_idx):
    ref = torch.zeros(num_weights, g.shape[-1], dtype=F64).index_add_(0, idx.reshape(-1), g.double().reshape(-1, g.shape[-1]))
    if padding_idx >= 0:
        ref[padding_idx] = 0.0
    return ref


def _tokens(N, nw):
    """rows r % 3 == 1 are never referenced (but for the last row); the first and the last row are: both are padding rows below"""
    idx = (torch.arange(N) * 7) % nw
    idx = idx - (idx % 3 == 1).long()
    idx[0], idx[-1] = 0, nw - 1
    return idx


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("N", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("nw,E", [(11, 1), (50, 300), (1000, 64)], ids=["11x1", "50x300", "1000x64"])
def test_embedding_and_its_scan_backward(gpu, dt, N, nw, E):
    """forward: the row gather (E = 64: packets).  Backward, scan form: integer gradients - the result EQUALS the float64 sum rounded
    once; positive closed-form gradients at FWD_TOL, cancelling ones at the rounding bound of a sum of n terms.  N on both sides of the 256-token trip, E on both sides of the 256-column block."""
    weight = closed_form((nw, E), 3, 2.0, dt)
    for idx in (_tokens(N, nw), torch.full((N,), 5 % nw), _tokens(N, nw).reshape(7, 100) if N == 700 else None):
        if idx is None:
            continue
        o = C.c_void_p()
        lib.lamp_embedding(C.byref(o), to_sten(weight), to_sten(idx))
        got = to_torch(S.STen(o))
        assert list(got.shape) == list(idx.shape) + [E] and torch.equal(got.double(), weight[idx].double()), "embedding"
        unused = torch.ones(nw, dtype=torch.bool)
        unused[idx.reshape(-1)] = False
        for pad in (-1, 0, nw - 1):
            g = small_ints(tuple(idx.shape) + (E,), 9, dt)
            with launched() as L:
                got = _emb_bwd(g, idx, nw, pad)
            assert L.count("embedding_bwd_scan") == 1 and L.count("index_add") == 0
            ref = _emb_ref(g, idx, nw, pad)
            assert ref.abs().max().item() < 2 ** 24
            assert torch.equal(got.double(), ref.to(dt).double()), f"padding_idx={pad}: integer gradients"
            assert not got[unused].any() and (pad < 0 or not got[pad].any())
            # in [0.5, 1.5]: the kernel adds up to 700 of them in f32, and a tolerance relative to the sum needs terms that do not cancel
            g = closed_form(tuple(idx.shape) + (E,), 9, 1.0, dt) + 1.0
            with launched() as L:
                got = _emb_bwd(g, idx, nw, pad)
            assert L.count("embedding_bwd_scan") == 1 and L.count("index_add") == 0
            assert_close(got, _emb_ref(g, idx, nw, pad), FWD_TOL[dt], f"padding_idx={pad}: closed-form gradients")
            # gradients in [-0.5, 0.5] that cancel: a row's n gradients are added one after the other in f32 (f64 for f64), which stays
            # within (n - 1) u of the sum of their magnitudes (u = 2^-24, 2^-53; 1 % for the higher-order terms), and bf16 rounds the
            # f32 sum once more (8 bits: 2^-8)
            g = closed_form(tuple(idx.shape) + (E,), 9, 1.0, dt)
            ref, mag = _emb_ref(g, idx, nw, pad), _emb_ref(g.abs(), idx, nw, pad)
            n = torch.bincount(idx.reshape(-1), minlength=nw).double()[:, None]
            bound = 1.01 * (n - 1).clamp(min=0) * (2.0 ** -53 if dt == F64 else 2.0 ** -24) * mag
            if dt == BF16:
                bound = bound + 2.0 ** -8 * (ref.abs() + bound)
            with launched() as L:
                got = _emb_bwd(g, idx, nw, pad)
            assert L.count("embedding_bwd_scan") == 1 and L.count("index_add") == 0
            err = (got.double() - ref).abs()
            assert bool((err <= bound).all()), f"padding_idx={pad}: cancelling gradients: {int((err > bound).sum())} outside the bound of n terms"


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
def test_embedding_backward_falls_back_to_index_add(gpu, dt):
    """70000 x 4096 > 2^28 row-token pairs: zero fill + atomic index_add.  Each of 1000 rows (and the last one) is hit four times with
    integers in [-3, 3]: |sum| <= 12 whatever the order; E = 8 puts four pairs of bf16 columns into shared 32-bit words."""
    nw, N, E = 70000, 4096, 8
    idx = (torch.arange(N) * 17) % 1000 * 70
    idx[::1024] = nw - 1
    g = small_ints((N, E), 9, dt)
    unused = torch.ones(nw, dtype=torch.bool)
    unused[idx] = False
    for pad in (-1, 0, nw - 1):
        with launched() as L:
            got = _emb_bwd(g, idx, nw, pad)
        assert L.count("index_add") == 1 and L.count("embedding_bwd_scan") == 0
        ref = _emb_ref(g, idx, nw, pad)
        assert ref.abs().max().item() <= 256
        assert torch.equal(got.double(), ref), f"padding_idx={pad}"
        assert not got[unused].any()


# ---- index_add, scatter_add, gather -----------------------------------------------------------------------------------------------------------
SIZES = [(300, 7), (64, 33), (4, 5, 6)]


@pytest.mark.parametrize("dt", ALL, ids=dtid)
@pytest.mark.parametrize("shape", SIZES, ids=["300x7", "64x33", "4x5x6"])
def test_index_add_scatter_add_gather(gpu, dt, shape):
    """every dim.  The 2 D + 3 sources of index_add hit every slice two or three times, so along the last dim both 16-bit halves of every
    32-bit word take duplicates at once; odd row widths (7, 33) move the halves from row to row.  Integers in [-3, 3]: |sum| <= 12."""
    x = small_ints(shape, 3, dt)
    X = to_sten(x)
    for dim in range(len(shape)):
        D = shape[dim]
        J = 2 * D + 3
        idx = (torch.arange(J) * 5 + 2) % D
        sshape = list(shape)
        sshape[dim] = J
        src = small_ints(sshape, 9, dt)
        with launched() as L:
            got = to_torch(X.indexAdd(dim, to_sten(idx), to_sten(src)))
        assert L.count("index_add") == 1
        ref = x.double().index_add(dim, idx, src.double())
        assert ref.abs().max().item() <= 256
        assert torch.equal(got.double(), ref), f"index_add dim {dim}"
        # scatter_add / gather: an index of the source's shape, neighbours along the last dim often one element apart
        index = (small_ints(sshape, 21, I64, 1000) + 1000 + torch.arange(sshape[-1])) % D
        o = C.c_void_p()
        lib.lamp_scatter_add(C.byref(o), X, dim, to_sten(index), to_sten(src))
        ref = x.double().scatter_add(dim, index, src.double())
        assert ref.abs().max().item() <= 256
        assert torch.equal(to_torch(S.STen(o)).double(), ref), f"scatter_add dim {dim}"
        table = _data(shape, 5, dt)
        o = C.c_void_p()
        lib.lamp_gather(C.byref(o), to_sten(table), dim, to_sten(index))
        assert torch.equal(to_torch(S.STen(o)).double(), torch.gather(table, dim, index).double()), f"gather dim {dim}"
