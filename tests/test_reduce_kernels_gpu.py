"""Every kernel form of the reductions (kernels/reduce.hip) against plain float64 formulas.

reduce_typed views the contiguous input as [K0, R1, K1, R2] (R1, R2 reduced) and picks, from those four numbers, the element size, the
pointer alignment and the number of compute units (W = 16 / sizeof(T) elements per 16-byte packet):
  reduce_block        a workgroup of 64 / 128 / 256 threads per output, over one contiguous run or (R1, K1 > 1) a strided one
  reduce_column       R2 == 1, K1 >= 64: a thread per column
  reduce_column_vec   the same in packets: K1 % W == 0, R1 >= 64, a 16-byte aligned pointer, K0 <= 65535 (K0 rides on blockIdx.z)
  reduce_generic      more than two reduced groups: a thread per output over stride tables
each of the first three split 1 .. 1024 ways over blockIdx.y when the outputs alone do not fill the device, and finished by
reduce_finalize or (nsplit >= 16) reduce_finalize_wide.  Every case below states the form and the split it was written for - worked out
for the 256 compute units of an MI355X, where the chooser aims at target_blocks = 1024 workgroups - and asserts both through the kernel
timers: the tag of the launch, and nsplit as the finalize kernel's declared work divided by the number of outputs.  tests/form_ref.py mirrors the chooser and
tests/test_form_ref.py checks the table against the mirror without a GPU.  f64 needs 32 packets for K1 >= 64, so the W-relative column
cases take the block form there; the "x2" cases run the column forms in f64 with twice the packets.

References are float64 torch expressions of the inputs AFTER rounding to the dtype under test; the tolerances are test_reductions'
(tests/test_ops_gpu.py).  Those are relative to a tensor's mean magnitude, which hides one lost packet or row, hence the probes:
  exact     integers in [-3, 3]: every partial sum (of the values or of their squares) is an integer below 2^24, exact in f32 and f64 in
            any order, so sum and norm2 must EQUAL the float64 result rounded once to the dtype (f64 norm2: to one unit in the last
            place, which is the device library's square root; max / min: the maxAll / minAll tests)
  position  zeros but for one row (or one run position) of ones: the result is exactly 1 where that row counts and 0 elsewhere; a
            skipped row shows as 0, one added twice as 2
Not covered: K0 > 65535 (the packet column form falling back to the scalar one) needs an input of at least 512 MB."""
import numpy as np
import pytest
import torch

from tests import form_ref as FR
from tests.form_ref import BF16, F32, F64, I64, ITEM, W, aligned, dtid, launched, misaligned, small_ints
from tests.util import DTYPES, FWD_TOL, assert_close, closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu

B, C_, CV, G = "reduce_block", "reduce_column", "reduce_column_vec", "reduce_generic"
FIN, WIDE = "reduce_finalize", "reduce_finalize_wide"
# id: (shape - an int, or (packets, plus) for a width of packets * W + plus -, reduced dims, (tag, nsplit, finalize) for f32 / bf16 and
#      for the f64 "x2" cases, the same for f64 where it differs, handed over misaligned)
CASES = {
    "run-64-threads":      ((37, 64), [1], (B, 1, FIN), None, False),
    "run-128-threads":     ((37, 65), [1], (B, 1, FIN), None, False),
    "run-256-threads":     ((37, 300), [1], (B, 1, FIN), None, False),
    "run-split-4":         ((5, 9000), [1], (B, 4, FIN), None, False),
    "run-split-34":        ((3, 70001), [1], (B, 34, WIDE), None, False),
    "all-split-1024":      ((2100000,), [], (B, 1024, WIDE), None, False),
    "strided-4d":          ((3, 7, 5, 33), [1, 3], (B, 1, FIN), None, False),
    "strided-3d":          ((7, 5, 33), [0, 2], (B, 1, FIN), None, False),
    "column-few-rows":     ((6, 120), [0], (C_, 1, FIN), None, False),
    "column-off-packet":   ((300, (17, 2)), [0], (C_, 4, FIN), (B, 1, FIN), False),
    "column-misaligned":   ((128, (16, 0)), [0], (C_, 1, FIN), (B, 1, FIN), True),
    "vec-minimum":         ((64, (16, 0)), [0], (CV, 1, FIN), (B, 1, FIN), False),
    "vec-ragged":          ((71, (17, 0)), [0], (CV, 1, FIN), (B, 1, FIN), False),
    "vec-second-x-block":  ((89, (33, 0)), [0], (CV, 1, FIN), None, False),
    "vec-k0":              ((3, 70, (16, 0)), [1], (CV, 1, FIN), (B, 1, FIN), False),
    "vec-split-4":         ((257, (16, 0)), [0], (CV, 4, FIN), (B, 1, FIN), False),
    "vec-split-15":        ((1000, (16, 0)), [0], (CV, 15, FIN), (B, 1, FIN), False),
    "vec-split-16-wide":   ((1024, (64, 0)), [0], (CV, 16, WIDE), None, False),
    "vec-split-256-empty": ((16385, (16, 0)), [0], (CV, 256, WIDE), (B, 8, FIN), False),
    "generic-4d":          ((6, 5, 8, 3), [0, 2], (G, 1, None), None, False),
    "generic-5d":          ((2, 3, 4, 5, 6), [0, 2, 4], (G, 1, None), None, False),
}
X2 = [k for k, v in CASES.items() if v[3] is not None]       # the cases f64 repeats with twice the packets


def case_shape(name, dt, x2=False):
    """x2: twice the packets, and one element instead of two off a packet (W = 2: two elements are a packet)"""
    w = W(dt)
    return tuple(s if isinstance(s, int) else (2 * s[0] * w + (1 if s[1] else 0) if x2 else s[0] * w + s[1]) for s in CASES[name][0])


def case_expect(name, dt, x2=False):
    _, _, narrow, wide, _ = CASES[name]
    return wide if (ITEM[dt] == 8 and not x2 and wide is not None) else narrow


PARAMS = [pytest.param(dt, k, False, id=f"{dtid(dt)}-{k}") for dt in DTYPES + [I64] for k in CASES] + \
         [pytest.param(dt, k, True, id=f"{dtid(dt)}-{k}-x2") for dt in (F64, I64) for k in X2]


def _put(x, name):
    return misaligned(x) if CASES[name][4] else aligned(x)


def _expect_launch(L, expect, nout, what):
    tag, nsplit, fin = expect
    ran = {t: L.count(t) for t in L if t.startswith("reduce_")}
    assert ran == ({tag: 1} if fin is None else {tag: 1, fin: 1}), f"{what}: launched {ran}, written for {expect}"
    if fin is not None:
        # the report carries seven significant digits; the largest product here is 256 x 128 = 32768
        assert nsplit * nout < 10 ** 7 and L.work(fin) == nsplit * nout, f"{what}: split {L.work(fin) / nout} ways, written for {nsplit}"


def _nout(shape, dims):
    return int(np.prod([s for i, s in enumerate(shape) if dims and i not in dims]))


@pytest.mark.parametrize("dt,name,x2", PARAMS)
def test_reduction_forms(gpu, dt, name, x2):
    shape, dims, expect = case_shape(name, dt, x2), CASES[name][1], case_expect(name, dt, x2)
    nout = _nout(shape, dims)
    full = not dims
    if dt == I64:
        x = small_ints(shape, 3, I64, 1000)
        with launched() as L:
            got = to_torch(_put(x, name).sum(dims, False))
        _expect_launch(L, expect, nout, "sum")
        assert torch.equal(got, x.sum(dims) if dims else x.sum())
        return
    x = closed_form(shape, 3, 2.0, dt)
    X, xd = _put(x, name), x.double()
    tol = FWD_TOL[dt] * 4
    stol = tol * (8 if full or (expect[0] == B and expect[1] > 1) else 4)      # test_reductions: "sum all" and "long rows" 8, else 4
    rdims = dims or list(range(len(shape)))
    with launched() as L:
        got = to_torch(X.sum(dims, False) if dims else X.sum())
    _expect_launch(L, expect, nout, "sum")
    assert_close(got, xd.sum(rdims), stol, "sum")
    assert_close(to_torch(X.sum(rdims, True)), xd.sum(rdims, keepdim=True), stol, "sum keepdim")
    assert_close(to_torch(X.mean(dims, False) if dims else X.mean()), xd.mean(rdims), tol * 4, "mean")
    with launched() as L:
        got = to_torch(X.norm2(rdims, True))
    _expect_launch(L, expect, nout, "norm2")
    assert_close(got, torch.linalg.vector_norm(xd, 2, rdims, True), tol, "norm2")
    for unbiased in (False, True):
        v, m = X.varAndMean(rdims, unbiased, True)
        rv, rm = torch.var_mean(xd, rdims, unbiased=unbiased, keepdim=True)
        assert_close(to_torch(v), rv, tol * 4, f"var unbiased={unbiased}")
        assert_close(to_torch(m), rm, tol * 4, "mean of varAndMean")
    target = [1 if i in rdims else s for i, s in enumerate(shape)]
    with launched() as L:
        got = to_torch(X.unbroadcast(target))
    _expect_launch(L, expect, nout, "unbroadcast")
    assert_close(got, xd.sum(rdims, keepdim=True), stol, "unbroadcast")
    if rdims[0] == 0 and rdims == list(range(len(rdims))) and len(rdims) < len(shape):
        assert_close(to_torch(X.unbroadcast(list(shape[len(rdims):]))), xd.sum(rdims), stol, "unbroadcast of leading dims")
    if len(dims) == 1:
        assert np.array_equal(X.argmax(dims[0], False).to_numpy(), torch.argmax(xd, dims[0]).numpy()), "argmax"


def _rounded_once(r64, dt):
    """r64 rounded to dt.  torch rounds float64 -> bfloat16 through float32; the caller's data must make that harmless."""
    if dt == BF16:
        f = r64.float()
        low = f.view(torch.int32) & 0xFFFF
        assert bool(((low != 0x8000) | (f.double() == r64)).all()), "a float32 value on a bfloat16 midpoint: rounded twice"
    return r64.to(dt)


@pytest.mark.parametrize("dt,name,x2", [p for p in PARAMS if p.values[0] != I64])
def test_reduction_forms_exact(gpu, dt, name, x2):
    """integers in [-3, 3]: sum and norm2 equal the float64 results rounded once, in every form.  f32 and bf16 take the root of their exact
    f32 sum of squares in double precision and round that, which hides the last bit of the root.  f64 shows it, and the device library's
    double-precision square root is good to one unit in the last place, not correctly rounded (in one run on an MI355X 6 of the 32 f64
    cases differed from float64 sqrt, in 1 to 6 outputs each): there the root is the reference or one of its two neighbours.  One element lost
    or counted twice moves a sum of squares S by at least 1 and its root by S^-1/2 / 2 > 2^-13 of itself, 2^39 such units."""
    shape, dims, expect = case_shape(name, dt, x2), CASES[name][1], case_expect(name, dt, x2)
    rdims = dims or list(range(len(shape)))
    x = small_ints(shape, 11, dt)
    xd = x.double()
    assert xd.abs().sum().item() < 2 ** 24 and (xd * xd).sum().item() < 2 ** 24
    X = _put(x, name)
    with launched() as L:
        got = to_torch(X.sum(rdims, False))
    _expect_launch(L, expect, _nout(shape, dims), "sum")
    ref = _rounded_once(xd.sum(rdims), dt)
    assert torch.equal(got.double(), ref.double()), f"sum: {int((got.double() != ref.double()).sum())} of {ref.numel()} differ"
    got = to_torch(X.norm2(rdims, False))
    ref = _rounded_once((xd * xd).sum(rdims).sqrt(), dt)
    if dt == F64:
        up, down = (torch.nextafter(ref, torch.full_like(ref, v)) for v in (float("inf"), float("-inf")))
        off = ~((got == ref) | (got == up) | (got == down))
        assert not bool(off.any()), f"norm2: {int(off.sum())} of {ref.numel()} are neither the float64 root nor a neighbour of it"
    else:
        assert torch.equal(got.double(), ref.double()), f"norm2: {int((got.double() != ref.double()).sum())} of {ref.numel()} differ"


def _probe_rows(R, nsplit):
    """row lanes 0, 7, 8 of the packet form's eight and its rows 31, 32 (the four-loads-in-flight trip and the next one), the first and
    the last row of the first two chunks and of the last non-empty one, the last row"""
    edges, _ = FR.split_rows(R, nsplit)
    rows = {0, 7, 8, 31, 32, R - 1}
    for lo, hi in edges[:2] + edges[-1:]:
        rows |= {lo, hi}
    return sorted(r for r in rows if 0 <= r < R)


COLUMN_CASES = [k for k, v in CASES.items() if v[2][0] in (C_, CV)]


@pytest.mark.parametrize("dt,name,x2", [p for p in PARAMS if p.values[0] != I64 and p.values[1] in COLUMN_CASES])
def test_column_reduction_counts_every_row_once(gpu, dt, name, x2):
    """[.., R, K] summed over R.  One row of ones at a time: every column of the result is exactly 1.  Then four single ones, in the first
    and the last element of a row's first and last packet, each in another row: the result is 1 in those four columns and 0 elsewhere."""
    shape, dims, expect = case_shape(name, dt, x2), CASES[name][1], case_expect(name, dt, x2)
    d = dims[0]
    R, K = shape[d], shape[-1]
    if expect[0] == CV:
        _, empty = FR.split_rows(R, expect[1])
        assert empty == (3 if name == "vec-split-256-empty" else 0)
    for r in _probe_rows(R, expect[1]):
        x = torch.zeros(shape, dtype=dt)
        x.select(d, r).fill_(1.0)
        with launched() as L:
            got = to_torch(_put(x, name).sum(dims, False))
        _expect_launch(L, expect, _nout(shape, dims), f"row {r}")
        assert torch.equal(got, torch.ones_like(got)), f"row {r} of {R}: columns {torch.nonzero(got.reshape(-1) != 1).reshape(-1).tolist()[:8]} are not 1"
    w = W(dt)
    x = torch.zeros(shape, dtype=dt)
    cols = [0, w - 1, K - w, K - 1]
    for r, c in zip((R - 1, 0, R // 2, R - 1), cols):
        x.select(d, r)[..., c] = 1.0
    got = to_torch(_put(x, name).sum(dims, False))
    assert torch.equal(got.double(), x.double().sum(dims)) and got.sum().item() == len(cols) * (x.numel() // (R * K))


RUN_CASES = ["run-64-threads", "run-128-threads", "run-256-threads", "run-split-4", "run-split-34", "all-split-1024"]


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("name", RUN_CASES)
def test_run_reduction_counts_every_position_once(gpu, dt, name):
    """[rows, D] summed over D (or one run of D elements).  Row i is zero but for a 1 at position p_i: every sum is exactly 1.  The
    positions: the first and the last thread of a wave and of the workgroup, the first and the last element of the first two chunks
    and of the last one, the last element."""
    shape, dims, expect = case_shape(name, dt), CASES[name][1], case_expect(name, dt)
    D = shape[-1]
    rows = shape[0] if len(shape) == 2 else 1
    edges, empty = FR.split_rows(D, expect[1])
    assert empty == 0
    pos = {0, 63, 64, 255, 256, D - 1}
    for lo, hi in edges[:2] + edges[-1:]:
        pos |= {lo, hi}
    pos = sorted(p for p in pos if 0 <= p < D)
    for at in range(0, len(pos), rows):
        batch = (pos[at:at + rows] * rows)[:rows]              # the last batch repeats its positions to fill the rows
        x = torch.zeros(rows, D, dtype=dt)
        x[torch.arange(rows), torch.tensor(batch)] = 1.0
        with launched() as L:
            got = to_torch(aligned(x.reshape(shape)).sum(dims, False) if dims else aligned(x.reshape(shape)).sum())
        _expect_launch(L, expect, rows, f"positions {batch}")
        assert torch.equal(got.reshape(-1).double(), torch.ones(rows, dtype=F64)), f"positions {batch}: sums {got.reshape(-1).tolist()}"


# ---- maxAll / minAll -----------------------------------------------------------------------------------------------------------------------
ALL_SIZES = [1, 63, 8191, 8193, 2100000]


def _all_positions(n, dt):
    tag, nsplit, fin = FR.reduce_plan((n,), [], ITEM[dt], FR.num_cus())
    edges, _ = FR.split_rows(n, nsplit)
    pos = {0, n - 1} | ({255, 256} if n > 256 else set())
    for lo, hi in edges[:2]:
        pos |= {lo, hi}
    pos = sorted(p for p in pos if 0 <= p < n)
    if n > 1000000:                                            # the first, the last of chunk 0, the first of chunk 1, the last
        pos = [0, edges[0][1], edges[1][0], n - 1]
    return pos, (tag, nsplit, fin)


def _max_min(X):
    return to_torch(X.maxAll()), to_torch(X.minAll())


@pytest.mark.parametrize("dt", DTYPES, ids=dtid)
@pytest.mark.parametrize("n", ALL_SIZES)
def test_max_all_min_all(gpu, dt, n):
    """the full reduction with kMax / kMin: exact on closed-form values and on small integers; the extreme value in the first and the
    last position, on both sides of a thread-trip boundary and of a chunk boundary; one NaN in each of those positions (the result is
    NaN, as ATen's); all -inf and all +inf (the identities of the two operations must not leak)"""
    pos, expect = _all_positions(n, dt)
    assert expect == {1: (B, 1, FIN), 63: (B, 1, FIN), 8191: (B, 1, FIN), 8193: (B, 4, FIN), 2100000: (B, 1024, WIDE)}[n]
    for x in (closed_form((n,), 3, 2.0, dt), small_ints((n,), 11, dt)):
        with launched() as L:
            mx, mn = _max_min(to_sten(x))
        assert {t: L.count(t) for t in L if t.startswith("reduce_")} == {expect[0]: 2, expect[2]: 2} and L.work(expect[2]) == expect[1]
        assert list(mx.shape) == [] and torch.equal(mx.double(), x.max().double()) and torch.equal(mn.double(), x.min().double())
    for v in (float("-inf"), float("inf")):
        mx, mn = _max_min(to_sten(torch.full((n,), v, dtype=dt)))
        assert mx.item() == v and mn.item() == v
    base = closed_form((n,), 3, 2.0, dt)
    for i, p in enumerate(pos):
        x = base.clone()
        x[p] = float("nan")
        mx, mn = _max_min(to_sten(x))
        assert torch.isnan(mx).item() and torch.isnan(mn).item(), f"NaN at {p} of {n}: max {mx.item()} min {mn.item()}"
        if n == 1:
            continue
        q = pos[(i + 1) % len(pos)]
        x = base.clone()
        x[p], x[q] = 5.0, -5.0
        mx, mn = _max_min(to_sten(x))
        assert mx.item() == 5.0 and mn.item() == -5.0, f"max at {p}, min at {q} of {n}: got {mx.item()}, {mn.item()}"
