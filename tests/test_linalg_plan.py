"""The launch plan of the Cholesky family (kernels/linalg.hip: linalg_plan), asked through lamp_debug_linalg_plan on a box without a GPU:
256 compute units passed in.  Pins the hardware limits, the form threshold, the block tiling, the packing of small matrices and the
workspace for every side up to twice the LDS side and a sample above, and that every decline carries a reason."""
import pytest
import torch

from tests.linalg_ref import linalg_plan

S = linalg_plan("linalg_cholesky", torch.float64, [4, 4])["lds_side"]
NB = linalg_plan("linalg_cholesky", torch.float64, [S + 1, S + 1])["nb"]
SIDES = list(range(1, 2 * S + 2)) + [511, 512, 1000, 4096, 8192]
BATCHES = [1, 3, 4097]
LDS_LIMIT = 160 * 1024


def ceil_div(a, b):
    return (a + b - 1) // b


def check_common(p, n, batch, es):
    assert p["accepted"] == 1 and p["reason"] == "", p
    assert p["n"] == n and p["batch"] == batch
    for k in ("lds_bytes", "potrf_lds_bytes", "solve_lds_bytes"):
        assert 0 <= p[k] <= LDS_LIMIT, (k, p)
    for k in ("threads", "potrf_threads", "solve_threads"):
        assert p[k] <= 1024 and p[k] % 64 == 0, (k, p)
    assert 1 <= p["grid_x"] <= 2 ** 31 - 1 and 1 <= p["grid_y"] <= 65535, p
    assert p["solve_grid_y"] <= 65535 and p["potrf_grid_x"] <= 2 ** 31 - 1 and p["solve_grid_x"] <= 2 ** 31 - 1
    # the LDS form exactly up to the threshold, the blocked form above it
    assert p["form"] == ("lds" if n <= S else "blocked"), p
    nb, steps = p["nb"], p["steps"]
    assert nb == (n if n <= S else NB) and steps == ceil_div(n, nb)
    # the block columns [k nb, min(n, (k + 1) nb)) tile [0, n) once each; only the last may be ragged
    cols = [(k * nb, min(n, (k + 1) * nb)) for k in range(steps)]
    assert cols[0][0] == 0 and cols[-1][1] == n and all(a[1] == b[0] for a, b in zip(cols, cols[1:]))
    assert all(hi - lo == nb for lo, hi in cols[:-1]) and 0 < cols[-1][1] - cols[-1][0] <= nb


def check_potrf_launch(p, side, batch, es):
    mpw, tpm = p["potrf_matrices_per_workgroup"], p["potrf_threads_per_matrix"]
    # matrix m is slot m % mpw of workgroup m // mpw: every matrix exactly once
    assert 1 <= mpw <= batch and p["potrf_grid_x"] == ceil_div(batch, mpw)
    assert p["potrf_threads"] >= mpw * tpm and tpm in (16, 64, 256, 1024)
    if side <= 32 and batch >= 4:
        assert mpw >= 4 and tpm <= 64                     # a wavefront per matrix at the most: small matrices share a workgroup
    ld = p["potrf_ld"]
    assert ld >= side and ld % 2 == 1
    assert p["potrf_lds_bytes"] == mpw * side * ld * es


def check_solve_launch(p, side, batch, nrhs, es):
    mpw, cpw = p["solve_matrices_per_workgroup"], p["solve_columns_per_workgroup"]
    assert 1 <= mpw <= batch and p["solve_grid_x"] == ceil_div(batch, mpw)
    assert 1 <= cpw <= max(nrhs, 1) and p["solve_grid_y"] == ceil_div(nrhs, cpw)        # every column exactly once
    assert mpw * cpw <= p["solve_threads"] <= 256
    n8 = ceil_div(side, 8) * 8
    ld = p["solve_ld"]
    assert ld >= n8 and ld % 2 == 1
    assert p["solve_lds_bytes"] == mpw * n8 * ld * es


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_cholesky_plan(dt):
    es = torch.finfo(dt).bits // 8
    for n in SIDES:
        for batch in BATCHES:
            p = linalg_plan("linalg_cholesky", dt, [batch, n, n] if batch > 1 else [n, n])
            check_common(p, n, batch, es)
            if n <= S:
                check_potrf_launch(p, n, batch, es)
                assert p["workspace_bytes"] == 0 and p["launches"] == 1
                assert (p["threads"], p["grid_x"], p["lds_bytes"]) == (p["potrf_threads"], p["potrf_grid_x"], p["potrf_lds_bytes"])
            else:
                check_potrf_launch(p, NB, batch, es)                       # the diagonal blocks
                check_solve_launch(p, NB, batch, n - NB, es)               # the widest panel: a row of it is a right-hand side
                assert p["workspace_bytes"] == batch * n * n * es          # the lower-triangular working copy
                assert p["launches"] == 2 + p["steps"] + 2 * (p["steps"] - 1)


@pytest.mark.parametrize("op", ["cholesky_solve", "cholesky_inverse", "triangular_solve"])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_solve_plans(op, dt):
    es = torch.finfo(dt).bits // 8
    solves = 1 if op == "triangular_solve" else 2
    for n in SIDES:
        for batch in BATCHES:
            for nrhs in ([n] if op == "cholesky_inverse" else [1, 3, 65]):
                a = [batch, n, n] if batch > 1 else [n, n]
                b = None if op == "cholesky_inverse" else ([batch, n, nrhs] if batch > 1 else [n, nrhs])
                p = linalg_plan(op, dt, a, b)
                check_common(p, n, batch, es)
                assert p["nrhs"] == nrhs and p["workspace_bytes"] == 0     # the solves work in the output
                check_solve_launch(p, min(n, p["nb"]), batch, nrhs, es)
                assert (p["threads"], p["grid_x"], p["grid_y"], p["lds_bytes"]) == (p["solve_threads"], p["solve_grid_x"], p["solve_grid_y"], p["solve_lds_bytes"])
                if n <= S:
                    assert p["launches"] == solves
                else:
                    assert p["launches"] == solves * (2 * p["steps"] - 1) + (1 if op == "cholesky_inverse" else 0)


def test_broadcast_batches_are_planned():
    p = linalg_plan("cholesky_solve", torch.float64, [3, 3], [5, 2, 3, 4])
    assert p["accepted"] == 1 and p["batch"] == 10 and p["nrhs"] == 4
    p = linalg_plan("triangular_solve", torch.float32, [5, 2, 3, 3], [3, 4])
    assert p["accepted"] == 1 and p["batch"] == 10 and p["nrhs"] == 4


def test_few_workgroups_take_narrower_ones():
    """one matrix, many right-hand sides: 64 columns per workgroup until the device is covered (the plan is the only place that knows `cus`)"""
    wide = linalg_plan("triangular_solve", torch.float32, [64, 64], [64, 4096], cus=8)
    narrow = linalg_plan("triangular_solve", torch.float32, [64, 64], [64, 4096], cus=256)
    assert wide["solve_columns_per_workgroup"] == 256 and narrow["solve_columns_per_workgroup"] == 64
    assert narrow["grid_y"] == 64 and wide["grid_y"] == 16


DECLINES = [
    ("linalg_cholesky", torch.bfloat16, [4, 4], None, "f32 and f64"),
    ("linalg_cholesky", torch.float16, [4, 4], None, "f32 and f64"),
    ("triangular_solve", torch.int64, [4, 4], [4, 1], "f32 and f64"),
    ("linalg_cholesky", torch.float32, [3, 4], None, "square"),
    ("cholesky_inverse", torch.float32, [2, 3, 4], None, "square"),
    ("linalg_cholesky", torch.float32, [4], None, "2 dimensions"),
    ("cholesky_solve", torch.float64, [3, 3], [3], "2 dimensions"),
    ("cholesky_solve", torch.float64, [3, 3], [5, 2], "mismatched sizes"),
    ("triangular_solve", torch.float64, [2, 3, 3], [2, 4, 1], "mismatched sizes"),
    ("linalg_cholesky", torch.float32, [46341, 46341], None, "2^31 - 1"),
    ("triangular_solve", torch.float32, [2, 2], [2, 2 ** 30], "2^31 - 1"),
    ("cholesky_solve", torch.float64, [2, 3, 3], [3, 3, 1], "batch shapes"),
    ("cholesky_solve", torch.float64, [2, 3, 3], [2, 2, 3, 1], "batch shapes"),
    ("triangular_solve", torch.float64, [2, 1, 3, 3], [2, 3, 1], "batch shapes"),
    ("cholesky_solve", torch.float64, [3, 3], None, "right-hand side"),
]


@pytest.mark.parametrize("op,dt,a,b,word", DECLINES, ids=[f"{d[0]}-{d[4].replace(' ', '_')}-{i}" for i, d in enumerate(DECLINES)])
def test_declines_carry_a_reason(op, dt, a, b, word):
    p = linalg_plan(op, dt, a, b)
    assert p["accepted"] == 0 and word in p["reason"], p
