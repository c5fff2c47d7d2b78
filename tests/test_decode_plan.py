"""The launch of the split-K weight-streaming decode kernels (kernels/decode_stream.h: dec_form, dec_plan, dec_rt), asked through
lamp_debug_decode_plan on a box without a GPU: 256 compute units passed in, w on a 16-byte boundary unless said otherwise.

The expectations were worked out by hand from dec_linear_run and rd_step_run as they stood before dec_plan existed (each with its own copy of
the arithmetic): tiles = ceil(N / (64 CL)); want = ceil(CUs / 2 / tiles), at most 16 slices (8 beyond four rows) and at most
K sizeof(T) / (R sizeof(acc)); Kc = ceil(K / want) raised to 64 and to a multiple of 32, at most 256; S = ceil(K / Kc).  Twelve launches
were confirmed on an MI355X (256 CUs) against grid.x / grid.y in a kernel trace of that older library (EXPERIMENTS.md, "Decode kernels:
one skeleton, one host plan")."""
import pytest
import torch

from tests.util import decode_plan

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ROWS = (1, 2, 4, 5, 16)
PACKET = {F32: 4, F64: 2, BF16: 8}

# (K, N) -> rows -> (tiles, Kc, S) for f32, f64, bf16
LINEAR = [
    ((12, 36), ROWS, ((1, 64, 1), (1, 64, 1), (1, 64, 1))),
    ((13, 19), ROWS, ((1, 64, 1), (1, 64, 1), (1, 64, 1))),
    ((48, 12), ROWS, ((1, 64, 1), (1, 64, 1), (1, 64, 1))),
    ((64, 256), ROWS, ((1, 64, 1), (2, 64, 1), (1, 64, 1))),
    ((65, 256), ROWS, ((1, 64, 2), (2, 64, 2), (1, 64, 2))),
    ((300, 4096), ROWS, ((16, 64, 5), (32, 96, 4), (8, 64, 5))),
    ((3072, 768), (1, 2, 4), ((3, 192, 16), (6, 192, 16), (2, 192, 16))),
    ((3072, 768), (16,), ((3, 256, 12), (6, 256, 12), (2, 256, 12))),
    ((1024, 50000), ROWS, ((196, 256, 4), (391, 256, 4), (98, 256, 4))),
]
# E = 8: (H, rows) -> form -> {dtype: (tiles, Kc, S)}
STEP = [
    (5, ROWS, {"rnn": {F32: (1, 64, 1), F64: (1, 64, 1)}, "gru": {F32: (1, 64, 1), F64: (1, 64, 1)}, "lstm": {F32: (1, 64, 1), F64: (1, 64, 1)},
               "gru2": {F32: (1, 64, 1), F64: (1, 64, 1)}}),
    (64, ROWS, {"rnn": {F32: (1, 64, 2), F64: (1, 64, 2)}, "gru": {F32: (1, 64, 2), F64: (1, 64, 2)}, "lstm": {F32: (1, 64, 2), F64: (1, 64, 2)},
                "gru2": {F32: (1, 64, 1), F64: (1, 64, 1)}}),
    (320, ROWS, {"rnn": {F32: (2, 64, 6), F64: (3, 64, 6)}, "gru": {F32: (5, 64, 6), F64: (5, 64, 6)}, "lstm": {F32: (5, 64, 6), F64: (5, 64, 6)},
                 "gru2": {F32: (2, 64, 5), F64: (3, 64, 5)}}),
    # the shape of tests/test_text_gpu.py whose slab reduction runs a partial second batch of eight
    (640, (1, 3), {"rnn": {F32: (3, 64, 11), F64: (5, 64, 11)}, "gru": {F32: (10, 64, 11), F64: (10, 64, 11)},
                   "lstm": {F32: (10, 64, 11), F64: (10, 64, 11)}, "gru2": {F32: (3, 64, 10), F64: (5, 64, 10)}}),
]


def _check(p, want, cl, v, unroll, R):
    tiles, kc, s = want
    assert (p["tiles"], p["kc"], p["s"]) == want
    assert p["grid"] == (tiles, s) and p["block"] == 256                      # four waves; blockIdx.x the column tile, blockIdx.y the slice
    assert (p["cl"], p["v"], p["unroll"]) == (cl, v, unroll)
    assert p["rt"] == (1 if R == 1 else 4 if R <= 4 else 16)


@pytest.mark.parametrize("shape,rows,want", LINEAR, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) and len(v) == 2 else None)
def test_linear_plan(shape, rows, want):
    K, N = shape
    for dt, w in zip((F32, F64, BF16), want):
        v = PACKET[dt] if N % PACKET[dt] == 0 else 1
        for R in rows:
            _check(decode_plan(dt, "linear", R, K=K, N=N), w, v, v, 8, R)


@pytest.mark.parametrize("H,rows,want", STEP, ids=lambda v: f"H{v}" if isinstance(v, int) else None)
def test_step_plan(H, rows, want):
    for form, per in want.items():
        for dt, w in per.items():
            n = {"rnn": H, "gru2": H, "gru": 3 * H, "lstm": 4 * H}[form]
            v = 1 if form == "gru" or n % PACKET[dt] else PACKET[dt]          # GRU's three columns are element loads
            cl = {"gru": 3, "lstm": 4}.get(form, v)                           # whole hidden units; RNN and GRU's second phase: one packet
            unroll = 4 if form in ("lstm", "gru") and dt == F64 else 8        # a lane's f64 unit is 32 (24) bytes > a packet: half the steps in flight
            for R in rows:
                _check(decode_plan(dt, form, R, E=8, H=H), w, cl, v, unroll, R)


def test_a_misaligned_w_is_read_by_elements():
    """V = 1; the cells keep their CL (and f64 LSTM and GRU their unroll of 4), the others fall to one column per lane and so to more tiles"""
    _check(decode_plan(F32, "linear", 1, K=3072, N=768, aligned=False), (12, 256, 12), 1, 1, 8, 1)     # want = ceil(128 / 12) = 11: Kc 280 -> 256
    _check(decode_plan(BF16, "linear", 16, K=64, N=256, aligned=False), (4, 64, 1), 1, 1, 8, 16)
    _check(decode_plan(F32, "rnn", 3, E=8, H=320, aligned=False), (5, 64, 6), 1, 1, 8, 3)
    _check(decode_plan(F32, "gru2", 3, E=8, H=320, aligned=False), (5, 64, 5), 1, 1, 8, 3)
    _check(decode_plan(F32, "lstm", 3, E=8, H=320, aligned=False), (5, 64, 6), 4, 1, 8, 3)
    _check(decode_plan(F64, "lstm", 3, E=8, H=320, aligned=False), (5, 64, 6), 4, 1, 4, 3)
    _check(decode_plan(F32, "gru", 3, E=8, H=320, aligned=False), (5, 64, 6), 3, 1, 8, 3)
    _check(decode_plan(F64, "gru", 3, E=8, H=320, aligned=False), (5, 64, 6), 3, 1, 4, 3)


def test_the_slices_follow_the_cu_count():
    """16 tiles: on 256 CUs want = ceil(128 / 16) = 8 slices, K = 300 gives 5 of 64; on 64 CUs want = 2, Kc = 150 -> 160, 2 slices; on 32
    CUs want = 1 and the product is not split (Kc is the LDS image's 256, 2 slices of K all the same)"""
    assert [decode_plan(F32, "linear", 1, K=300, N=4096, cus=c)[k] for c in (256, 64) for k in ("tiles", "kc", "s")] == [16, 64, 5, 16, 160, 2]
    assert [decode_plan(F32, "linear", 1, K=300, N=4096, cus=32)[k] for k in ("tiles", "kc", "s")] == [16, 256, 2]
    assert [decode_plan(F32, "linear", 1, K=200, N=4096, cus=32)[k] for k in ("tiles", "kc", "s")] == [16, 224, 1]


def test_more_than_4096_tiles_are_refused():
    assert decode_plan(F32, "linear", 1, K=64, N=4096 * 64, aligned=False)["tiles"] == 4096
    with pytest.raises(Exception, match="tiles"):
        decode_plan(F32, "linear", 1, K=64, N=4096 * 64 + 1, aligned=False)
