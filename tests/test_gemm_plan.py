"""Which kernel form a dense product takes (gemm.hip's gemm_plan and tail split), asked through lamp_debug_gemm_plan on a box without a
GPU: 256 compute units passed in, default switches.

The expectations were worked out by hand from the dispatcher as it stood before gemm_plan existed, and every shape row was then
confirmed on an MI355X (256 CUs) against a kernel trace of that older library: kernel name, grid x and grid z give form, tile count
and split, two GEMM launches give a tail split.  The trace agreed with the hand-made table in every row (EXPERIMENTS.md, entry 83).
Block sizes and LDS bytes are the constants of the four launch sites of that dispatcher: 256 threads / 4 x 16 KiB for the 128 x 128
kernel, 512 / 3 x 48 KiB for 256 x 128, 512 / 2 x 64 KiB for 256 x 256, 256 / none for the f32 / f64 kernels."""
import pytest
import torch

from tests.util import gemm_plan

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
LAYOUTS = [(True, False), (True, True), (False, False), (False, True)]      # (a_kc, b_kc): a, a . b^T, a^T . b, a^T . b^T
GEOMETRY = {"128x128": (256, 65536), "256x128": (512, 147456), "256x256": (512, 131072), "256x256-splitk": (512, 131072),
            "fp64x64": (256, 0), "fp64x64-splitk": (256, 0), "f32-128x128": (256, 0)}

# (batch, M, N, K) -> parts of (form, rows, tiles, split, K per slice)
BF16_ROWS = [
    ((1, 64, 64, 64), [("128x128", 64, 1, 1, 64)]),
    ((1, 130, 70, 45), [("128x128", 130, 2, 1, 45)]),
    ((1, 2048, 2048, 64), [("256x128", 2048, 128, 1, 64)]),
    ((1, 2048, 2048, 192), [("256x128", 2048, 128, 1, 192)]),
    ((1, 2048, 2048, 256), [("256x128", 2048, 128, 1, 256)]),
    ((1, 2048, 2048, 512), [("256x128", 2048, 128, 1, 512)]),
    ((1, 2048, 1024, 128), [("128x128", 2048, 128, 1, 128)]),                   # 64 half tiles < 128
    ((1, 4096, 2048, 64), [("256x128", 4096, 256, 1, 64)]),
    ((1, 3072, 3072, 768), [("256x256", 3072, 144, 1, 768)]),                   # the round-cost rule
    ((1, 3072, 768, 768), [("128x128", 3072, 144, 1, 768)]),                    # beats the split
    ((1, 4096, 4096, 128), [("256x256", 4096, 256, 1, 128)]),
    ((1, 4096, 4096, 192), [("256x256", 4096, 256, 1, 192)]),
    ((1, 4096, 4096, 4096), [("256x256", 4096, 256, 1, 4096)]),
    ((1, 2048, 2048, 2048), [("256x256-splitk", 2048, 64, 2, 1024)]),
    ((1, 768, 768, 12288), [("256x256-splitk", 768, 9, 16, 768)]),
    ((1, 768, 3072, 4096), [("256x256-splitk", 768, 36, 4, 1024)]),
    ((1, 256, 768, 6144), [("128x128", 256, 12, 1, 6144)]),
    ((1, 512, 256, 2048), [("128x128", 512, 8, 1, 2048)]),
    ((1, 256, 256, 4096), [("128x128", 256, 4, 1, 4096)]),                      # split x tiles < 64
    ((1, 22016, 768, 768), [("256x256", 22016, 258, 1, 768)]),                  # K < 2048: no tail split
    ((1, 24576, 768, 2048), [("256x256", 21760, 255, 1, 2048), ("256x256-splitk", 2816, 33, 4, 512)]),
    ((1, 24576, 768, 3072), [("256x256", 21760, 255, 1, 3072), ("256x256-splitk", 2816, 33, 4, 768)]),
    ((1, 16640, 1024, 2048), [("256x256", 16384, 256, 1, 2048), ("128x128", 256, 16, 1, 2048)]),
    ((128, 256, 128, 64), [("256x128", 256, 1, 1, 64)]),                        # 128 tiles over the batch
    ((200, 256, 256, 64), [("256x256", 256, 1, 1, 64)]),                        # 200 tiles over the batch
    ((3, 33, 17, 65), [("128x128", 33, 1, 1, 65)]),
]
FP_ROWS = [
    ((1, 1024, 256, 784), ("fp64x64-splitk", 64, 7, 112)),
    ((1, 784, 256, 1024), ("fp64x64-splitk", 52, 10, 112)),
    ((1, 256, 10, 1024), ("fp64x64-splitk", 4, 16, 64)),
    ((1, 100, 60, 1000), ("fp64x64-splitk", 2, 13, 80)),
    ((1, 64, 64, 130), ("fp64x64-splitk", 1, 2, 80)),
    ((1, 1, 300, 4097), ("fp64x64-splitk", 5, 29, 144)),
    ((1, 64, 64, 128), ("fp64x64-splitk", 1, 2, 64)),
    ((1, 64, 64, 127), ("fp64x64", 1, 1, 127)),
]


def _check(parts, want, batch):
    got = [(p["form"], p["rows"], p["tiles"], p["split"], p["kchunk"]) for p in parts]
    assert got == want
    for p in parts:
        assert (p["block"], p["lds"]) == GEOMETRY[p["form"]]
        assert p["batch"] == batch                                            # blockIdx.z of an unsplit form; no split form is batched
        assert p["split"] == 1 or batch == 1


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("shape,want", BF16_ROWS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_bf16_plan(shape, want, a_kc, b_kc):
    batch, M, N, K = shape
    _check(gemm_plan(BF16, M, N, K, batch, a_kc, b_kc), want, batch)


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("shape", [s for s, _ in BF16_ROWS], ids=lambda v: "x".join(map(str, v)))
def test_f16_is_always_the_128_tile(shape, a_kc, b_kc):
    batch, M, N, K = shape
    _check(gemm_plan(F16, M, N, K, batch, a_kc, b_kc), [("128x128", M, -(-M // 128) * -(-N // 128), 1, K)], batch)


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("shape,want", FP_ROWS, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else None)
def test_f32_f64_split_plan(shape, want, dt, a_kc, b_kc):
    batch, M, N, K = shape
    form, tiles, split, kchunk = want
    _check(gemm_plan(dt, M, N, K, batch, a_kc, b_kc), [(form, M, tiles, split, kchunk)], batch)


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_f32_big_tile_is_f32_only_and_needs_128_tiles(a_kc, b_kc):
    _check(gemm_plan(F32, 2048, 2048, 2048, 1, a_kc, b_kc), [("f32-128x128", 2048, 256, 1, 2048)], 1)
    _check(gemm_plan(F64, 2048, 2048, 2048, 1, a_kc, b_kc), [("fp64x64", 2048, 1024, 1, 2048)], 1)
    _check(gemm_plan(F32, 1024, 1024, 64, 1, a_kc, b_kc), [("fp64x64", 1024, 256, 1, 64)], 1)          # 64 big tiles < 128


@pytest.mark.parametrize("dt", [F32, F64])
def test_knn_epilogue_keeps_the_unsplit_kernel(dt):
    _check(gemm_plan(dt, 64, 64, 130, 1, True, True, knn=True), [("fp64x64", 64, 1, 1, 130)], 1)
    _check(gemm_plan(dt, 64, 64, 130, 1, True, True), [("fp64x64-splitk", 64, 1, 2, 80)], 1)


@pytest.mark.parametrize("M,N,K,ok", [(2048, 2048, 256, ("256x128", 128)), (4096, 4096, 128, ("256x256", 256))])
def test_bf16_big_rule_rejection_edges(M, N, K, ok):
    """each condition of the LDS-DMA kernels on its own: one operand pointer off 16 bytes, C off 8 bytes, ldc % 4 != 0, lda or
    ldb % 8 != 0 - the product falls to the bounds-checked 128 x 128 kernel (K < 512: no split-K either)"""
    t128 = (M // 128) * (N // 128)
    assert [(p["form"], p["tiles"], p["vec"]) for p in gemm_plan(BF16, M, N, K)] == [ok + ("11",)]
    assert [(p["form"], p["tiles"], p["vec"]) for p in gemm_plan(BF16, M, N, K, has_self=True)] == [ok + ("11",)]
    for kw, vec in ((dict(align=(8, 0, 0)), "01"), (dict(align=(0, 8, 0)), "10"), (dict(align=(0, 0, 4)), "11"), (dict(ldc=N + 2), "11"),
                    (dict(lda=K + 4), "01"), (dict(ldb=N + 4), "10"), (dict(ldc=N + 4), None)):
        parts = gemm_plan(BF16, M, N, K, **kw)
        if vec is None:                                                       # a padded but aligned ldc is no rejection
            assert [(p["form"], p["tiles"]) for p in parts] == [ok], kw
        else:
            assert [(p["form"], p["tiles"], p["vec"]) for p in parts] == [("128x128", t128, vec)], kw


def test_tail_split_follows_the_cu_count():
    """288 tiles of 256 x 256: on 256 CUs the last round holds 32 tiles (an eighth of the device) and its rows become a second
    product; on 304 CUs the tiles fit one round and there is one launch"""
    assert [p["rows"] for p in gemm_plan(BF16, 24576, 768, 2048, cus=256)] == [21760, 2816]
    assert [(p["form"], p["rows"], p["tiles"]) for p in gemm_plan(BF16, 24576, 768, 2048, cus=304)] == [("256x256", 24576, 288)]
