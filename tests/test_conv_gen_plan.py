"""The launch plan of the general matrix-core convolution (kernels/conv_gen.hip: gen_plan), asked through lamp_debug_conv_gen_plan on a
box without a GPU, 256 compute units passed in.

The product of a pass is R[U][V] over K (fwd: Cout x pixels over Cin kh kw; dgrad: Cin x input pixels over Cout kh kw; wgrad: Cout x
Cin kh kw over the output pixels).  grid = (V tiles, U tiles, splits); split z owns K range [z k_per_split, min(K, (z + 1) k_per_split)).
"""
import ctypes as C
import os
import re

import pytest
import torch

from lamp_amd._capi import ROOT, i64_array, lib
from tests.conv_gen_cases import CASES, regular_geometry
from tests.util import TORCH2LAMP

FWD, DGRAD, WGRAD = 0, 1, 2
PASSES = {"fwd": FWD, "dgrad": DGRAD, "wgrad": WGRAD}
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


def plan(pass_, dt, dims, taps, groups=1, cus=256):
    buf = C.create_string_buffer(2048)
    lib.lamp_debug_conv_gen_plan(int(pass_), TORCH2LAMP[dt], i64_array(dims), (C.c_int * 8)(*taps), C.c_int64(groups), int(cus), buf, len(buf))
    d = dict(line.split("=", 1) for line in buf.value.decode().splitlines())
    return {k: (v if k == "reason" else int(v)) for k, v in d.items()}


def extents(pass_, dims, taps):
    N, Cin, H, W, Cout, Ho, Wo = dims
    khkw = taps[0] * taps[1]
    return {FWD: (Cout, N * Ho * Wo, Cin * khkw), DGRAD: (Cin, N * H * W, Cout * khkw), WGRAD: (Cout, Cin * khkw, N * Ho * Wo)}[pass_]


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("pn", list(PASSES))
@pytest.mark.parametrize("cid", list(CASES))
def test_plan_covers_the_product(cid, pn, dtn):
    dims, taps = regular_geometry(CASES[cid])
    p = plan(PASSES[pn], DTYPES[dtn], dims, taps)
    assert p["accepted"] == 1, p
    U, V, K = extents(PASSES[pn], dims, taps)
    assert (p["U"], p["V"], p["K"]) == (U, V, K)
    # rows and columns: every element in exactly one tile
    assert p["grid_x"] == -(-V // p["tile_v"]) and p["grid_y"] == -(-U // p["tile_u"])
    # K: split z owns [z len, min(K, (z + 1) len)) - contiguous, in order, none empty, nothing twice; len is whole stages
    splits, klen = p["splits"], p["k_per_split"]
    assert splits >= 1 and p["grid_z"] == splits
    assert klen % p["tile_k"] == 0 and (splits - 1) * klen < K <= splits * klen
    if PASSES[pn] != WGRAD:
        assert splits == 1
    assert p["workspace_bytes"] == (splits * U * V * 4 if splits > 1 else 0)
    assert 0 < p["lds_bytes"] <= 160 * 1024
    assert 1 <= p["grid_x"] <= 2 ** 31 - 1 and 1 <= p["grid_y"] <= 65535 and 1 <= p["grid_z"] <= 65535 and 1 <= p["threads"] <= 1024


@pytest.mark.parametrize("dtn", list(DTYPES))
def test_c5_weight_gradient_splits_k_with_a_ragged_tail(dtn):
    dims, taps = regular_geometry(CASES["C5"])
    p = plan(WGRAD, DTYPES[dtn], dims, taps)
    K = dims[0] * dims[5] * dims[6]
    assert p["accepted"] == 1 and p["splits"] >= 3, p
    last = K - (p["splits"] - 1) * p["k_per_split"]
    assert 0 < last < p["k_per_split"], (K, p)


@pytest.mark.parametrize("cus", [1, 8, 256, 304])
@pytest.mark.parametrize("pn", list(PASSES))
def test_declined_geometries(pn, cus):
    dims, taps = regular_geometry(CASES["C1"])
    ok = plan(PASSES[pn], torch.float32, dims, taps, cus=cus)
    assert ok["accepted"] == 1 and ok["reason"] == ""
    f64 = plan(PASSES[pn], torch.float64, dims, taps, cus=cus)
    assert f64["accepted"] == 0 and "dtype" in f64["reason"], f64
    dims4, taps4 = regular_geometry(CASES["C4"])
    grouped = plan(PASSES[pn], torch.float32, dims4, taps4, groups=2, cus=cus)
    assert grouped["accepted"] == 0 and "groups" in grouped["reason"], grouped
    # an operand of 2^31 elements: x = [2^15, 2^6, 1, 2^10]
    big = plan(PASSES[pn], torch.bfloat16, [2 ** 15, 2 ** 6, 1, 2 ** 10, 8, 1, 2 ** 10], [1, 3, 1, 1, 0, 1, 1, 1], cus=cus)
    assert big["index_bits"] == 32 and big["accepted"] == 0 and "2^31" in big["reason"], big
    # ... and one element fewer than that is taken
    edge = plan(PASSES[pn], torch.bfloat16, [2 ** 15 - 1, 2 ** 6, 1, 2 ** 10, 8, 1, 2 ** 10], [1, 3, 1, 1, 0, 1, 1, 1], cus=cus)
    assert edge["accepted"] == 1, edge


def test_header_declares_the_modules_and_the_switch():
    src = open(os.path.join(ROOT, "include", "lamp_host.h")).read()
    for name in ("lamp_module_conv1d", "lamp_module_conv2d_transposed", "lamp_module_weight_norm_linear", "lamp_convolution_matrix_path"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in lib.decls
    assert "lamp_debug_conv_gen_plan" not in src          # exported, but a test tool: not part of the public headers
    hip = open(os.path.join(ROOT, "include", "lamp_hip.h")).read()
    assert "conv1d" not in hip and "conv2d_transposed" not in hip and "weight_norm_linear" not in hip
