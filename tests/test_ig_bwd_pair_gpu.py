"""lamp_convolution_backward_pair on a wide block's short-K entry pair (res3 of Cnn.resnet: a 3x3 16 -> 128 and its sibling 1x1 16 -> 128 on 8x8
maps, stride 1): the paired input gradient and both weight gradients from ONE launch of the eight-image implicit-GEMM form (ig_bwd_pair_kernel,
timer class conv_bwd_igemm), which accumulates each weight gradient while that source's eight images are resident in LDS.

The reference everywhere is the two calls it replaces, in the same process: lamp_convolution_backward_input_pair (dx, bitwise) and
lamp_convolution_backward_weight_pair (the four-wave kernel: the same image ranges per partial sum, so only the order of f32 sums inside a partial
may differ - the bound of test_conv_bwd_pair_gpu.py for another order of the f32 sums, 2^-7), and ATen in f64 on the same bf16 values (2e-2).
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from lamp_amd._capi import lib
from tests.test_conv_bwd_pair_gpu import _Case, _conv_launches, _num_cus
from tests.util import assert_close

pytestmark = pytest.mark.gpu
aten = torch.ops.aten

# (cin, ca, cb): res3's entry, and the narrower pairs that leave waves (64: four, 32: six) and x channels (8 of 16) without work
GEOMS = {"res3": (16, 128, 128), "64+64": (16, 64, 64), "8->32": (8, 32, 32)}
_REFS = {}


def _n0():
    """the eight-image form's smallest batch (ig_form): four images per CU"""
    return 4 * _num_cus()


def _reference(geom, ragged, with_add):
    """the two pair calls and the f64 weight gradients, computed once per case, shared by the tests below and left unchanged"""
    key = (geom, ragged, with_add)
    if key not in _REFS:
        cin, ca, cb = GEOMS[geom]
        cs = _Case(_n0() + (3 if ragged else 0), cin, 8, ca, cb, stride=1)
        ref, launches, rows = _conv_launches(lambda: [cs.input_pair(with_add)] + cs.weight_pair())
        okey = (geom, ragged, "oracle")
        if okey not in _REFS:
            x, ga, gb = cs.x.double(), cs.ga.double(), cs.gb.double()
            wa = aten.convolution_backward(ga, x, cs.wa.double(), [0], [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1]
            wb = aten.convolution_backward(gb, x, cs.wb.double(), [0], [1, 1], [0, 0], [1, 1], False, [0, 0], 1, [False, True, False])[1]
            _REFS[okey] = (wa, wb)
        _REFS[key] = (cs, ref, launches, rows, _REFS[okey])
    return _REFS[key]


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_entry_pair_backward_is_the_pair_calls_in_one_launch(gpu, geom, ragged, with_add):
    """N = 4 x CUs and that + 3 (a last workgroup of three images): dx bitwise the input-gradient pair's; dw, dw1 within 2^-7 of the weight-gradient
    pair's (the same partition, another order inside a partial at most) and within 2e-2 of ATen in f64; one conv_* launch, of class conv_bwd_igemm."""
    cs, ref, ref_launches, ref_rows, oracle = _reference(geom, ragged, with_add)
    got, launches, rows = _conv_launches(lambda: cs.merged(with_add))
    assert torch.equal(got[0], ref[0]), f"dx: max diff {(got[0].float() - ref[0].float()).abs().max().item()}"
    for g, r, o, name in zip(got[1:], ref[1:], oracle, ("dw (3x3)", "dw1 (1x1)")):
        assert g.shape == r.shape
        diff = (g.double() - r.double()).abs()
        print(f"{geom} N={cs.N} addend={with_add} {name}: max |diff| to the separate launch {diff.max().item():.3e} (changed {diff.gt(0).float().mean().item():.3f}), "
              f"max |diff| to f64 {(g.double() - o).abs().max().item():.3e} of max {o.abs().max().item():.3e}")
        assert_close(g, r.double(), 2.0 ** -7, f"{name} against the separate launch")
        assert_close(g, o, 2e-2, f"{name} against ATen in f64")
    assert rows.get("conv_bwd_igemm", 0) == 1 and launches == 1, rows
    assert ref_launches == 2 and "conv_bwd_igemm" not in ref_rows, ref_rows


def _fallback_case(what):
    n0 = _n0()
    return {"100 channels": lambda: _Case(n0, 16, 8, 100, 100, stride=1),
            "N = 64": lambda: _Case(64, 16, 8, 128, 128, stride=1),
            "f32": lambda: _Case(n0, 16, 8, 32, 32, stride=1, dt=torch.float32),
            "32 input channels": lambda: _Case(n0, 32, 8, 128, 128, stride=1),
            "unequal Cout": lambda: _Case(n0, 16, 8, 128, 64, stride=1)}[what]()


@pytest.mark.parametrize("what", ["100 channels", "N = 64", "f32", "32 input channels", "unequal Cout"])
def test_entry_pair_backward_runs_the_pair_calls_where_the_kernel_does_not_take_the_geometry(gpu, what):
    """The K-tail geometry (100 + 100), a batch below the eight-image form's, f32, more than 16 input channels and unequal output channels: the three
    results and the launches are those of the two pair calls."""
    cs = _fallback_case(what)
    for with_add in (False, True):
        want, sep_launches, sep_rows = _conv_launches(lambda: [cs.input_pair(with_add)] + cs.weight_pair())
        got, launches, rows = _conv_launches(lambda: cs.merged(with_add))
        for g, w, name in zip(got, want, ("dx", "dw", "dw1")):
            assert g.shape == w.shape and torch.equal(g, w), f"{name} (addend: {with_add}): the merged call differs from the pair calls"
        conv = lambda rs: {k: v for k, v in rs.items() if k.startswith("conv_")}
        assert "conv_bwd_igemm" not in rows and conv(rows) == conv(sep_rows) and launches == sep_launches >= 2, (rows, sep_rows)


_PAIR = r"""
import torch
from lamp_amd._capi import lib
from tests.test_conv_bwd_pair_gpu import _Case, _conv_launches, _num_cus
cs = _Case(4 * _num_cus(), 16, 8, 128, 128, stride=1)
for with_add in (False, True):
    want, sep_launches, sep_rows = _conv_launches(lambda: [cs.input_pair(with_add)] + cs.weight_pair())
    got, launches, rows = _conv_launches(lambda: cs.merged(with_add))
    print("EQUAL", *[int(torch.equal(g, w)) for g, w in zip(got, want)])
    conv = lambda rs: {k: v for k, v in rs.items() if k.startswith("conv_")}
    print("SAME_LAUNCHES", int(conv(rows) == conv(sep_rows) and launches == sep_launches), rows.get("conv_bwd_igemm", 0))
"""


def _child(script, env_extra, *args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, **env_extra)
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", script, *args], cwd=root, env=env, capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return [ln.split() for ln in out.stdout.splitlines() if ln.strip()]


def test_entry_pair_backward_runs_the_pair_calls_with_the_switch_off(gpu):
    """LAMP_IG_BWD_PAIR=0 (a fresh process: the switch is read once): res3's pair at N = 4 x CUs gives the pair calls' bits and launches."""
    rows = _child(_PAIR, {"LAMP_IG_BWD_PAIR": "0"})
    assert [r for r in rows if r[0] == "EQUAL"] == [["EQUAL", "1", "1", "1"]] * 2, rows
    assert [r for r in rows if r[0] == "SAME_LAUNCHES"] == [["SAME_LAUNCHES", "1", "0"]] * 2, rows


_STEP = r"""
import ctypes as C, hashlib, os, sys
import numpy as np
import torch
from lamp_amd import nn, sten as S
from lamp_amd._capi import lib
from oracle import lamp_oracle as O
from tests.util import to_sten
outdir = sys.argv[1]
ncu = C.c_int(0); lib.lamp_device_num_cus(C.byref(ncu))
B = 4 * ncu.value
ob = O.resnet(100, torch.bfloat16)
init = [to_sten(v.value) for v in ob.state()]
x = to_sten(O.closed_form(B * 3 * 32 * 32, 5, 1.0, torch.bfloat16).reshape(B, 3, 32, 32))
t = to_sten((torch.arange(B) * 7) % 100)
def fresh():
    hm = nn.resnet(100, 0.0, S.BF16)
    hm.load(init)
    return hm, nn.SupervisedModel(hm, nn.SupervisedModel.NLL, S.STen.ones([100], S.BF16))
def digest(ts):
    h = hashlib.sha256()
    for v in ts: h.update(v.to_numpy().tobytes())
    return h.hexdigest()
hm, model = fresh()
acc = S.STen.zeros([1], S.F64)
lib.lamp_kernel_timer_enable(1)
n, grads = model.addTotalLossAndReturnGradientsAndNumExamples(x, t, acc)
buf = C.create_string_buffer(1 << 16)
lib.lamp_kernel_timer_report(buf, len(buf))
lib.lamp_kernel_timer_enable(0)
rows = {l.split()[0]: int(l.split()[1]) for l in buf.value.decode().splitlines() if l.strip()}
grads = list(grads)
print("LOSS", digest([acc]))
for i, g in enumerate(grads):
    shape = tuple(g.shape)
    entry = shape in ((128, 16, 3, 3), (128, 16, 1, 1))
    if entry: np.save(os.path.join(outdir, "g%d.npy" % i), np.asarray(g.to_numpy(), dtype=np.float32))
    print("GRAD", i, "entry" if entry else "other", digest([g]))
print("LAUNCHES", rows.get("conv_bwd_igemm", 0))
# the same step captured into a HIP graph (after one eager step on the capture stream, as bench.py does) and replayed twice
hm2, model2 = fresh()
acc2 = S.STen.zeros([1], S.F64)
lib.lamp_device_synchronize()
st = C.c_void_p(); lib.lamp_stream_get_from_pool(0, 0, C.byref(st)); lib.lamp_stream_set_current(st)
model2.addTotalLossAndReturnGradientsAndNumExamples(x, t, acc2)
lib.lamp_device_synchronize()
lib.lamp_graph_begin_capture()
n2, g2 = model2.addTotalLossAndReturnGradientsAndNumExamples(x, t, acc2)
graph = C.c_void_p(); lib.lamp_graph_end_capture(C.byref(graph))
for k in range(2):
    lib.lamp_graph_launch(graph)
    lib.lamp_device_synchronize()
    print("REPLAY", digest(list(g2)))
print("EAGER", digest(grads))
"""


def test_training_step_with_the_merged_entry_backward_is_the_step_without_it(gpu):
    """nn.resnet(100), one bf16 training step at B = 4 x CUs with LAMP_IG_BWD_PAIR 0 and 1 (a fresh process each): the loss and every gradient but the
    two entry filters' (128 x 16 x 3 x 3, 128 x 16 x 1 x 1) are identical, those two within 2^-7 of the step without (their f64 bound is the operator
    tests' above: the step's intermediates are not at hand here); the step captured into a HIP graph and replayed twice writes the eager step's
    gradients; the eager step's report shows one conv_bwd_igemm launch (none with the switch off)."""
    seen = {}
    with tempfile.TemporaryDirectory() as tmp:
        for flag in ("0", "1"):
            d = os.path.join(tmp, flag)
            os.mkdir(d)
            rows = _child(_STEP, {"LAMP_IG_BWD_PAIR": flag}, d)
            replays = [r[1] for r in rows if r[0] == "REPLAY"]
            eager = [r[1] for r in rows if r[0] == "EAGER"]
            assert len(replays) == 2 and len(eager) == 1 and replays[0] == replays[1] == eager[0], f"LAMP_IG_BWD_PAIR={flag}: the replayed graph's gradients differ from the eager step's"
            seen[flag] = {"loss": [r[1] for r in rows if r[0] == "LOSS"], "grads": {int(r[1]): (r[2], r[3]) for r in rows if r[0] == "GRAD"},
                          "launches": [int(r[1]) for r in rows if r[0] == "LAUNCHES"],
                          "entry": {int(r[1]): torch.from_numpy(np.load(os.path.join(d, f"g{r[1]}.npy"))) for r in rows if r[0] == "GRAD" and r[2] == "entry"}}
    off, on = seen["0"], seen["1"]
    assert off["loss"] == on["loss"] and len(on["loss"]) == 1, "the loss differs"
    assert len(on["grads"]) == len(off["grads"]) == 37 and len(on["entry"]) == len(off["entry"]) == 2, (len(on["grads"]), len(on["entry"]))
    for i, (kind, dig) in on["grads"].items():
        assert off["grads"][i][0] == kind
        if kind == "other":
            assert off["grads"][i][1] == dig, f"gradient {i} differs"
        else:
            diff = (on["entry"][i].double() - off["entry"][i].double()).abs()
            print(f"entry filter gradient {i} {tuple(on['entry'][i].shape)}: max |diff| {diff.max().item():.3e}, changed {diff.gt(0).float().mean().item():.3f}")
            assert_close(on["entry"][i], off["entry"][i].double(), 2.0 ** -7, f"entry filter gradient {i} against the step without the merged launch")
    assert off["launches"] == [0] and on["launches"] == [1], (off["launches"], on["launches"])
