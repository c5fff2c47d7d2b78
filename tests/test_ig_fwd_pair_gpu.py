"""lamp_convolution_pair on a wide block's short-K entry pair (res3 of Cnn.resnet: a 3x3 16 -> 128 and its sibling 1x1 16 -> 128 on 8x8 maps,
stride 1): ig_fwd_pair_k16_kernel runs the arithmetic of the eight-image kernel's sibling form (ig_conv8d_kernel<3, NCT, 1>) on another schedule -
both filters resident in LDS, every wave over its own sixteen channel tiles without a workgroup barrier - so NOTHING may change a bit.

The reference is the launch it replaces: the same calls in a fresh process with LAMP_IG_FWD_PAIR=0 (the switch is read once per process), compared
by SHA-256 of every result's bytes; and ATen in f32 on the same bf16 values, within the bound of the pair test in test_ops_gpu.py (FWD_TOL * 4).
One child per switch value runs every operator case; one more per switch value runs the training step.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from lamp_amd import sten as S
from lamp_amd._capi import lib, i64_array
from tests.util import FWD_TOL, assert_close, closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu
aten = torch.ops.aten

# name -> (LAMP_IG_VARIANT or "", N as ("n0", extra) or a number, cin, cout, dtype name)
# the geometries the new kernel takes: one workgroup, two, and N = 4 x CUs with 128 / 64 output channels and 16 / 8 input channels
TAKEN = {"d N=8": ("d", 8, 16, 128, "bfloat16"), "d N=16": ("d", 16, 16, 128, "bfloat16"), "16->128": ("", ("n0", 0), 16, 128, "bfloat16"),
         "16->64": ("", ("n0", 0), 16, 64, "bfloat16"), "8->128": ("", ("n0", 0), 8, 128, "bfloat16")}
# ... and those it declines: a ragged last workgroup, two k-steps, output channels that are neither 64 nor 128, f32, a batch below the eight-image form's
DECLINED = {"ragged": ("", ("n0", 3), 16, 128, "bfloat16"), "32 input channels": ("", ("n0", 0), 32, 128, "bfloat16"),
            "100 channels": ("", ("n0", 0), 16, 100, "bfloat16"), "f32": ("", ("n0", 0), 16, 128, "float32"),
            "N = 64": ("", 64, 16, 128, "bfloat16")}

_OPS = r"""
import ctypes as C, hashlib, os, sys
import torch
from lamp_amd import sten as S
from lamp_amd._capi import lib, i64_array
from tests.util import closed_form, to_sten
from tests.test_ig_fwd_pair_gpu import TAKEN, DECLINED
ncu = C.c_int(0); lib.lamp_device_num_cus(C.byref(ncu))
def digest(ts):
    h = hashlib.sha256()
    for v in ts: h.update(v.to_numpy().tobytes())
    return h.hexdigest()
def report():
    buf = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_report(buf, len(buf))
    lib.lamp_kernel_timer_enable(0)
    return {l.split()[0]: int(l.split()[1]) for l in buf.value.decode().splitlines() if l.strip()}
one, p1, p0 = i64_array([1, 1]), i64_array([1, 1]), i64_array([0, 0])
for name, (variant, N, cin, cout, dtn) in list(TAKEN.items()) + list(DECLINED.items()):
    dt = getattr(torch, dtn)
    if not isinstance(N, int): N = 4 * ncu.value + N[1]
    if variant: os.environ["LAMP_IG_VARIANT"] = variant
    else: os.environ.pop("LAMP_IG_VARIANT", None)
    X = to_sten(closed_form((N, cin, 8, 8), 3, 2.0, dt))
    WA, BA = to_sten(closed_form((cout, cin, 3, 3), 17, 0.2, dt)), to_sten(closed_form((cout,), 5, 1.0, dt))
    WB, BB = to_sten(closed_form((cout, cin, 1, 1), 23, 0.4, dt)), to_sten(closed_form((cout,), 13, 1.0, dt))
    G, B = to_sten(closed_form((cout,), 1, 1.0, dt) + 1.0), to_sten(closed_form((cout,), 9, 1.0, dt))
    for with_bias in (1, 0):
        o2 = (C.c_void_p * 2)()
        lib.lamp_kernel_timer_enable(1)
        lib.lamp_convolution_pair(o2, X, WA, BA if with_bias else None, one, p1, one, WB, BB if with_bias else None, one, p0, one, 2, 1)
        rows = report()
        outs = [S.STen(o2[0]), S.STen(o2[1])]
        conv = sum(n for t, n in rows.items() if t.startswith("conv_"))
        bns, stats_passes = [], 0
        for y in outs:
            out = (C.c_void_p * 3)()
            RM, RV = to_sten(torch.zeros(cout, dtype=dt)), to_sten(torch.ones(cout, dtype=dt))
            lib.lamp_kernel_timer_enable(1)
            lib.lamp_native_batch_norm_relu(out, y, G, B, RM, RV, 1, 0.1, 1e-5)
            stats_passes += report().get("bn_fwd_stats", 0)
            bns.append(digest([S.STen(out[i]) for i in range(3)] + [RM, RV]))
        print("CASE", name.replace(" ", "_"), with_bias, digest(outs[:1]), digest(outs[1:]), bns[0], bns[1], conv, stats_passes)
"""

_STEP = r"""
import ctypes as C, hashlib, sys
import torch
from lamp_amd import nn, sten as S
from lamp_amd._capi import lib
from oracle import lamp_oracle as O
from tests.util import to_sten
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
n, grads = model.addTotalLossAndReturnGradientsAndNumExamples(x, t, acc)
grads = list(grads)
print("LOSS", digest([acc]))
for i, g in enumerate(grads): print("GRAD", i, digest([g]))
for i, v in enumerate(hm.state): print("STATE", i, digest([v.value]))
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

_RUNS = {}


def _child(script, flag):
    """the script's output rows in a fresh process with LAMP_IG_FWD_PAIR=flag, run once per (script, flag) and shared by the tests below"""
    key = (script, flag)
    if key not in _RUNS:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, PYTHONPATH=root, LAMP_IG_FWD_PAIR=flag)
        env.pop("LAMP_IG_VARIANT", None)
        out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", script], cwd=root, env=env, capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
        _RUNS[key] = [ln.split() for ln in out.stdout.splitlines() if ln.strip()]
    return _RUNS[key]


def _case_rows(flag, name, with_bias):
    rows = [r for r in _child(_OPS, flag) if r[0] == "CASE" and r[1] == name.replace(" ", "_") and r[2] == str(with_bias)]
    assert len(rows) == 1, rows
    return rows[0][3:]


@pytest.mark.parametrize("with_bias", [1, 0])
@pytest.mark.parametrize("name", list(TAKEN))
def test_entry_pair_forward_is_bitwise_the_launch_it_replaces(gpu, name, with_bias):
    """Both outputs, and the five results of lamp_native_batch_norm_relu on each (no bn_fwd_stats launch: the statistics were handed over), carry
    the bytes of the LAMP_IG_FWD_PAIR=0 run; one conv_* launch either way."""
    off, on = _case_rows("0", name, with_bias), _case_rows("1", name, with_bias)
    for k, what in enumerate(("3x3 output", "1x1 output", "batch norm of the 3x3 output", "batch norm of the 1x1 output")):
        assert on[k] == off[k], f"{name}, bias {with_bias}: {what} differs from the eight-image kernel's"
    assert on[4] == off[4] == "1", (on[4], off[4])
    assert on[5] == off[5] == "0", f"{name}: a statistics pass ran ({on[5]} with the kernel, {off[5]} without)"


@pytest.mark.parametrize("with_bias", [1, 0])
@pytest.mark.parametrize("name", list(DECLINED))
def test_entry_pair_forward_declines_what_it_does_not_take(gpu, name, with_bias):
    """A ragged batch, 32 input channels, 100 output channels, f32 and a small batch: the old launch's bits and launch counts."""
    off, on = _case_rows("0", name, with_bias), _case_rows("1", name, with_bias)
    assert on == off, (name, with_bias, on, off)


@pytest.mark.parametrize("variant,N", [("d", 8), ("", None)])
def test_entry_pair_forward_against_the_oracle(gpu, monkeypatch, variant, N):
    """N = 8 (one workgroup, LAMP_IG_VARIANT=d) and N = 4 x CUs, 16 -> 128 with bias: both outputs within FWD_TOL[bf16] * 4 of ATen in f32 on the
    same bf16 values - the bound of test_convolution_pair_is_the_two_convolutions_in_one_launch."""
    dt = torch.bfloat16
    if variant:
        monkeypatch.setenv("LAMP_IG_VARIANT", variant)
    else:
        monkeypatch.delenv("LAMP_IG_VARIANT", raising=False)
    if N is None:
        ncu = C.c_int(0)
        lib.lamp_device_num_cus(C.byref(ncu))
        N = 4 * ncu.value
    cin, cout = 16, 128
    x = closed_form((N, cin, 8, 8), 3, 2.0, dt)
    wa, ba = closed_form((cout, cin, 3, 3), 17, 0.2, dt), closed_form((cout,), 5, 1.0, dt)
    wb, bb = closed_form((cout, cin, 1, 1), 23, 0.4, dt), closed_form((cout,), 13, 1.0, dt)
    one, p1, p0 = i64_array([1, 1]), i64_array([1, 1]), i64_array([0, 0])
    o2 = (C.c_void_p * 2)()
    lib.lamp_convolution_pair(o2, to_sten(x), to_sten(wa), to_sten(ba), one, p1, one, to_sten(wb), to_sten(bb), one, p0, one, 2, 1)
    pa, pb = S.STen(o2[0]), S.STen(o2[1])
    ra = aten.convolution(x.float(), wa.float(), ba.float(), [1, 1], [1, 1], [1, 1], False, [0, 0], 1)
    rb = aten.convolution(x.float(), wb.float(), bb.float(), [1, 1], [0, 0], [1, 1], False, [0, 0], 1)
    assert_close(to_torch(pa), ra.double(), FWD_TOL[dt] * 4, "3x3 against the oracle")
    assert_close(to_torch(pb), rb.double(), FWD_TOL[dt] * 4, "1x1 against the oracle")


def test_training_step_with_the_entry_pair_kernel_is_the_step_without_it(gpu):
    """nn.resnet(100), one bf16 training step at B = 4 x CUs with LAMP_IG_FWD_PAIR 0 and 1 (a fresh process each): the loss, every gradient and
    every state tensor carry the same bytes; the step captured into a HIP graph and replayed twice writes the eager step's gradients."""
    seen = {}
    for flag in ("0", "1"):
        rows = _child(_STEP, flag)
        replays = [r[1] for r in rows if r[0] == "REPLAY"]
        eager = [r[1] for r in rows if r[0] == "EAGER"]
        assert len(replays) == 2 and len(eager) == 1 and replays[0] == replays[1] == eager[0], f"LAMP_IG_FWD_PAIR={flag}: the replayed graph's gradients differ from the eager step's"
        seen[flag] = {kind: [r[1:] for r in rows if r[0] == kind] for kind in ("LOSS", "GRAD", "STATE")}
    off, on = seen["0"], seen["1"]
    assert len(on["LOSS"]) == 1 and len(on["GRAD"]) == 37 and len(on["STATE"]) >= 37, (len(on["LOSS"]), len(on["GRAD"]), len(on["STATE"]))
    for kind in ("LOSS", "GRAD", "STATE"):
        assert len(on[kind]) == len(off[kind])
        for a, b in zip(on[kind], off[kind]):
            assert a == b, f"{kind} {a[0] if len(a) > 1 else ''} differs between LAMP_IG_FWD_PAIR=0 and 1"
