"""lamp_convolution_chain_pair: a convolution and the 3x3 + 1x1 pair behind it (the stem of Cnn.resnet and the two branches of its first
residual block, cnn.scala:95-109) from one call - one launch of the narrow kernel where it keeps the stem's output in LDS for the pair.

The reference everywhere is the two calls it replaces, lamp_convolution followed by lamp_convolution_pair, in the same process: the fused
launch runs the same MFMA chains over the same rounded values, so every comparison is bitwise (torch.equal).  The oracle comparison (ATen
f32 on the same bf16 values) uses the tolerance of the existing pair test.
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

ONE, Z = i64_array([1, 1]), i64_array([0, 0])


def _conv_launches(fn):
    """runs fn() under the kernel timer: (its result, launches of the conv_* classes, the whole report)"""
    lib.lamp_kernel_timer_enable(1)
    r = fn()
    buf = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_report(buf, len(buf))
    lib.lamp_kernel_timer_enable(0)
    rows = {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines() if ln.strip()}       # "tag count total_ms flops bytes"
    return r, sum(n for t, n in rows.items() if t.startswith("conv_")), rows


class _Case:
    """x -> conv(k0 x k0, stride s0, pad k0 // 2) -> (3x3 stride s pad 1, 1x1 stride s pad 0); closed-form values, optionally three biases"""

    def __init__(self, N, cin, c0, cout, H=32, k0=5, s0=1, stride=2, biases=False, dt=torch.bfloat16):
        self.dt, self.stride, self.s0, self.k0 = dt, stride, s0, k0
        self.x = closed_form((N, cin, H, H), 3, 2.0, dt)
        self.w0 = closed_form((c0, cin, k0, k0), 7, 0.2, dt)
        self.wa = closed_form((cout, c0, 3, 3), 17, 0.2, dt)
        self.wb = closed_form((cout, c0, 1, 1), 23, 0.4, dt)
        self.b0 = closed_form((c0,), 11, 1.0, dt) if biases else None
        self.ba = closed_form((cout,), 5, 1.0, dt) if biases else None
        self.bb = closed_form((cout,), 13, 1.0, dt) if biases else None
        self.X, self.W0, self.WA, self.WB = to_sten(self.x), to_sten(self.w0), to_sten(self.wa), to_sten(self.wb)
        self.B0, self.BA, self.BB = (to_sten(b) if b is not None else None for b in (self.b0, self.ba, self.bb))
        self.sd0, self.p0_ = i64_array([s0, s0]), i64_array([k0 // 2, k0 // 2])
        self.sd, self.p1, self.p0 = i64_array([stride, stride]), i64_array([1, 1]), i64_array([0, 0])

    def chain(self):
        o3 = (C.c_void_p * 3)()
        lib.lamp_convolution_chain_pair(o3, self.X, self.W0, self.B0, self.sd0, self.p0_, ONE, self.WA, self.BA, self.sd, self.p1, ONE,
                                        self.WB, self.BB, self.sd, self.p0, ONE, 2, 1)
        return [S.STen(o3[i]) for i in range(3)]

    def separate(self):
        o = C.c_void_p()
        lib.lamp_convolution(C.byref(o), self.X, self.W0, self.B0, self.sd0, self.p0_, ONE, 2, 0, Z, 1)
        s = S.STen(o)
        o2 = (C.c_void_p * 2)()
        lib.lamp_convolution_pair(o2, s, self.WA, self.BA, self.sd, self.p1, ONE, self.WB, self.BB, self.sd, self.p0, ONE, 2, 1)
        return [s, S.STen(o2[0]), S.STen(o2[1])]

    def assert_equal(self, what=""):
        got, want = self.chain(), self.separate()
        for g, w, name in zip(got, want, ("s", "a (3x3)", "b (1x1)")):
            assert torch.equal(to_torch(g), to_torch(w)), f"{what}{name}: the chain call differs from the two calls"
        return got, want


def _bn(t, cout, dt):
    """batch norm + relu of t under the kernel timer (the bn() of test_convolution_pair_is_the_two_convolutions_in_one_launch)"""
    g, b = closed_form((cout,), 1, 1.0, dt) + 1.0, closed_form((cout,), 9, 1.0, dt)
    out = (C.c_void_p * 3)()
    RM, RV = to_sten(torch.zeros(cout, dtype=dt)), to_sten(torch.ones(cout, dtype=dt))
    lib.lamp_kernel_timer_enable(1)
    lib.lamp_native_batch_norm_relu(out, t, to_sten(g), to_sten(b), RM, RV, 1, 0.1, 1e-5)
    rep = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_report(rep, len(rep))
    lib.lamp_kernel_timer_enable(0)
    return [to_torch(S.STen(out[i])) for i in range(3) if out[i]] + [to_torch(RM), to_torch(RV)], rep.value


# N = 2051: the smallest batch at which every persistent workgroup of a <= 1024-workgroup grid walks two or three images with a ragged remainder
@pytest.mark.parametrize("N", [1, 5, 2051])
@pytest.mark.parametrize("c0,cout,biases", [(6, 6, False), (6, 6, True), (8, 8, False)])
def test_chain_pair_is_the_two_calls_in_one_launch(gpu, N, c0, cout, biases):
    """The ResNet's own entry (3 -> 6 5x5 pad 2 on 32 x 32, then 6 -> 6 3x3 stride 2 + 1x1 stride 2), the same with all three biases, and
    3 -> 8 with an 8 -> 8 pair (all 16 MFMA columns in use): s, a and b are BITWISE those of lamp_convolution + lamp_convolution_pair, from ONE
    launch; a batch norm reading a or b launches no statistics pass (N >= 2) and returns the bits it returns for the two calls' outputs."""
    cs = _Case(N, 3, c0, cout, biases=biases)
    want = cs.separate()
    got, launches, rows = _conv_launches(cs.chain)
    for g, w, name in zip(got, want, ("s", "a (3x3)", "b (1x1)")):
        assert torch.equal(to_torch(g), to_torch(w)), f"{name}: the chain call differs from the two calls"
    assert launches == 1, rows
    for g, w, name in zip(got[1:], want[1:], ("a", "b")):
        (r1, rep1), (r2, rep2) = _bn(g, cout, cs.dt), _bn(w, cout, cs.dt)
        assert (b"bn_fwd_stats" in rep1) == (b"bn_fwd_stats" in rep2), f"{name}: the chain's output carries a different hand-off"
        if N >= 2:
            assert b"bn_fwd_stats" not in rep1, f"{name}: no statistics were handed over"
        for u, v in zip(r1, r2):
            assert torch.equal(u, v), f"{name}: batch norm of the chain's output differs from batch norm of the pair's"
    if N == 5:
        # the oracle: ATen f32 on the same bf16 values (a and b from the ROUNDED s, as both forms compute them)
        f = lambda t: None if t is None else t.float()
        rs = aten.convolution(cs.x.float(), cs.w0.float(), f(cs.b0), [1, 1], [2, 2], [1, 1], False, [0, 0], 1)
        assert_close(to_torch(got[0]), rs.double(), FWD_TOL[cs.dt] * 4, "s against the oracle")
        sb = to_torch(got[0]).float()
        ra = aten.convolution(sb, cs.wa.float(), f(cs.ba), [2, 2], [1, 1], [1, 1], False, [0, 0], 1)
        rb = aten.convolution(sb, cs.wb.float(), f(cs.bb), [2, 2], [0, 0], [1, 1], False, [0, 0], 1)
        assert_close(to_torch(got[1]), ra.double(), FWD_TOL[cs.dt] * 4, "3x3 against the oracle")
        assert_close(to_torch(got[2]), rb.double(), FWD_TOL[cs.dt] * 4, "1x1 against the oracle")


@pytest.mark.parametrize("what", ["24x24", "stride-2 first", "f32"])
def test_chain_pair_runs_the_two_calls_where_the_kernel_does_not_take_the_geometry(gpu, what):
    """A 24 x 24 image (three column groups per row: not an aligned-window form), a stride-2 first convolution and f32 tensors: the entry point
    runs lamp_convolution + lamp_convolution_pair itself - their values, and exactly their launches (2 where the pair itself is one launch:
    the stride-2 case; the 24 x 24 and f32 pairs are two launches of their own, unchanged here)."""
    cs = {"24x24": lambda: _Case(5, 3, 6, 6, H=24),
          "stride-2 first": lambda: _Case(5, 3, 6, 6, s0=2),
          "f32": lambda: _Case(5, 3, 6, 6, dt=torch.float32)}[what]()
    want, sep_launches, _ = _conv_launches(cs.separate)
    got, launches, rows = _conv_launches(cs.chain)
    for g, w, name in zip(got, want, ("s", "a (3x3)", "b (1x1)")):
        assert torch.equal(to_torch(g), to_torch(w)), f"{name}: the chain call differs from the two calls"
    assert launches == sep_launches and launches >= 2, (launches, sep_launches, rows)
    if what == "stride-2 first":
        assert launches == 2, rows
    # ... against one launch where it fuses (same channels on the ResNet's 32 x 32 map)
    _, fused_launches, rows = _conv_launches(_Case(5, 3, 6, 6).chain)
    assert fused_launches == 1, rows


def test_chain_launch_sees_every_write_to_each_of_the_three_filters(gpu):
    """The chain launch reads two cached fragment images (the stem's, and the pair's with both filters in it): whichever of the three filters
    is written - in place, or by the optimiser, which re-packs cached images itself - the next chain call equals the two calls on the
    current weights, bit for bit (the pattern of test_pair_launch_sees_every_write_to_either_filter)."""
    from lamp_amd import nn as NN
    cs = _Case(16, 3, 6, 6, biases=True)
    cs.assert_equal("first call: "); cs.assert_equal("cached call: ")
    lib.lamp_mul_scalar_(cs.W0, 0.5); cs.assert_equal("after the stem filter was scaled in place: ")
    lib.lamp_mul_scalar_(cs.WA, -1.5); cs.assert_equal("after the 3x3 was scaled in place: ")
    lib.lamp_mul_scalar_(cs.WB, 0.75); cs.assert_equal("after the 1x1 was scaled in place: ")
    g0, ga, gb = S.STen.ones([6, 3, 5, 5], S.BF16, 0), S.STen.ones([6, 6, 3, 3], S.BF16, 0), S.STen.ones([6, 6, 1, 1], S.BF16, 0)
    NN.SGDW([cs.W0], 0.25, 0.0).step([g0], 1.0); cs.assert_equal("after the optimiser stepped the stem alone: ")
    NN.SGDW([cs.WA], 0.25, 0.0).step([ga], 1.0); cs.assert_equal("after the optimiser stepped the 3x3 alone: ")
    NN.SGDW([cs.WB], 0.25, 0.0).step([gb], 1.0); cs.assert_equal("after the optimiser stepped the 1x1 alone: ")
    every = NN.SGDW([cs.W0, cs.WA, cs.WB], 0.125, 0.0)
    every.step([g0, ga, gb], 1.0); cs.assert_equal("after the optimiser stepped all three: ")
    every.step([g0, ga, gb], 1.0); got, _ = cs.assert_equal("after a second step of all three (images re-packed in place): ")
    # ... and the values follow the weights (oracle on the CURRENT values)
    rs = aten.convolution(cs.x.float(), to_torch(cs.W0).float(), cs.b0.float(), [1, 1], [2, 2], [1, 1], False, [0, 0], 1)
    assert_close(to_torch(got[0]), rs.double(), FWD_TOL[cs.dt] * 4, "s against the oracle on the current weights")


_STEP = r"""
import ctypes as C, hashlib, sys
import torch
from lamp_amd import nn, sten as S
from lamp_amd._capi import lib
from oracle import lamp_oracle as O
from tests.util import to_sten
B = 67
torch.manual_seed(1234)
ob = O.resnet(100, torch.bfloat16)
x = to_sten(O.closed_form(B * 3 * 32 * 32, 5, 1.0, torch.bfloat16).reshape(B, 3, 32, 32))
t = to_sten((torch.arange(B) * 7) % 100)
def fresh():
    hm = nn.resnet(100, 0.0, S.BF16)
    hm.load([to_sten(v.value) for v in ob.state()])
    return hm, nn.SupervisedModel(hm, nn.SupervisedModel.NLL, S.STen.ones([100], S.BF16))
def digest(ts):
    h = hashlib.sha256()
    for v in ts: h.update(v.to_numpy().tobytes())
    return h.hexdigest()
# eager step under the kernel timer, then AdamW
hm, model = fresh()
acc = S.STen.zeros([1], S.F64)
lib.lamp_kernel_timer_enable(1)
n, grads = model.addTotalLossAndReturnGradientsAndNumExamples(x, t, acc)
buf = C.create_string_buffer(1 << 16)
lib.lamp_kernel_timer_report(buf, len(buf))
lib.lamp_kernel_timer_enable(0)
rows = {l.split()[0]: int(l.split()[1]) for l in buf.value.decode().splitlines() if l.strip()}
assert len(grads) == 37
print("GRADS", digest([acc] + list(grads)))
nn.AdamW([p.value for p in hm.parameters], 0.0, 1e-3, 0.9, 0.95).step(list(grads), 1.0)
print("STATE", digest([s.value for s in hm.state]))
print("LAUNCHES", rows.get("conv_fwd_narrow", 0), rows.get("conv_dgrad_narrow", 0), rows.get("conv_wgrad_narrow", 0))
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
print("EAGER", digest(list(grads)))
"""


def test_resnet_step_with_the_chain_is_bitwise_the_step_without_it(gpu):
    """nn.resnet(100), one bf16 training step at B = 67 with LAMP_CONV_CHAIN on and off (two processes: the switch is read once): loss, all
    37 gradients and the state after the AdamW step are identical; the step captured into a HIP graph and replayed twice writes the eager
    step's gradients; and the eager step's kernel-timer report shows one narrow forward launch fewer with the switch on (the narrow
    input- and weight-gradient launches are the same: backward is not touched)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seen = {}
    for flag in ("0", "1"):
        env = dict(os.environ, LAMP_CONV_CHAIN=flag, PYTHONPATH=root)
        out = subprocess.run([sys.executable, "-c", _STEP], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        rows = [ln.split() for ln in out.stdout.splitlines()]
        seen[flag] = {r[0]: r[1:] for r in rows if r and r[0] in ("GRADS", "STATE", "LAUNCHES", "EAGER")}
        replays = [r[1] for r in rows if r and r[0] == "REPLAY"]
        assert len(replays) == 2 and replays[0] == replays[1] == seen[flag]["EAGER"][0], f"LAMP_CONV_CHAIN={flag}: the replayed graph's gradients differ from the eager step's"
    assert seen["0"]["GRADS"] == seen["1"]["GRADS"], "loss or gradients differ"
    assert seen["0"]["STATE"] == seen["1"]["STATE"], "the state after the AdamW step differs"
    off, on = [int(v) for v in seen["0"]["LAUNCHES"]], [int(v) for v in seen["1"]["LAUNCHES"]]
    assert on[0] == off[0] - 1, (off, on)
    assert on[1:] == off[1:] and min(on) >= 1, (off, on)
