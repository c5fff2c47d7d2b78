"""lamp_convolution_backward_pair: the paired input gradient and both weight gradients of the 3x3 + 1x1 pair a residual block applies to its
input (cnn.scala:16-20), from one call - one launch of the narrow kernel (ncv_bwd_pair_kernel) on the stride-2 bf16 blocks, which stages x and
the two output gradients once for all three results.

The reference everywhere is the calls it replaces, in the same process: lamp_convolution_backward_input_pair for dx (with and without addend),
lamp_convolution_backward_weight_pair for the weight gradients where the two gradients share the 16 MFMA rows (res1), two
lamp_convolution_backward calls with the weight mask where they do not (res2).  dx is bitwise.  dw is bitwise where the merged launch walks the
images in the partition (workgroups, images per workgroup) of the launch it replaces.  The weight-gradient reduction declares no work with the
kernel timer, so the partition cannot be read back from a report; `_partition` below mirrors the launch plan's arithmetic instead (LDS bytes
per workgroup -> workgroups per CU -> images per workgroup) and says where the two coincide - at every case of this file but one (res2's 1x1
at N = 2051), by design of the kernel (it shortens its rounds until two workgroups share a CU, see narrow_conv_backward_pair).  Where they
differ, the bound is the one of
test_two_layers_weight_gradients_share_one_launch (another partition of the f32 sums: 2^-7, fewer than a quarter of the elements changed) and
the f64 ATen tolerance of test_weight_gradients_of_a_block_s_two_first_convolutions.

res2 (6 -> 16 + 6 -> 16): the merged launch includes the 1x1's weight gradient (its 16 rows are a second A fragment) - one launch for three.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from lamp_amd import sten as S
from lamp_amd._capi import lib, i64_array
from tests.util import assert_close, closed_form, to_sten, to_torch

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


def _num_cus():
    n = C.c_int(0)
    lib.lamp_device_num_cus(C.byref(n))
    return n.value


def _round_up(v, m):
    return (v + m - 1) // m * m


def _partition(N, cin, H, ca, cb):
    """((workgroups, images per workgroup) of the merged launch, ... of the launch that computes the 3x3's weight gradient in the reference, ... the
    1x1's, rounds of the merged kernel) for the stride-2 3x3 + 1x1 pair on an H x H map, from the LDS arithmetic of the launch plans in
    conv_narrow.hip (150 KiB per CU, at most 4 workgroups; the merged kernel's registers allow two workgroups per CU, the reference's four).
    ca + cb <= 16: the reference is the pair launch for both; else the 1x1 has a launch of its own, with a smaller staged image."""
    ho = H // 2
    howo, cpi = ho * ho, ho * ho // 32
    hs = max(H + 2, (ho - 1) * 2 + 3)
    ximg = cin * hs * _round_up(8 + max(H // 2, ho) + 8, 8) * 2                  # elements: two column-parity planes
    ig_ref = max(1, 256 // howo)
    red = 4 * 16 * (2 * 3 * 16) * 4
    w2 = ca + cb > 16
    lds_ref = ig_ref * (ximg + 16 * howo) * 2 + red                              # (w2: the 3x3 alone; else the pair launch - the same bytes)
    # the dilated image of the input gradient: [ca + cb][hs_d][ws_d], pitch widened to a bank-conflict-free one (ncv_plan)
    hs_d = max(1 + (ho - 1) * 2 + 1, H + 2)
    ws_d = _round_up(max(8 + (ho - 1) * 2 + 1, H - 1 + 7 + 8), 8)
    ws_d = _round_up(max(ws_d, H + 16), 8)
    ncg = H // 8
    for k in range(16):
        step = (2 * (ws_d // 8 + k)) & 15
        if step % ncg == 0 and (step // ncg) & 1 == 1 and (ca + cb) * hs_d * (ws_d + 8 * k) * 2 <= 64 * 1024:
            ws_d += 8 * k
            break
    dil = (ca + cb) * hs_d * ws_d * 2
    tail = max(dil, red + (4 * 16 * 32 * 4 if w2 else 0))
    lds_of = lambda ig: ig * (ximg + (32 if w2 else 16) * howo) * 2 + tail
    ig = ig_ref
    while lds_of(ig) * 2 > 150 * 1024 and ig % 2 == 0 and ((ig // 2) * cpi) % 4 == 0:
        ig //= 2
    per_cu_ref = max(1, min(4, 150 * 1024 // lds_ref))
    lds_ref_b = ig_ref * (cin * max(H, (ho - 1) * 2 + 1) * _round_up(8 + max(H // 2, ho) + 8, 8) * 2 + 16 * howo) * 2 + 4 * 16 * 16 * 4 if w2 else lds_ref
    per_cu_ref_b = max(1, min(4, 150 * 1024 // lds_ref_b))
    per_cu = min(per_cu_ref, max(1, min(2, 150 * 1024 // lds_of(ig))))

    def part(pc):
        rounds = (N + ig_ref - 1) // ig_ref
        nb = min(rounds, _num_cus() * pc)
        ipb = (rounds + nb - 1) // nb * ig_ref
        return (N + ipb - 1) // ipb, ipb
    return part(per_cu), part(per_cu_ref), part(per_cu_ref_b), ig


class _Case:
    """x [N, cin, H, H] -> (3x3 stride s pad 1 to ca channels, 1x1 stride s pad 0 to cb channels); closed-form values"""

    def __init__(self, N, cin, H, ca, cb, stride=2, dt=torch.bfloat16):
        self.N, self.cin, self.H, self.ca, self.cb, self.stride, self.dt = N, cin, H, ca, cb, stride, dt
        ho = (H - 1) // stride + 1
        self.x = closed_form((N, cin, H, H), 3, 2.0, dt)
        self.wa, self.wb = closed_form((ca, cin, 3, 3), 17, 0.5, dt), closed_form((cb, cin, 1, 1), 19, 0.7, dt)
        self.ga, self.gb = closed_form((N, ca, ho, ho), 23, 1.0, dt), closed_form((N, cb, ho, ho), 31, 1.0, dt)
        self.add = closed_form((N, cin, H, H), 41, 3.0, dt)
        self.X, self.WA, self.WB, self.GA, self.GB, self.A = (to_sten(t) for t in (self.x, self.wa, self.wb, self.ga, self.gb, self.add))
        self.sd, self.p1, self.p0 = i64_array([stride, stride]), i64_array([1, 1]), i64_array([0, 0])

    def merged(self, with_add):
        o3 = (C.c_void_p * 3)()
        lib.lamp_convolution_backward_pair(o3, self.X, self.GA, self.WA, self.sd, self.p1, ONE, self.GB, self.WB, self.sd, self.p0, ONE, 2, 1,
                                           self.A if with_add else None)
        return [to_torch(S.STen(o3[i])) for i in range(3)]            # (reading the weight gradients runs their deferred reductions)

    def input_pair(self, with_add):
        o = C.c_void_p()
        lib.lamp_convolution_backward_input_pair(C.byref(o), self.X, self.GA, self.WA, self.sd, self.p1, ONE, self.GB, self.WB, self.sd, self.p0, ONE, 2, 1,
                                                 self.A if with_add else None)
        return to_torch(S.STen(o))

    def weight_pair(self):
        o2 = (C.c_void_p * 2)()
        lib.lamp_convolution_backward_weight_pair(o2, self.X, self.GA, self.WA, self.sd, self.p1, ONE, self.GB, self.WB, self.sd, self.p0, ONE, 2, 1)
        return [to_torch(S.STen(o2[0])), to_torch(S.STen(o2[1]))]

    def weight_singles(self):
        out = []
        for G, W, pad in ((self.GA, self.WA, self.p1), (self.GB, self.WB, self.p0)):
            o3 = (C.c_void_p * 3)()
            lib.lamp_convolution_backward(o3, G, self.X, W, self.sd, pad, ONE, 2, 0, Z, 1, (C.c_uint8 * 3)(0, 1, 0))
            out.append(to_torch(S.STen(o3[1])))
        return out

    def reference(self, with_add):
        """the calls the merged one replaces: res2's 32 rows of output gradient do not share a weight-gradient launch"""
        dx = self.input_pair(with_add)
        return [dx] + (self.weight_singles() if self.ca + self.cb > 16 else self.weight_pair())

    def oracle(self, with_add):
        """ATen in f64 on the same bf16 values"""
        s = [self.stride, self.stride]
        x, wa, wb, ga, gb = (t.double() for t in (self.x, self.wa, self.wb, self.ga, self.gb))
        ra = aten.convolution_backward(ga, x, wa, [0], s, [1, 1], [1, 1], False, [0, 0], 1, [True, True, False])
        rb = aten.convolution_backward(gb, x, wb, [0], s, [0, 0], [1, 1], False, [0, 0], 1, [True, True, False])
        dx = ra[0] + rb[0]
        return [dx + self.add.double() if with_add else dx, ra[1], rb[1]]


# (cin, H, ca, cb, reference launches): res1 and res2 of Cnn.resnet, and a pair that fills all 16 MFMA rows of the weight gradient's tile
GEOMS = {"res1": (6, 32, 6, 6, 2), "res2": (6, 16, 16, 16, 3), "8+8": (8, 16, 8, 8, 2)}
# N = 1 and 5, and the smallest batch at which a workgroup of the launch plan (one image per round on the 16x16 output map of res1, four on the 8x8
# maps; at most 2 x 256 workgroups) walks more than one round with a ragged last one
BATCHES = {"res1": [1, 5, 1027], "res2": [1, 5, 2051], "8+8": [1, 5, 2051]}
_REFS = {}


def _reference(geom, N, with_add):
    """computed once per (geometry, batch, addend), shared by the tests below and left unchanged"""
    key = (geom, N, with_add)
    if key not in _REFS:
        cin, H, ca, cb, _ = GEOMS[geom]
        cs = _Case(N, cin, H, ca, cb)
        ref, launches, rows = _conv_launches(lambda: cs.reference(with_add))
        _REFS[key] = (cs, ref, launches, rows)
    return _REFS[key]


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("geom,N", [(g, n) for g in GEOMS for n in BATCHES[g]])
def test_backward_pair_is_the_pair_calls_in_one_launch(gpu, geom, N, with_add):
    """dx bitwise lamp_convolution_backward_input_pair's; dw_a, dw_b bitwise the weight-gradient launches' where the partition is theirs
    (every case here but res2's 1x1 at N = 2051, whose own launch stages a smaller image, fits three workgroups per CU and so gives each of
    its 513 workgroups one round where the merged launch's 257 take two: another partition, the stated bound); ONE conv_* launch where the reference has 2 (res1, 8+8) or 3 (res2: the 1x1's weight gradient rides along)."""
    cs, ref, ref_launches, ref_rows = _reference(geom, N, with_add)
    got, launches, rows = _conv_launches(lambda: cs.merged(with_add))
    assert torch.equal(got[0], ref[0]), f"dx: max diff {(got[0].float() - ref[0].float()).abs().max().item()}"
    mine, theirs_a, theirs_b, ig = _partition(N, *GEOMS[geom][:4])
    print(f"{geom} N={N}: partition merged {mine} reference {theirs_a} / {theirs_b} (rounds of {ig}); launches {rows} vs {ref_rows}")
    for g, r, name, theirs in zip(got[1:], ref[1:], ("dw_a (3x3)", "dw_b (1x1)"), (theirs_a, theirs_b)):
        assert g.shape == r.shape
        diff = (g.double() - r.double()).abs()
        print(f"  {name}: max |diff| {diff.max().item():.3e}, changed {diff.gt(0).float().mean().item():.3f}")
        if mine == theirs:
            assert torch.equal(g, r), f"{name}: same partition {mine}, max diff {diff.max().item()}"
        else:
            assert_close(g, r.double(), 2.0 ** -7, f"{name} against the separate launch (partition {mine} vs {theirs})")
            assert diff.gt(0).float().mean().item() < 0.25, f"{name}: more than a quarter of the elements changed their rounding"
    if mine != theirs_a or mine != theirs_b or N == 5:
        want = cs.oracle(with_add)
        assert_close(got[1], want[1], 2e-2, "3x3 weight gradient against the oracle")
        assert_close(got[2], want[2], 2e-2, "1x1 weight gradient against the oracle")
        if N == 5:
            assert_close(got[0], want[0], 3e-2, "dx against the oracle")
    assert rows.get("conv_bwd_narrow", 0) == 1 and launches == 1, rows
    assert ref_launches == GEOMS[geom][4], ref_rows


@pytest.mark.parametrize("what", ["stride 1", "f32", "20 channels"])
def test_backward_pair_runs_the_pair_calls_where_the_kernel_does_not_take_the_geometry(gpu, what):
    """Stride 1, f32 tensors and 20 + 20 output channels: the entry point runs lamp_convolution_backward_input_pair and
    lamp_convolution_backward_weight_pair itself - the three results are theirs bit for bit, and so are the launches."""
    cs = {"stride 1": lambda: _Case(5, 6, 16, 6, 6, stride=1),
          "f32": lambda: _Case(5, 6, 32, 6, 6, dt=torch.float32),
          "20 channels": lambda: _Case(5, 6, 16, 20, 20)}[what]()
    for with_add in (False, True):
        want, sep_launches, sep_rows = _conv_launches(lambda: [cs.input_pair(with_add)] + cs.weight_pair())
        got, launches, rows = _conv_launches(lambda: cs.merged(with_add))
        for g, w, name in zip(got, want, ("dx", "dw_a", "dw_b")):
            assert g.shape == w.shape and torch.equal(g, w), f"{name} (addend: {with_add}): the merged call differs from the pair calls"
        assert "conv_bwd_narrow" not in rows and launches == sep_launches >= 2, (rows, sep_rows)
        ref = cs.oracle(with_add)
        tol = 1e-4 if cs.dt == torch.float32 else 3e-2
        for g, r, name in zip(got, ref, ("dx", "dw_a", "dw_b")):
            assert_close(g, r, tol, f"{name} against the oracle")


_STEP = r"""
import ctypes as C, hashlib, sys
import torch
from lamp_amd import nn, sten as S
from lamp_amd._capi import lib
from oracle import lamp_oracle as O
from tests.util import to_sten, closed_form
kind = sys.argv[1]
B = 64
if kind == "resnet":
    ob = O.resnet(100, torch.bfloat16)
    init = [to_sten(v.value) for v in ob.state()]
    x = to_sten(O.closed_form(B * 3 * 32 * 32, 5, 1.0, torch.bfloat16).reshape(B, 3, 32, 32))
    classes = 100
    def build():
        hm = nn.resnet(100, 0.0, S.BF16)
        hm.load(init)
        return hm
else:
    # one residual block of the res2 form behind a convolution and a batch norm (its input needs a gradient), pooled to 16 classes
    x = to_sten(closed_form((B, 3, 16, 16), 5, 1.0, torch.bfloat16))
    classes = 16
    def build():
        right = nn.Sequential(nn.Conv2D(6, 16, 3, S.BF16, stride=2, padding=1), nn.BatchNorm2D(16, S.BF16), nn.Fun("relu"),
                              nn.Conv2D(16, 16, 3, S.BF16, padding=1), nn.BatchNorm2D(16, S.BF16))
        left = nn.Sequential(nn.Conv2D(6, 16, 1, S.BF16, stride=2), nn.BatchNorm2D(16, S.BF16))
        hm = nn.Sequential(nn.Conv2D(3, 6, 3, S.BF16, padding=1), nn.BatchNorm2D(6, S.BF16), nn.Residual(right, left), nn.Fun("relu"),
                           nn.Fun("avgpool2d", 8, 1), nn.Fun("flatten_last", 3), nn.Fun("logsoftmax", 1))
        st = hm.state
        hm.load([to_sten(closed_form(tuple(v.value.shape), 7 + 3 * i, 1.0, torch.bfloat16) + (1.0 if len(v.value.shape) == 1 else 0.0)) for i, v in enumerate(st)])
        return hm
t = to_sten((torch.arange(B) * 7) % classes)
def fresh():
    hm = build()
    return hm, nn.SupervisedModel(hm, nn.SupervisedModel.NLL, S.STen.ones([classes], S.BF16))
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
print("NGRADS", len(grads))
print("GRADS", digest([acc] + list(grads)))
nn.AdamW([p.value for p in hm.parameters], 0.0, 1e-3, 0.9, 0.95).step(list(grads), 1.0)
print("STATE", digest([s.value for s in hm.state]))
print("LAUNCHES", rows.get("conv_bwd_narrow", 0), rows.get("conv_dgrad_narrow", 0), rows.get("conv_wgrad_narrow", 0))
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


@pytest.mark.parametrize("kind,merged,fewer", [("block", 1, (1, 2)), ("resnet", 2, (2, 3))])
def test_training_step_with_the_merged_backward_is_bitwise_the_step_without_it(gpu, kind, merged, fewer):
    """A residual block of the res2 form behind a convolution, and nn.resnet(100): one bf16 training step at B = 64 with LAMP_CONV_BWD_PAIR on
    and off (a fresh process each: the switch is read once): loss, every gradient and the state after the AdamW step are identical; the step
    captured into a HIP graph and replayed twice writes the eager step's gradients; and the eager step's report shows the merged launches
    (res1's and res2's in the network) in place of the paired input-gradient launch and the one or two weight-gradient launches of each."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seen = {}
    for flag in ("0", "1"):
        env = dict(os.environ, LAMP_CONV_BWD_PAIR=flag, PYTHONPATH=root)
        out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", _STEP, kind], cwd=root, env=env, capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
        rows = [ln.split() for ln in out.stdout.splitlines()]
        seen[flag] = {r[0]: r[1:] for r in rows if r and r[0] in ("NGRADS", "GRADS", "STATE", "LAUNCHES", "EAGER")}
        replays = [r[1] for r in rows if r and r[0] == "REPLAY"]
        assert len(replays) == 2 and replays[0] == replays[1] == seen[flag]["EAGER"][0], f"LAMP_CONV_BWD_PAIR={flag}: the replayed graph's gradients differ from the eager step's"
    assert seen["0"]["NGRADS"] == seen["1"]["NGRADS"] and int(seen["1"]["NGRADS"][0]) == (37 if kind == "resnet" else 12)
    assert seen["0"]["GRADS"] == seen["1"]["GRADS"], "loss or gradients differ"
    assert seen["0"]["STATE"] == seen["1"]["STATE"], "the state after the AdamW step differs"
    off, on = [int(v) for v in seen["0"]["LAUNCHES"]], [int(v) for v in seen["1"]["LAUNCHES"]]
    assert off[0] == 0 and on[0] == merged, (off, on)
    assert on[1] == off[1] - fewer[0] and on[2] == off[2] - fewer[1], (off, on)
