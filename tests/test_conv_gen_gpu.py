"""The general matrix-core convolution (kernels/conv_gen.hip) behind 1-D and transposed convolutions: forward, input gradient and weight
gradient in f32 and bf16 against ATen on the CPU in f64 ON THE SAME (f32- / bf16-representable) OPERANDS, at the tolerances of
test_convolution_forward_backward (f32: 1e-5 forward, 1e-4 backward; bf16: 2^-7 both; assert_close's default scale).  ATen's own f32
accumulation stays within 1.2e-6 / 7.7e-6 of f64 on these shapes and f32 accumulation with one bf16 rounding within 3.0e-3, so the
tolerances leave room for any summation order.  The kernel classes that ran are read from the kernel timer.
"""
import ctypes as C

import pytest
import torch

from lamp_amd import nn
from lamp_amd import sten as S
from lamp_amd._capi import lib, i64_array
from tests.conv_gen_cases import CASES
from tests.util import assert_close, closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu
aten = torch.ops.aten

FWD_TOL = {torch.float64: 1e-12, torch.float32: 1e-5, torch.bfloat16: 2.0 ** -7}
BWD_TOL = {torch.float64: 1e-10, torch.float32: 1e-4, torch.bfloat16: 2.0 ** -7}
DTS = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]
GEN = ("conv_gen_fwd", "conv_gen_dgrad", "conv_gen_wgrad")
DIRECT = ("conv_fwd_direct", "conv_dgrad_direct", "conv_wgrad_direct", "conv_wgrad_lds")


class _Problem:
    """operands (closed-form values, rounded to dt) and the f64 reference of one case; built once per (case, dtype, groups)"""

    def __init__(self, case, dt, groups=1):
        transposed, N, cx, spatial, cy, k, s, p, d, op = case
        n = len(spatial)
        self.dt, self.n, self.transposed, self.groups = dt, n, transposed, groups
        self.x = closed_form((N, cx) + tuple(spatial), 3, 2.0, dt)
        wshape = ((cx, cy // groups) if transposed else (cy, cx // groups)) + (k,) * n
        self.w = closed_form(wshape, 17, 1.0, dt)
        self.b = closed_form((cy,), 5, 1.0, dt)
        self.args = ([s] * n, [p] * n, [d] * n, transposed, [op] * n, groups)
        self.ref = aten.convolution(self.x.double(), self.w.double(), self.b.double(), *self.args)
        self.gy = closed_form(tuple(self.ref.shape), 23, 1.0, dt)
        self.refb = aten.convolution_backward(self.gy.double(), self.x.double(), self.w.double(), [cy], *self.args, [True, True, True])
        self.cargs = (i64_array([s] * n), i64_array([p] * n), i64_array([d] * n))
        self.op = i64_array([op] * n)

    def forward(self):
        o = C.c_void_p()
        lib.lamp_convolution(C.byref(o), to_sten(self.x), to_sten(self.w), to_sten(self.b), *self.cargs, self.n, int(self.transposed), self.op, self.groups)
        return to_torch(S.STen(o))

    def backward(self):
        out = (C.c_void_p * 3)()
        lib.lamp_convolution_backward(out, to_sten(self.gy), to_sten(self.x), to_sten(self.w), *self.cargs, self.n, int(self.transposed), self.op, self.groups,
                                      (C.c_uint8 * 3)(1, 1, 1))
        return [to_torch(S.STen(out[i])) for i in range(3)]

    def check(self, y, grads, what):
        assert_close(y, self.ref, FWD_TOL[self.dt], what + " forward")
        for got, ref, name in zip(grads, self.refb, ("input gradient", "weight gradient", "bias gradient")):
            assert_close(got, ref, BWD_TOL[self.dt], what + " " + name)


_problems = {}


def problem(cid, dt, groups=1):
    key = (cid, dt, groups)
    if key not in _problems:
        _problems[key] = _Problem(CASES[cid], dt, groups)
    return _problems[key]


def timed(fn):
    """fn() under the kernel timer: (its result, {tag: launches})"""
    lib.lamp_kernel_timer_filter(None)
    buf = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_report(buf, len(buf))          # drop what earlier tests left in the log
    lib.lamp_kernel_timer_enable(1)
    try:
        r = fn()
    finally:
        lib.lamp_kernel_timer_report(buf, len(buf))
        lib.lamp_kernel_timer_enable(0)
    return r, {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines() if ln.strip()}


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cid", list(CASES))
def test_values(gpu, cid, dt):
    pr = problem(cid, dt)
    (y, grads), ran = timed(lambda: (pr.forward(), pr.backward()))
    print(cid, dt, ran)
    assert [ran.get(t, 0) for t in GEN] == [1, 1, 1], f"each pass of the general kernel once (transposed: dgrad forward, fwd for dx): {ran}"
    assert not any(ran.get(t, 0) for t in DIRECT), f"a direct kernel ran: {ran}"
    pr.check(y, grads, cid)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cid", ["C5", "T5"])
def test_backward_is_deterministic(gpu, cid, dt):
    pr = problem(cid, dt)
    first, second = pr.backward(), pr.backward()
    for a, b, name in zip(first, second, ("dx", "dw", "db")):
        assert torch.equal(a, b), f"{cid} {name} differs between two runs"


@pytest.mark.parametrize("cid", ["T2", "C1"])
def test_switch(gpu, cid):
    pr = problem(cid, torch.float32)
    prev = nn.convolutionMatrixPath(False)
    try:
        assert prev is True, "the matrix path is on by default"
        (y0, g0), ran0 = timed(lambda: (pr.forward(), pr.backward()))
        assert nn.convolutionMatrixPath(True) is False
        (y1, g1), ran1 = timed(lambda: (pr.forward(), pr.backward()))
    finally:
        nn.convolutionMatrixPath(prev)
    assert not any(ran0.get(t, 0) for t in GEN), f"switched off, the general kernel still ran: {ran0}"
    assert sum(ran0.get(t, 0) for t in DIRECT) == 3, f"switched off, the three direct kernels run: {ran0}"
    assert [ran1.get(t, 0) for t in GEN] == [1, 1, 1] and not any(ran1.get(t, 0) for t in DIRECT), ran1
    pr.check(y0, g0, cid + " direct")
    pr.check(y1, g1, cid + " matrix")


@pytest.mark.parametrize("cid,dt,groups", [("C1", torch.float64, 1), ("C4", torch.float32, 2)], ids=["C1-f64", "C4-groups2"])
def test_declined_geometries_keep_the_direct_kernels(gpu, cid, dt, groups):
    pr = problem(cid, dt, groups)
    (y, grads), ran = timed(lambda: (pr.forward(), pr.backward()))
    assert not any(t.startswith("conv_gen") for t in ran), f"the general kernel took a geometry it declines: {ran}"
    pr.check(y, grads, cid)


def test_backward_input_add(gpu):
    pr = problem("C1", torch.float32)
    add = closed_form(tuple(pr.x.shape), 29, 1.0, pr.dt)

    def run():
        o = C.c_void_p()
        lib.lamp_convolution_backward_input_add(C.byref(o), to_sten(pr.gy), to_sten(pr.x), to_sten(pr.w), *pr.cargs, pr.n, pr.op, 1, to_sten(add))
        return to_torch(S.STen(o))

    got, ran = timed(run)
    assert ran.get("conv_gen_dgrad", 0) == 1 and not any(ran.get(t, 0) for t in DIRECT), ran
    assert_close(got, pr.refb[0] + add.double(), 1e-4, "input gradient + addend")
