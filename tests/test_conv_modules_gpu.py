"""Conv1D, Conv2DTransposed and WeightNormLinear (lamp-core nn/Conv1D.scala, nn/Conv2DTransposed.scala, nn/WeightNormLinear.scala) through
the module machinery: values and parameter gradients against torch autograd in f64 on the same (f32- / bf16-representable) operands,
checkpoints, one AdamW step and a captured forward + backward.

Tolerances: f32 1e-5 on outputs and 1e-4 on gradients (the single-operator bars); bf16 2^-6 with assert_close's scale="max", because the
networks are chains of two bf16 stages - the case that scale is documented for.
"""
import ctypes as C
import os
import tempfile

import pytest
import torch
import torch.nn.functional as TF

from lamp_amd import autograd as A
from lamp_amd import nn
from lamp_amd import sten as S
from lamp_amd._capi import lib
from tests.util import TORCH2LAMP, assert_close, closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu
F64 = torch.float64
DTS = [torch.float32, torch.bfloat16]
DT_IDS = ["f32", "bf16"]


def tolerances(dt):
    return (1e-5, 1e-4, "mean") if dt == torch.float32 else (2.0 ** -6, 2.0 ** -6, "max")


# ---- the two networks: (library module, state tensors, input, f64 restatement) --------------------------------------------------------
def conv1d_stack(dt):
    ldt = TORCH2LAMP[dt]
    m = nn.Sequential(nn.Conv1D(20, 40, 3, ldt, padding=1), nn.Fun("relu"), nn.Conv1D(40, 24, 5, ldt, stride=2, padding=2, bias=False))
    state = [closed_form((40, 20, 3), 17, 1.0, dt), closed_form((40,), 5, 1.0, dt), closed_form((24, 40, 5), 29, 0.5, dt), closed_form((24,), 7, 1.0, dt)]
    x = closed_form((3, 20, 50), 3, 2.0, dt)

    def ref(s, xr):
        return TF.conv1d(TF.relu(TF.conv1d(xr, s[0], s[1], padding=1)), s[2], s[3], stride=2, padding=2)

    return m, state, x, ref


def transposed_autoencoder(dt):
    ldt = TORCH2LAMP[dt]
    m = nn.Sequential(nn.Conv2D(3, 24, 3, ldt, stride=2, padding=1), nn.Fun("relu"), nn.Conv2DTransposed(24, 3, 4, ldt, stride=2, padding=1))
    state = [closed_form((24, 3, 3, 3), 17, 1.0, dt), closed_form((24,), 5, 1.0, dt), closed_form((24, 3, 4, 4), 29, 0.5, dt), closed_form((3,), 7, 1.0, dt)]
    x = closed_form((2, 3, 16, 16), 3, 2.0, dt)

    def ref(s, xr):
        return TF.conv_transpose2d(TF.relu(TF.conv2d(xr, s[0], s[1], stride=2, padding=1)), s[2], s[3], stride=2, padding=1)

    return m, state, x, ref


def sum_of_squares(m, x):
    y = m.forward(A.const(x))
    return y, (y * y).sum()


def check_network(build, dt, out_shape, needs_grad):
    m, state, x, ref = build(dt)
    assert [tuple(v.value.shape) for v in m.state] == [tuple(t.shape) for t in state]
    assert [bool(v.needsGrad) for v in m.state] == needs_grad
    m.load([to_sten(t) for t in state])
    y, loss = sum_of_squares(m, to_sten(x))
    grads = m.gradients(loss)
    rs = [t.double().requires_grad_(g) for t, g in zip(state, needs_grad)]
    yr = ref(rs, x.double())
    gr = torch.autograd.grad((yr * yr).sum(), [r for r, g in zip(rs, needs_grad) if g])
    ftol, btol, scale = tolerances(dt)
    assert list(y.value.shape) == out_shape
    assert_close(to_torch(y.value), yr.detach(), ftol, "output", scale=scale)
    assert len(grads) == len(gr)
    for k, (got, want) in enumerate(zip(grads, gr)):
        assert_close(to_torch(got), want, btol, f"gradient of parameter {k}", scale=scale)


def test_weight_norm_linear_known_answer(gpu):
    """nn.test.scala:406-415: V = G = ones [1, 3], bias ones, x = [[1, 3, 5], [2, 4, 6]] in f64: the output sums to 23"""
    m = nn.WeightNormLinear(3, 1, S.F64)
    assert [tuple(v.value.shape) for v in m.state] == [(1, 3), (1, 3), (1, 1)] and all(v.needsGrad for v in m.state)
    state = [torch.ones(1, 3, dtype=F64), torch.ones(1, 3, dtype=F64), torch.ones(1, 1, dtype=F64)]
    m.load([to_sten(t) for t in state])
    x = torch.tensor([[1.0, 3.0, 5.0], [2.0, 4.0, 6.0]], dtype=F64)
    total = m.forward(A.const(to_sten(x))).sum()
    assert abs(to_torch(total.value).item() - 23.0) <= 1e-12
    grads = m.gradients(total)
    v, g, b = (t.clone().requires_grad_(True) for t in state)
    w = g * v / v.norm(dim=0, keepdim=True)
    want = torch.autograd.grad((x.mm(w.t()) + b).sum(), [v, g, b])
    for got, ref, name in zip(grads, want, ("V", "G", "bias")):
        assert (to_torch(got) - ref).abs().max().item() <= 1e-10, name
    assert len(nn.WeightNormLinear(3, 2, S.F32, bias=False).state) == 2


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_conv1d_stack(gpu, dt):
    check_network(conv1d_stack, dt, [3, 24, 25], [True, True, True, False])


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_conv2d_transposed_autoencoder(gpu, dt):
    check_network(transposed_autoencoder, dt, [2, 3, 16, 16], [True, False, True, False])


def test_checkpoint_round_trip(gpu):
    m, state, x, _ = conv1d_stack(torch.float32)
    m.load([to_sten(t) for t in state])
    lib.lamp_manual_seed(5)
    wn = nn.WeightNormLinear(7, 5, S.F32)
    xw = closed_form((4, 7), 3, 2.0, torch.float32)
    with tempfile.TemporaryDirectory() as d:
        for mod, inp, fresh in ((m, x, conv1d_stack(torch.float32)[0]), (wn, xw, nn.WeightNormLinear(7, 5, S.F32))):
            path = os.path.join(d, "ckpt")
            lib.lamp_module_write_checkpoint(mod.h, path.encode())
            lib.lamp_module_load_from_file(fresh.h, path.encode())
            for a, b in zip(fresh.state, mod.state):
                assert torch.equal(to_torch(a.value), to_torch(b.value))
            assert torch.equal(to_torch(fresh.forward(A.const(to_sten(inp))).value), to_torch(mod.forward(A.const(to_sten(inp))).value))


def test_adamw_step(gpu):
    m, state, x, _ = conv1d_stack(torch.float32)
    m.load([to_sten(t) for t in state])
    X = to_sten(x)
    params = m.parameters
    assert len(params) == 3
    opt = nn.AdamW([p.value for p in params], weightDecay=0.0, learningRate=1e-3)
    _, loss = sum_of_squares(m, X)
    before = to_torch(loss.value).item()
    grads = m.gradients(loss)
    tp = [to_torch(p.value).double().clone().requires_grad_(True) for p in params]
    for p, g in zip(tp, grads):
        p.grad = to_torch(g).double()
    opt.step(grads, 1.0)
    torch.optim.AdamW(tp, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0).step()
    for k, (p, want) in enumerate(zip(params, tp)):
        assert_close(to_torch(p.value), want.detach(), 1e-5, f"parameter {k} after one AdamW step")
    after = to_torch(sum_of_squares(m, X)[1].value).item()
    assert after < before, (before, after)


def test_graph_capture(gpu):
    """forward + backward of the Conv1D stack (mean-squared-error against zeros: the sum of squares up to a factor) captured on one stream
    and replayed twice: the gradients equal the eager step's bit for bit"""
    m, state, x, _ = conv1d_stack(torch.float32)
    st = C.c_void_p(); lib.lamp_stream_get_from_pool(0, 0, C.byref(st)); lib.lamp_stream_set_current(st)
    try:
        m.load([to_sten(t) for t in state])
        model = nn.SupervisedModel(m, nn.SupervisedModel.MSE)
        x_buf, target = to_sten(x), S.STen.zeros([3, 24, 25], S.F32)
        _, eager = model.addTotalLossAndReturnGradientsAndNumExamples(x_buf, target, S.STen.zeros([1], S.F32))
        eager = [to_torch(g).clone() for g in eager]
        assert all(bool(g.abs().max() > 0) for g in eager)
        acc = S.STen.zeros([1], S.F32)
        lib.lamp_device_synchronize()
        lib.lamp_graph_begin_capture()
        _, grads = model.addTotalLossAndReturnGradientsAndNumExamples(x_buf, target, acc)
        g = C.c_void_p(); lib.lamp_graph_end_capture(C.byref(g))
        for replay in range(2):
            for t in grads:
                t.copyFrom(S.STen.zeros(t.shape, S.F32))       # the replay has to produce them again
            lib.lamp_graph_launch(g)
            lib.lamp_device_synchronize()
            for k, (got, want) in enumerate(zip(grads, eager)):
                assert torch.equal(to_torch(got), want), f"replay {replay}: gradient {k} differs from the eager step"
        lib.lamp_graph_release(g)
    finally:
        d = C.c_void_p(); lib.lamp_stream_get_default(0, C.byref(d)); lib.lamp_stream_set_current(d)
        lib.lamp_stream_release(st); lib.lamp_stream_release(d)
