"""RAdam, Yogi and the learning-rate schedules without a GPU: the restatement of tests/optim_ref.py reproduces the reference's own
known answers (adamw.test.scala:43-67,128-155), RAdam's branch switches where its formula says, Yogi's sign is that of the ROUNDED
square, the schedules give the reference's values (reducelronplateau.test.scala), and the public names exist."""
import numpy as np
import pytest
import torch

from tests import optim_ref as R

K = R.KATS


def test_restated_radam_reproduces_the_reference_kat():
    k = K["radam"]
    p = torch.tensor([k["init"]], dtype=torch.float64)
    g = torch.tensor([k["gradients"]], dtype=torch.float64)
    opt = R.RAdam([p], k["weightDecay"], k["learningRate"], k["beta1"], k["beta2"])
    opt.step([g], 1.0)
    assert p[0].tolist() == k["step1"]
    opt.step([g], 1.0)
    assert p[0].tolist() == k["step2"]
    assert g[0].tolist() == k["gradients"], "RAdam only reads its gradients"


def test_restated_yogi_reproduces_the_reference_kat_by_mutating_the_gradient():
    k = K["yogi"]
    p = torch.tensor([k["init"]], dtype=torch.float64)
    g = torch.tensor([k["gradients"]], dtype=torch.float64)
    opt = R.Yogi([p], k["weightDecay"], k["learningRate"], k["beta1"], k["beta2"])
    opt.step([g], 1.0)
    assert np.array_equal(np.round(p[0].numpy(), 4), np.round(k["step1"], 4))
    assert g[0].tolist() == k["gradients_after_step1"]
    opt.step([g], 1.0)                                   # the same tensor, now -g^2, as the reference's test does
    assert np.array_equal(np.round(p[0].numpy(), 4), np.round(k["step2"], 4))
    # a second step on the ORIGINAL gradient gives other values: the write-back is part of the known answer
    p2 = torch.tensor([k["init"]], dtype=torch.float64)
    o2 = R.Yogi([p2], k["weightDecay"], k["learningRate"], k["beta1"], k["beta2"])
    for _ in range(2):
        o2.step([torch.tensor([k["gradients"]], dtype=torch.float64)], 1.0)
    assert not np.array_equal(np.round(p2[0].numpy(), 4), np.round(k["step2"], 4))


@pytest.mark.parametrize("b2", [0.999, 0.9])
def test_radam_is_unrectified_for_four_steps(b2):
    assert [R.radam_is_rectified(b2, t) for t in range(1, 9)] == [False] * 4 + [True] * 4


def test_radam_is_never_rectified_at_beta2_one_half():
    assert R.radam_rho(0.5, 1)[1] <= 4                   # rhoInf = 3: (rhoInf - 4) must not be used
    assert not any(R.radam_is_rectified(0.5, t) for t in range(1, 2000))
    assert R.radam_rho(0.6, 1)[1] <= 4 + 1e-12           # the largest beta2 that is never rectified


def test_the_gpu_descriptor_case_crosses_the_radam_branches():
    """what the eight steps of tests/test_optimizers_gpu.py's descriptor case are meant to exercise"""
    from tests import test_optimizers_gpu as G
    assert len(G.SIZES) == 46 and G.STEPS == 8
    assert [R.radam_is_rectified(0.999, t) for t in range(1, G.STEPS + 1)] == [False] * 4 + [True] * 4
    assert not any(R.radam_is_rectified(0.5, t) for t in range(1, G.STEPS + 1))
    assert sorted(set(G.HYPER["beta2"])) == [0.5, 0.999] and G.HYPER["beta2"].count(0.5) == 2


def test_radam_branch_changes_the_update():
    """steps 1-4 move the parameter by stepParam * m only (no second moment in the update), step 5 divides by sqrt(v) + eps"""
    p = torch.ones(3, dtype=torch.float64)
    g = torch.tensor([0.5, -2.0, 4.0], dtype=torch.float64)
    opt = R.RAdam([p], 0.0, 0.1, 0.9, 0.999)
    for t in range(1, 5):
        before = p.clone()
        opt.step([g.clone()], 1.0)
        np.testing.assert_allclose((p - before).numpy(), (-0.1 * g).numpy(), rtol=1e-12)   # m / (1 - b1^t) == g for a constant gradient
    before = p.clone()
    opt.step([g.clone()], 1.0)
    d = (p - before) / before.new_tensor(-0.1) / torch.sign(g)
    assert float(d.max() - d.min()) < 1e-6 and float(d.max()) < 0.5, "rectified: the step no longer scales with |g|"


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_yogi_leaves_v_where_it_equals_the_rounded_square(dt):
    g0 = torch.tensor([0.3, 0.7, 0.0, 0.3], dtype=dt)
    v0 = g0 * g0                                         # as rounded by torch
    v0[3] = 1.0                                          # a control that does move
    if dt == torch.float32:                              # these squares are inexact: the exact product differs from the rounded one
        assert all(float(x) * float(x) != float(x * x) for x in g0[:2])
    p, g = torch.ones(4, dtype=dt), g0.clone()
    opt = R.Yogi([p], 0.0, 0.01, 0.9, 0.999)
    opt.vt[0].copy_(v0)
    opt.step([g], 1.0)
    assert torch.equal(opt.vt[0][:3], v0[:3])
    assert opt.vt[0][3] != v0[3]
    assert g[:3].tolist() == [0.0, 0.0, 0.0] and g[3] == g0[3] * g0[3]


def test_reduce_lr_on_plateau_sequence():
    from lamp_amd.nn import LearningRateSchedule as L
    k = K["reduce_lr_on_plateau"]
    lrs = L.reduceLROnPlateau(stopFactor=k["stopFactor"])
    st = lrs.init
    for epoch, loss, expected in k["sequence"]:
        st, f = lrs.learningRateFactor(st, epoch, loss)
        assert f == expected, (epoch, loss, f, expected)
    with pytest.raises(AssertionError):
        lrs.learningRateFactor(lrs.init, 0, None)


def test_epoch_count_schedules():
    from lamp_amd.nn import LearningRateSchedule as L

    def at(s, e):
        st, f = s.learningRateFactor(s.init, e, None)
        assert st == s.init
        return f
    assert [at(L.noop(), e) for e in (0, 7)] == [1.0, 1.0]
    d = L.decrement(20, 0.5)
    assert [at(d, e) for e in (0, 19, 20, 40)] == [1.0, 1.0, 0.5, 0.25]
    lin = L.linear(1.0, 0.1, 10)
    assert at(lin, 0) == 1.0 and at(lin, 5) == 1.0 + (0.1 - 1.0) * 0.5 and at(lin, 10) == 0.1
    assert at(lin, 11) == 0.1 and at(lin, 1000) == 0.1, "linear clamps at `end`"
    s = L.stepAfter(3, 0.2)
    assert [at(s, e) for e in (0, 3, 4)] == [1.0, 1.0, 0.2]
    c = L.cyclicSchedule(3.0, 10)
    assert at(c, 0) == 1.0 and at(c, 5) == 3.0 and at(c, 10) == 1.0        # start, half a period, a full period
    assert at(c, 2) == 1.0 + 2.0 * (2 / 5.0)
    assert at(c, 7) == 3.0 + (3.0 + (1.0 - 3.0) * (7 / 5.0))               # the falling half as LearningRateSchedule.scala:105-111 writes it
    assert L.interpolate(1.0, 3.0, 4.0, 1.0) == 1.5
    assert at(L.fromEpochCount(lambda e: e * 2), 4) == 8.0


def test_public_names_exist():
    from lamp_amd import nn
    for name in ("RAdam", "RAdam_factory", "Yogi", "Yogi_factory", "LearningRateSchedule"):
        assert callable(getattr(nn, name, None)), name
    for name in ("noop", "decrement", "linear", "stepAfter", "cyclicSchedule", "fromEpochCount", "interpolate", "reduceLROnPlateau"):
        assert callable(getattr(nn.LearningRateSchedule, name, None)), name
    from lamp_amd._capi import parse_header, HEADERS
    decls = {}
    for h in HEADERS:
        decls.update(parse_header(h))
    for fn in ("lamp_radam_step_", "lamp_yogi_step_", "lamp_optimizer_radam", "lamp_optimizer_yogi"):
        assert fn in decls, fn
