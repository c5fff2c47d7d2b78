"""Shampoo without a GPU: the restatement of tests/shampoo_ref.py reproduces the reference's own known answers (shampoo.test.scala:18-60),
its "inverse fourth root" is the diagonal matrix the kernels' reference mode stores, the preconditioner schedule is the reference's,
the shared trajectory case stays within the conditioning the GPU tests' bounds assume, and the public names exist."""
import os

import numpy as np
import pytest
import torch

from tests import shampoo_ref as R

K = R.KATS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_shampoo_reproduces_the_reference_kat():
    k = K["matrix"]
    p = torch.tensor([k["init"]], dtype=torch.float64)
    g = torch.tensor([k["gradients"]], dtype=torch.float64)
    opt = R.Shampoo([p], learningRate=k["learningRate"])
    opt.step([g], 1.0)
    assert np.round(p[0].numpy(), 4).tolist() == k["step1"]
    opt.step([g], 1.0)
    assert np.round(p[0].numpy(), 4).tolist() == k["step2"]
    assert g[0].tolist() == k["gradients"], "without momentum the gradients are only read"


def test_the_column_scaled_root_gives_other_values():
    """the known answer pins the row scaling: the paper's L^-1/4 moves the second parameter to 0.9168 / 0.8580 instead"""
    k = K["matrix"]
    p = torch.tensor([k["init"]], dtype=torch.float64)
    g = torch.tensor([k["gradients"]], dtype=torch.float64)
    opt = R.Shampoo([p], learningRate=k["learningRate"], paper=True)
    opt.step([g], 1.0)
    assert np.round(p[0].numpy(), 4).tolist() == [0.9445, 0.9168]
    opt.step([g], 1.0)
    assert np.round(p[0].numpy(), 4).tolist() == [0.9053, 0.8580]


def test_the_diagonal_case_of_the_reference_runs_and_stays_finite():
    k = K["diagonal"]
    gen = torch.Generator().manual_seed(3)
    p = torch.ones(k["shape"], dtype=torch.float64)
    g = torch.rand(k["shape"], generator=gen, dtype=torch.float64)
    opt = R.Shampoo([p], learningRate=k["learningRate"])
    assert opt.lt[0].shape == (1, 1) and opt.rt[0].shape == (513,), "a side is a vector iff it is > 512"
    for _ in range(2):
        opt.step([g], 1.0)
    assert torch.isfinite(p).all() and not torch.equal(p, torch.ones_like(p))


@pytest.mark.parametrize("shape,dt", [((6, 450), torch.float32), ((16, 144), torch.float32), ((144, 16), torch.float32), ((256, 64), torch.float32),
                                      ((512, 512), torch.float32), ((144, 16), torch.float64)])
def test_the_reference_root_is_the_diagonal_of_sorted_singular_values(shape, dt):
    """the design's premise: (u * s^-1/4 as a column).mm(vt) of a symmetric positive-definite matrix is diag(sort_desc(s)^-1/4), within
    1e-6 of its largest entry (2e-7 measured for f32 statistics, 5e-14 for f64)"""
    gen = torch.Generator().manual_seed(5)
    stat = 1e-4 * torch.eye(shape[0], dtype=dt)
    for _ in range(3):
        g = torch.randn(shape, generator=gen, dtype=dt) * 0.05
        stat += g.mm(g.t())
    root = R.inverse_root(stat, torch.float64, paper=False)
    s = torch.linalg.svdvals(stat.double())
    want = torch.diag(torch.sort(s, descending=True).values.pow(-0.25))
    err = float((root - want).abs().max() / want.abs().max())
    print(f"{shape} {dt}: distance from diag(sort_desc(s)^-1/4) = {err:.2e}")
    assert err <= 1e-6


def test_schedule_recomputes_on_steps_1_to_100_then_on_multiples_of_n():
    for every in (1, 3, 100, 250):
        got = [t for t in range(1, 1001) if R.recomputes(t, every)]
        assert got == list(range(1, 101)) + [t for t in range(101, 1001) if t % every == 0]


def test_trajectory_case_is_conditioned_as_the_gpu_bounds_assume():
    """kappa = s_max / s_min of every matrix statistic of the shared trajectory stays below 1e4 in f32, for each momentum and clipping"""
    worst = 0.0
    for mom in (0.0, 0.5):
        for clip in (None, R.TRAJ_CLIP):
            params, steps = R.trajectory_inputs()
            ps = [p.clone() for p in params]
            opt = R.Shampoo(ps, learningRate=R.TRAJ_LR, momentum=mom, clip=clip)
            for gs in steps:
                opt.step([None if g is None else g.clone() for g in gs], 1.0)
                for stat in opt.lt + opt.rt:
                    if stat.dim() == 2:
                        s = torch.linalg.svdvals(stat.double())
                        worst = max(worst, float(s.max() / s.min()))
    print(f"largest kappa of the trajectory case: {worst:.3e}")
    assert worst < 1e4


def test_names_are_exported():
    from lamp_amd import nn, sten
    assert callable(nn.Shampoo) and callable(nn.Shampoo_factory) and callable(sten.symmetricEig)
    assert "diagonalThreshold" in nn.Shampoo.__doc__ and "IGNORED" in nn.Shampoo.__doc__
    hip = open(os.path.join(ROOT, "include", "lamp_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "lamp_host.h")).read()
    assert "int lamp_symmetric_eig(" in hip and "int lamp_shampoo_step_(" in hip and "int lamp_optimizer_shampoo(" in host
