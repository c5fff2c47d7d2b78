"""nn/Shampoo.scala restated op by op in torch on the CPU: the yardstick of tests/test_shampoo.py and tests/test_shampoo_gpu.py.

Everything is as the reference writes it: the "inverse fourth root" scales the ROWS of U (Shampoo.scala:143-146),
a side is a vector iff its dimension is > 512 (diagonalThreshold is never read), momentum blends into the gradient tensors it is handed,
and the roots are recomputed on every step up to step 100 and on multiples of updatePreconditionerEveryNIterations afterwards.
`paper=True` is the one keyword the reference lacks: the COLUMNS of U are scaled, which gives U diag(s^-1/4) U^T."""
import json
import os

import torch

from tests.optim_ref import gradient_clipping_in_place

KATS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shampoo_kats.json")))


# The trajectory case shared by the CPU and the GPU tests: sides 6 and 75, 16 and 144 (a second row per lane, the largest side of the
# ResNet), 130 (the global-workspace form; rank 4 per step, so rank-deficient throughout) and 4, 7 and 1 x 1 (a 1-D parameter), 3 and a
# vector right side (513), a vector left side (600) and 2, and one parameter whose gradient is None.
TRAJ_SHAPES = [[6, 3, 5, 5], [16, 144], [130, 4], [7], [3, 513], [600, 2], [4, 3]]
TRAJ_NONE_AT = 6
TRAJ_STEPS = 8
TRAJ_GRAD_SCALE = 0.02          # keeps s_max of every statistic below 1, i.e. kappa below 1e4 against eps = 1e-4 (test_shampoo.py checks it)
TRAJ_CLIP = 1.0                 # the global norm of a step's gradients is about 1.55: the clipping is active
TRAJ_LR = 0.01


def trajectory_inputs():
    """f32-representable parameters and per-step gradients (seeded normal; one parameter's gradient is None)"""
    gen = torch.Generator().manual_seed(16)
    params = [torch.randn(s, generator=gen, dtype=torch.float32) for s in TRAJ_SHAPES]
    steps = []
    for _ in range(TRAJ_STEPS):
        gs = [torch.randn(s, generator=gen, dtype=torch.float32) * TRAJ_GRAD_SCALE for s in TRAJ_SHAPES]
        gs[TRAJ_NONE_AT] = None
        steps.append(gs)
    return params, steps


def recomputes(stepCount: int, every: int) -> bool:
    """Shampoo.scala:137-139, negated: whether this step (counted from 1) recomputes the inverse roots"""
    return not (stepCount > 100 and stepCount % every != 0)


def inverse_root(stat: torch.Tensor, dtype, paper: bool) -> torch.Tensor:
    """Shampoo.scala:142-149 for one side"""
    if stat.dim() == 2:
        u, s, vt = torch.linalg.svd(stat.double())
        s2 = s.pow(-0.25)
        if paper:
            return (u * s2.view(1, -1)).mm(u.t()).to(dtype)
        return (u * s2.view(-1, 1)).mm(vt).to(dtype)
    return stat.pow(-0.25)


class Shampoo:
    def __init__(self, parameters, learningRate=0.001, clip=None, eps=1e-4, diagonalThreshold=256, updatePreconditionerEveryNIterations=100,
                 momentum=0.0, paper=False):
        n = len(parameters)
        per = lambda v: [float(x) for x in v] if hasattr(v, "__len__") else [float(v)] * n
        self.parameters, self.learningRate, self.momentum = parameters, per(learningRate), per(momentum)
        self.clip, self.eps, self.every, self.paper = clip, eps, updatePreconditionerEveryNIterations, paper

        def side(p, d):
            t = torch.ones(d, dtype=p.dtype) if d > 512 else torch.eye(d, dtype=p.dtype)
            t *= eps
            return t
        self.lt = [side(p, p.shape[0]) for p in parameters]
        self.ltinv = [t.clone() for t in self.lt]
        self.rt = [side(p, p.numel() // p.shape[0]) for p in parameters]
        self.rtinv = [t.clone() for t in self.rt]
        self.lastGradient = [torch.zeros_like(p) for p in parameters]
        self.stepCount = 0

    @property
    def state(self):
        s = [torch.tensor(float(self.stepCount), dtype=torch.float64)]
        for a, b in zip(self.lt, self.ltinv):
            s += [a, b]
        for a, b in zip(self.rt, self.rtinv):
            s += [a, b]
        return s + self.lastGradient

    def step(self, gradients, scheduleFactor=1.0):
        if self.clip is not None:
            gradient_clipping_in_place(gradients, self.clip)
        self.stepCount += 1
        for i, (p, g) in enumerate(zip(self.parameters, gradients)):
            if g is None:
                continue
            lr, mom = self.learningRate[i], self.momentum[i]
            if mom > 0:
                g *= (1.0 - mom)
                torch.add(g, self.lastGradient[i], alpha=mom, out=g)
                self.lastGradient[i].copy_(g)
            gm = g.view(g.shape[0], -1)
            lt, rt = self.lt[i], self.rt[i]
            if lt.dim() == 2:
                lt += gm.mm(gm.t())
            else:
                lt += (gm * gm).sum(dim=1)
            if rt.dim() == 2:
                rt += gm.t().mm(gm)
            else:
                rt += (gm * gm).sum(dim=0)
            if recomputes(self.stepCount, self.every):
                self.ltinv[i].copy_(inverse_root(lt, g.dtype, self.paper))
                self.rtinv[i].copy_(inverse_root(rt, g.dtype, self.paper))
            li, ri = self.ltinv[i], self.rtinv[i]
            t1 = li.mm(gm) if lt.dim() == 2 else li.unsqueeze(1) * gm
            t2 = t1.mm(ri) if rt.dim() == 2 else t1 * ri.unsqueeze(0)
            p.add_(t2.view(g.shape), alpha=-lr)
