"""torch-CPU restatement of AdamW.step (AdamW.scala:101-176), SGDW.step (SGD.scala:46-98), RAdam.step (RAdam.scala:67-140) and Yogi.step
(Yogi.scala:73-133), op by op as the reference calls ATen:
mul_, add(out=), addcmul(out=), sqrt, addcdiv(out=), pow_, sign_, sub(out=).  Any floating dtype, several tensors, one hyperparameter
value per tensor (a scalar is repeated), optional clipping, undefined (None) gradients skipped with the step count still advancing.
Yogi MUTATES the gradient tensors it is handed, as the reference does."""
import json
import math
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "optimizer_kats.json")) as f:
    KATS = json.load(f)


def gradient_clipping_in_place(gradients, theta):
    """nn/package.scala:72-100."""
    gs = [g for g in gradients if g is not None]
    if not gs:
        return
    s = torch.zeros(1, dtype=gs[0].dtype)
    for g in gs:
        s += torch.norm(g.view(-1), 2.0, [0], False).pow(2.0)
    scalar = torch.tensor(theta, dtype=gs[0].dtype) / torch.sqrt(s)
    s2 = torch.minimum(scalar, torch.ones(1, dtype=gs[0].dtype))
    for g in gs:
        g.mul_(s2)


def radam_rho(b2, stepCount):
    """(rho, rhoInf, beta2PowT) of RAdam.scala:98-101."""
    beta2PowT = math.pow(b2, float(stepCount))
    rhoInf = (2.0 / (1.0 - b2)) - 1
    rho = rhoInf - (2.0 * stepCount * beta2PowT / (1.0 - beta2PowT))
    return rho, rhoInf, beta2PowT


def radam_is_rectified(b2, stepCount):
    return radam_rho(b2, stepCount)[0] > 4


class _Moments:
    def __init__(self, parameters, weightDecay, learningRate, beta1, beta2, eps, clip):
        self.parameters = list(parameters)
        n = len(self.parameters)
        per = lambda v: [float(x) for x in v] if hasattr(v, "__len__") else [float(v)] * n
        self.weightDecay, self.learningRate, self.beta1, self.beta2 = per(weightDecay), per(learningRate), per(beta1), per(beta2)
        self.eps, self.clip = eps, clip
        self.mt = [torch.zeros_like(p) for p in self.parameters]
        self.vt = [torch.zeros_like(p) for p in self.parameters]
        self.stepCount = 0

    def state(self):
        return [torch.tensor(float(self.stepCount), dtype=torch.float64)] + self.mt + self.vt

    def load(self, tensors):
        for cur, inc in zip(self.state()[1:], list(tensors)[1:]):
            cur.copy_(inc)
        self.stepCount = int(tensors[0].item())


class AdamW(_Moments):
    """AdamW.scala:101-176.  mixedPrecision: a 16-bit parameter gets an f32 working copy and f32 moments, its gradient is widened, and the
    model parameter is written as the cast of the working copy (AdamW.scala:48-63,167-169).  The working copies come last in the state."""

    def __init__(self, parameters, weightDecay, learningRate=0.001, beta1=0.9, beta2=0.999, eps=1e-8, clip=None, debias=True,
                 mixedPrecision=False):
        super().__init__(parameters, weightDecay, learningRate, beta1, beta2, eps, clip)
        self.debias = debias
        self.upCast = lambda t: t.float() if mixedPrecision and t.dtype in (torch.float16, torch.bfloat16) else t
        self.workingCopy = [None if self.upCast(p) is p else self.upCast(p) for p in self.parameters]
        self.mt = [self.upCast(torch.zeros_like(p)) for p in self.parameters]
        self.vt = [self.upCast(torch.zeros_like(p)) for p in self.parameters]

    def state(self):
        return super().state() + [w for w in self.workingCopy if w is not None]

    def step(self, gradients, scheduleFactor=1.0):
        if self.clip is not None:
            gradient_clipping_in_place(gradients, self.clip)
        self.stepCount += 1
        for i, (paramInModel, g0) in enumerate(zip(self.parameters, gradients)):
            if g0 is None:
                continue
            mt, vt = self.mt[i], self.vt[i]
            wd, b1, b2, lr = self.weightDecay[i], self.beta1[i], self.beta2[i], self.learningRate[i]
            g = self.upCast(g0)
            mt.mul_(b1)
            torch.add(mt, g, alpha=1.0 - b1, out=mt)
            vt.mul_(b2)
            torch.addcmul(vt, g, g, value=1 - b2, out=vt)
            denom = torch.sqrt(vt)
            denom.add_(self.eps, alpha=1.0)
            if self.debias:
                stepParam = scheduleFactor * lr * math.sqrt(1 - math.pow(b2, float(self.stepCount))) / (1 - math.pow(b1, float(self.stepCount)))
            else:
                stepParam = scheduleFactor * lr
            stepWd = stepParam * wd
            param = paramInModel if self.workingCopy[i] is None else self.workingCopy[i]
            if wd != 0.0:
                torch.add(param, param, alpha=-1 * stepWd, out=param)
            torch.addcdiv(param, mt, denom, value=-1 * stepParam, out=param)
            if param is not paramInModel:
                paramInModel.copy_(param.to(paramInModel.dtype))


class SGDW:
    """SGD.scala:46-98.  momentum None: no velocity; a value or one per tensor: velocity = zeros_like(param), which is the whole state."""

    def __init__(self, parameters, learningRate, weightDecay, momentum=None, clip=None):
        self.parameters = list(parameters)
        n = len(self.parameters)
        per = lambda v: [float(x) for x in v] if hasattr(v, "__len__") else [float(v)] * n
        self.learningRate, self.weightDecay, self.clip = per(learningRate), per(weightDecay), clip
        self.momentum = None if momentum is None else per(momentum)
        self.velocity = [None if momentum is None else torch.zeros_like(p) for p in self.parameters]

    def state(self):
        return [v for v in self.velocity if v is not None]

    def load(self, tensors):
        for cur, inc in zip(self.state(), tensors):
            cur.copy_(inc)

    def step(self, gradients, scheduleFactor=1.0):
        if self.clip is not None:
            gradient_clipping_in_place(gradients, self.clip)
        for i, (param, g) in enumerate(zip(self.parameters, gradients)):
            if g is None:
                continue
            wd, lr, velocity = self.weightDecay[i], self.learningRate[i], self.velocity[i]
            if velocity is None:
                if wd != 0.0:
                    torch.add(param, param, alpha=(-1) * wd * scheduleFactor, out=param)
                torch.add(param, g, alpha=(-1) * lr * scheduleFactor, out=param)
            else:
                velocity.mul_(self.momentum[i])
                torch.add(velocity, g, alpha=lr * scheduleFactor, out=velocity)
                if wd != 0.0:
                    torch.add(param, param, alpha=-1 * wd * scheduleFactor, out=param)
                torch.add(param, velocity, alpha=-1, out=param)


class RAdam(_Moments):
    def __init__(self, parameters, weightDecay, learningRate=0.001, beta1=0.9, beta2=0.999, eps=1e-8, clip=None):
        super().__init__(parameters, weightDecay, learningRate, beta1, beta2, eps, clip)

    def step(self, gradients, scheduleFactor=1.0):
        if self.clip is not None:
            gradient_clipping_in_place(gradients, self.clip)
        self.stepCount += 1
        for i, (param, g) in enumerate(zip(self.parameters, gradients)):
            if g is None:
                continue
            mt, vt = self.mt[i], self.vt[i]
            wd, b1, b2, lr = self.weightDecay[i], self.beta1[i], self.beta2[i], self.learningRate[i]
            mt.mul_(b1)
            torch.add(mt, g, alpha=1.0 - b1, out=mt)
            vt.mul_(b2)
            torch.addcmul(vt, g, g, value=1 - b2, out=vt)
            rho, rhoInf, beta2PowT = radam_rho(b2, self.stepCount)
            stepWd = scheduleFactor * wd
            if wd != 0.0:
                torch.add(param, param, alpha=-1 * stepWd, out=param)
            if rho > 4:
                stepParam = scheduleFactor * lr * math.sqrt(
                    (1 - beta2PowT) * ((rho - 4) / (rhoInf - 4)) * ((rho - 2) / rho) * (rhoInf / (rhoInf - 2))
                ) / (1 - math.pow(b1, float(self.stepCount)))
                denom = torch.sqrt(vt)
                denom.add_(self.eps, alpha=1.0)
                torch.addcdiv(param, mt, denom, value=-1 * stepParam, out=param)
            else:
                stepParam = scheduleFactor * lr / (1 - math.pow(b1, float(self.stepCount)))
                torch.add(param, mt, alpha=-1 * stepParam, out=param)


class Yogi(_Moments):
    def __init__(self, parameters, weightDecay, learningRate=0.01, beta1=0.9, beta2=0.999, eps=1e-3, clip=None, debias=True):
        super().__init__(parameters, weightDecay, learningRate, beta1, beta2, eps, clip)
        self.debias = debias

    def step(self, gradients, scheduleFactor=1.0):
        if self.clip is not None:
            gradient_clipping_in_place(gradients, self.clip)
        self.stepCount += 1
        for i, (param, g) in enumerate(zip(self.parameters, gradients)):
            if g is None:
                continue
            mt, vt = self.mt[i], self.vt[i]
            wd, b1, b2, lr = self.weightDecay[i], self.beta1[i], self.beta2[i], self.learningRate[i]
            mt.mul_(b1)
            torch.add(mt, g, alpha=1.0 - b1, out=mt)
            g.pow_(2.0)
            tmp = torch.sub(vt, g, alpha=1.0)
            tmp.sign_()
            g.mul_(tmp)
            torch.sub(vt, g, alpha=1.0 - b2, out=vt)
            debiasTerm = 1.0 / (1 - math.pow(b1, float(self.stepCount))) if self.debias else 1.0
            stepParam = scheduleFactor * lr * debiasTerm
            stepWd = scheduleFactor * wd
            denom = torch.sqrt(vt)
            if self.debias:
                denom.mul_(1.0 / math.sqrt(1 - math.pow(b2, float(self.stepCount))))
            denom.add_(self.eps)
            if wd != 0.0:
                torch.add(param, param, alpha=-1 * stepWd, out=param)
            torch.addcdiv(param, mt, denom, value=-1 * stepParam, out=param)
