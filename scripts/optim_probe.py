#!/usr/bin/env python3
"""The fused RAdam / Yogi steps against the same updates composed from the library's own element-wise operators (mul_, addOut,
addcmulOut, sqrt, addcdivOut, sign, subOut: the reference's call chain, about ten launches per tensor for RAdam and thirteen plus two
temporaries for Yogi), with the fused AdamW step as the yardstick, on two parameter sets in f32:

    resnet   the CIFAR ResNet's 37 parameter tensors (launch-bound)
    lm       the parameters of `bench.py --workload lm` (12 x 768 x 12 heads, context 384: bandwidth-bound)

All forms alternate inside one process after a warm-up of each.  A window is `reps` steps followed by a device synchronise, sized to
last at least --window seconds; the median per step over the windows is reported with the spread (min - max).  RAdam is timed past
its fifth step (the rectified branch: the one with the square root and the division).  Achieved bytes/s counts 7 accesses per element
for RAdam and AdamW (p, g, m, v read; p, m, v written) and 8 for Yogi (the gradient is written back) against the 6.29 TB/s a float4
copy measures on the MI355X (8 TB/s specified).

    python scripts/optim_probe.py [--windows 5] [--window 0.5] [--sets resnet,lm]
"""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lamp_amd import nn, sten as S   # noqa: E402
from lamp_amd._capi import lib       # noqa: E402

HBM_COPY = 6.29e12
LR, WD, B1, B2 = 1e-3, 0.01, 0.9, 0.999


def composed_radam(ps, gs, ms, vs, t, eps=1e-8):
    beta2PowT = B2 ** t
    rhoInf = 2.0 / (1.0 - B2) - 1
    rho = rhoInf - 2.0 * t * beta2PowT / (1.0 - beta2PowT)
    for p, g, m, v in zip(ps, gs, ms, vs):
        m *= B1
        S.STen.addOut(m, m, g, 1.0 - B1)
        v *= B2
        S.STen.addcmulOut(v, v, g, g, 1.0 - B2)
        S.STen.addOut(p, p, p, -WD)
        if rho > 4:
            step = LR * math.sqrt((1 - beta2PowT) * ((rho - 4) / (rhoInf - 4)) * ((rho - 2) / rho) * (rhoInf / (rhoInf - 2))) / (1 - B1 ** t)
            d = v.sqrt()
            d += eps
            S.STen.addcdivOut(p, p, m, d, -step)
        else:
            S.STen.addOut(p, p, m, -LR / (1 - B1 ** t))


def composed_yogi(ps, gs, ms, vs, t, eps=1e-3):
    for p, g, m, v in zip(ps, gs, ms, vs):
        m *= B1
        S.STen.addOut(m, m, g, 1.0 - B1)
        S.STen.mulOut(g, g, g)                         # gradients.pow_(2)
        s = v.sub(g, 1.0).sign()
        g *= s
        S.STen.subOut(v, v, g, 1.0 - B2)
        d = v.sqrt()
        d *= 1.0 / math.sqrt(1 - B2 ** t)
        d += eps
        S.STen.addOut(p, p, p, -WD)
        S.STen.addcdivOut(p, p, m, d, -LR / (1 - B1 ** t))


def window(fn, reps):
    lib.lamp_device_synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    lib.lamp_device_synchronize()
    return (time.perf_counter() - t0) / reps


def parameter_shapes(which):
    if which == "resnet":
        return [p.value.shape for p in nn.resnet(100, 0.0, S.F32).parameters]
    from lamp_amd import transformer as TR
    ctx, vocab, dim, heads, blocks = 384, 256, 768, 12, 12
    return [p.value.shape for p in TR.LanguageModelLoss(ctx, vocab, blocks, dim, dim // heads, heads, dim * 4, 0.0, -1000, S.F32, 0).parameters]


def probe(which, windows, seconds):
    shapes = parameter_shapes(which)
    numel = sum(math.prod(s) for s in shapes)
    fresh = lambda scale=1.0: [S.STen.randn(s) * scale for s in shapes]
    forms = {}

    def fused(make):
        ps, gs = fresh(), fresh(0.1)
        opt = make(ps)
        return lambda: opt.step(gs, 1.0)

    def composed(chain):
        ps, gs, ms, vs = fresh(), fresh(0.1), [S.STen.zeros(s) for s in shapes], [S.STen.zeros(s) for s in shapes]
        return lambda: chain(ps, gs, ms, vs, 10)

    forms["RAdam fused"] = (fused(lambda ps: nn.RAdam(ps, WD, LR, B1, B2)), 7)
    forms["RAdam composed"] = (composed(composed_radam), 7)
    forms["Yogi fused"] = (fused(lambda ps: nn.Yogi(ps, WD, LR, B1, B2)), 8)
    forms["Yogi composed"] = (composed(composed_yogi), 8)
    forms["AdamW fused"] = (fused(lambda ps: nn.AdamW(ps, WD, LR, B1, B2)), 7)
    reps = {}
    for name, (fn, _) in forms.items():                # warm-up (RAdam past its branch change), then the window length
        for _ in range(8):
            fn()
        reps[name] = max(3, int(math.ceil(seconds / window(fn, 3))))
    ts = {name: [] for name in forms}
    for _ in range(windows):                           # alternate
        for name, (fn, _) in forms.items():
            ts[name].append(window(fn, reps[name]))
    print(f"{which}: {len(shapes)} tensors, {numel} elements f32, windows of >= {seconds} s")
    for name, (_, streams) in forms.items():
        t = ts[name]
        med = statistics.median(t)
        print(f"{which}: {name:15s} {1e6 * med:10.1f} us per step (min {1e6 * min(t):.1f}, max {1e6 * max(t):.1f}, {reps[name]} steps per window), "
              f"{streams} accesses per element = {streams * 4 * numel / med / 1e12:.2f} TB/s ({100 * streams * 4 * numel / med / HBM_COPY:.0f} % of a float4 copy)")
    for kind in ("RAdam", "Yogi"):
        f, c = ts[f"{kind} fused"], ts[f"{kind} composed"]
        print(f"{which}: {kind} composed / fused {statistics.median(c) / statistics.median(f):.2f} (fused max {1e6 * max(f):.1f} us against composed min {1e6 * min(c):.1f} us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--sets", default="resnet,lm")
    a = ap.parse_args()
    for which in a.sets.split(","):
        probe(which, a.windows, a.window)


if __name__ == "__main__":
    main()
