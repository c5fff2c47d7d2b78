#!/usr/bin/env python3
"""The batched Jacobi eigensolver (lamp_symmetric_eig, kernels/eig.hip) and the Shampoo step built on it.

    eig      one lamp_symmetric_eig call (values only, as Shampoo's reference mode asks; and with vectors) on one matrix eps I + G G^T of
             each side in {16, 128, 144, 256, 512} and on the CIFAR ResNet's set of matrix sides together, the sweeps each took, against
             torch.linalg.svd in f64 on the host's CPU for the same matrices (the reference has no GPU path here: Shampoo.scala:143
             decomposes on whatever device the statistics live on, through ATen's svd)
    step     nn.Shampoo on the ResNet's 37 parameter tensors in f32: a step that recomputes the inverse roots (every one of the first
             100) and a step between two recomputations (past step 100, off the period), with the fused AdamW step as the yardstick

All forms alternate inside one process after a warm-up of each.  A window is `reps` calls followed by a device synchronise, sized to
last at least --window seconds; the median per call over the windows is reported with the spread (min - max).

    python scripts/shampoo_probe.py [--windows 5] [--window 0.3]
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

SIDES = [16, 128, 144, 256, 512]
EPS = 1e-4


def window(fn, reps):
    lib.lamp_device_synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    lib.lamp_device_synchronize()
    return (time.perf_counter() - t0) / reps


def measure(forms, windows, seconds, caps=None):
    reps = {}
    for name, fn in forms.items():
        for _ in range(2):
            fn()
        reps[name] = max(2, int(math.ceil(seconds / window(fn, 2))))
        if caps and name in caps:
            reps[name] = min(reps[name], caps[name])
    ts = {name: [] for name in forms}
    for _ in range(windows):
        for name, fn in forms.items():
            ts[name].append(window(fn, reps[name]))
    return ts, reps


def report(prefix, ts, reps):
    for name, t in ts.items():
        print(f"{prefix}: {name:34s} {1e3 * statistics.median(t):10.3f} ms per call (min {1e3 * min(t):.3f}, max {1e3 * max(t):.3f}, {reps[name]} calls per window)")


def resnet_shapes():
    return [p.value.shape for p in nn.resnet(100, 0.0, S.F32).parameters]


def matrix_sides(shapes):
    out = []
    for s in shapes:
        d1, d2 = s[0], math.prod(s[1:])
        out += [d for d in (d1, d2) if d <= 512]
    return out


def statistic(n):
    import torch
    g = torch.randn(n, max(1, n // 4), dtype=torch.float64) * 0.05          # rank n/4: a degenerate cluster at eps, as Shampoo's statistics have
    return EPS * torch.eye(n, dtype=torch.float64) + g.mm(g.t())


def probe_eig(windows, seconds):
    import torch
    torch.manual_seed(0)
    sets = {f"side {n}": [statistic(n)] for n in SIDES}
    sides = matrix_sides(resnet_shapes())
    sets[f"resnet ({len(sides)} sides {min(sides)}..{max(sides)})"] = [statistic(n) for n in sides]
    for label, mats in sets.items():
        dev = [S.STen.from_numpy(a.numpy()) for a in mats]
        _, _, sweeps = S.symmetricEig(dev)
        forms = {"GPU values": lambda: S.symmetricEig(dev), "GPU values + vectors": lambda: S.symmetricEig(dev, vectors=True),
                 "CPU torch.linalg.svd f64": lambda: [torch.linalg.svd(a) for a in mats]}
        ts, reps = measure(forms, windows, seconds)
        print(f"eig {label}: sweeps min {min(sweeps)} max {max(sweeps)}")
        report(f"eig {label}", ts, reps)


def probe_step(windows, seconds):
    shapes = resnet_shapes()
    fresh = lambda scale=1.0: [S.STen.randn(s) * scale for s in shapes]

    def shampoo(period_step):
        ps, gs = fresh(), fresh(0.01)
        opt = nn.Shampoo(ps, learningRate=1e-4, updatePreconditionerEveryNIterations=10 ** 9)
        if period_step:                                  # past step 100 and never on the period: the stored roots are used
            st = [t.clone() for t in opt.state]      # (state()[0] is refreshed from the host counter whenever the state is asked for)
            st[0].fill_(1000.0)
            opt.load(st)
        return lambda: opt.step(gs, 1.0)

    ps, gs = fresh(), fresh(0.01)
    adam = nn.AdamW(ps, 0.01, 1e-3, 0.9, 0.999)
    # the recomputing form is timed within its first 100 steps only: 2 warm-up + 2 sizing + windows * reps calls stay below 100
    forms = {"Shampoo, roots recomputed": shampoo(False), "Shampoo, between recomputations": shampoo(True), "AdamW fused": lambda: adam.step(gs, 1.0)}
    ts, reps = measure(forms, windows, seconds, caps={"Shampoo, roots recomputed": (100 - 4) // windows})
    print(f"step: {len(shapes)} tensors f32, {len(matrix_sides(shapes))} matrix sides")
    report("step", ts, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--parts", default="eig,step")
    a = ap.parse_args()
    if "eig" in a.parts.split(","):
        probe_eig(a.windows, a.window)
    if "step" in a.parts.split(","):
        probe_step(a.windows, a.window)


if __name__ == "__main__":
    main()
