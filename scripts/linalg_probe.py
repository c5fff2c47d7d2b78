#!/usr/bin/env python3
"""The Cholesky family (kernels/linalg.hip): time per call and GFLOP/s of the factorisation, of a Cholesky solve, and of the product the
trailing update is at the same shape, in f32 and f64.

    shapes   batch 4096 of 8 x 8 (8 right-hand sides), batch 4096 of 32 x 32 (32), one 128 x 128 (128) - the LDS forms - and one
             4096 x 4096 (256), the blocked form
    cholesky lamp_linalg_cholesky (lower), status read-back included: n^3 / 3 operations per matrix
    solve    lamp_cholesky_solve on the factor: two substitutions, 2 n^2 nrhs operations per matrix
    update   C -= P P^T through lamp_baddbmm_out_transposed2 alone: at 4096 the first block column's update on views of one matrix (4032 x
             4032 x 64, ldc 4096), at the LDS sides (which make no such call) a [n, min(n, 64)] panel per matrix, for scale

All forms alternate inside one process after a warm-up of each.  A window is `reps` calls followed by a device synchronise, sized to
last at least --window seconds; the median per call over the windows is reported with the spread (min - max).  The plan of each call is
printed with it.  There is no earlier implementation to compare with: the figures are what these kernels do, nothing more.

    python scripts/linalg_probe.py [--windows 5] [--window 0.3] [--shapes small,big]
"""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lamp_amd import sten as S       # noqa: E402
from lamp_amd._capi import lib       # noqa: E402

SHAPES = {"small": [(4096, 8, 8), (4096, 32, 32), (1, 128, 128)], "big": [(1, 4096, 256)]}      # (batch, n, nrhs)
NB = 64


def window(fn, reps):
    lib.lamp_device_synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    lib.lamp_device_synchronize()
    return (time.perf_counter() - t0) / reps


def measure(forms, windows, seconds):
    reps = {}
    for name, fn in forms.items():
        for _ in range(2):
            fn()
        reps[name] = max(2, int(math.ceil(seconds / window(fn, 2))))
    ts = {name: [] for name in forms}
    for _ in range(windows):
        for name, fn in forms.items():
            ts[name].append(window(fn, reps[name]))
    return ts, reps


def spd(batch, n, dtype):
    import torch
    g = torch.Generator().manual_seed(n)
    m = torch.randn(n, n, generator=g, dtype=torch.float64)
    a = (m @ m.t() / n + torch.eye(n, dtype=torch.float64)).to(dtype)
    return a.expand(batch, n, n).contiguous() if batch > 1 else a


def probe(batch, n, nrhs, dtype, windows, seconds):
    import torch
    name = "f32" if dtype == torch.float32 else "f64"
    shape = [batch, n, n] if batch > 1 else [n, n]
    a = S.STen.from_numpy(spd(batch, n, dtype).numpy())
    b = S.STen.from_numpy(torch.randn(*shape[:-1], nrhs, dtype=torch.float64).to(dtype).numpy())
    factor = a.choleskyLower()
    work = a.view(batch, n, n).cloneTensor()
    if n > 128:      # the first block column's trailing update, on views of the working matrix
        c, p = work.narrow(1, NB, n - NB).narrow(2, NB, n - NB), work.narrow(1, NB, n - NB).narrow(2, 0, NB)
    else:
        c, p = work, work.narrow(2, 0, min(n, NB))
    m, k = c.shape[1], p.shape[2]
    flops = {"cholesky": batch * n ** 3 / 3, "solve": batch * 2.0 * n * n * nrhs, "update": batch * 2.0 * m * m * k}
    forms = {"cholesky": lambda: a.choleskyLower(), "solve": lambda: b.choleskySolve(factor, False),
             "update": lambda: lib.lamp_baddbmm_out_transposed2(c.h, c.h, p.h, p.h, 1.0, -1.0)}
    ts, reps = measure(forms, windows, seconds)
    for form, t in ts.items():
        med = statistics.median(t)
        print(f"{name} batch {batch} n {n} nrhs {nrhs}: {form:9s} {1e3 * med:10.4f} ms per call (min {1e3 * min(t):.4f}, max {1e3 * max(t):.4f}, "
              f"{reps[form]} calls per window)  {flops[form] / med / 1e9:10.2f} GFLOP/s", flush=True)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--shapes", default="small,big")
    args = ap.parse_args()
    for group in args.shapes.split(","):
        for batch, n, nrhs in SHAPES[group]:
            for dtype in (torch.float32, torch.float64):
                probe(batch, n, nrhs, dtype, args.windows, args.window)


if __name__ == "__main__":
    main()
