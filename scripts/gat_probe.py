#!/usr/bin/env python3
"""Graph attention at ogbn-arxiv's size with self loops added (N = 169 343, E = 1 166 243 + N, f32): forward + backward of the fused
GraphAttentionAggregate node against the reference's chain of Exp / IndexAdd / Log / IndexSelect / Mult nodes, H = 4 and 8 heads of
V = 32.

The synthetic graph of scripts/gcn_probe.py (the data set's counts, a share of the edges drawn towards a handful of hub nodes so that a
few destinations have thousands of incoming edges) plus one self loop per node.  Scores are uniform in [-4, 4], values normal.  Both
forms alternate inside one process, after a warm-up of each; every repetition is (aggregate(score, value) * l).sum().backprop() with
score and value as parameters and ends in a device synchronise; medians are reported.  The yardstick is the traffic of a perfect gather
per kernel (every value / gradient row an edge needs read once, every result written once; the kernel timer's byte counts), and the fused
kernels' rates come from the kernel timer.

    python scripts/gat_probe.py [--reps 30] [--windows 5]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lamp_amd import autograd as A, graph as G, sten as S   # noqa: E402
from lamp_amd._capi import lib                             # noqa: E402
from scripts.gcn_probe import N, edges, timed               # noqa: E402

KERNELS = ("gat_forward", "gat_backward_score", "gat_backward_value")


def step(score, value, lf, si, sj, heads, csr, fused):
    prev = G.graphAttentionFused(fused)
    try:
        sv, vv = A.param(score), A.param(value)
        (G.graphAttentionAggregate(sv, vv, si, sj, heads, csr) * lf).sum().backprop()
        return sv.partialDerivative, vv.partialDerivative
    finally:
        G.graphAttentionFused(prev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    i, j = edges()
    i, j = np.concatenate([i, np.arange(N)]), np.concatenate([j, np.arange(N)])
    e = i.shape[0]
    deg_in, deg_out = np.bincount(j, minlength=N), np.bincount(i, minlength=N)
    print(f"N {N} E {e}: incoming edges median {int(np.median(deg_in))} max {int(deg_in.max())}, destinations above {G.gatLongRow()}: "
          f"{int((deg_in > G.gatLongRow()).sum())}; outgoing max {int(deg_out.max())}")
    si, sj = S.STen.from_numpy(i), S.STen.from_numpy(j)
    t0 = time.perf_counter()
    csr = G.computeEdgeCsr(si, sj, N)
    lib.lamp_device_synchronize()
    print(f"edge CSR, both groupings (range check, sort, bincount, prefix sum each): {1e3 * (time.perf_counter() - t0):.2f} ms, once per graph")
    buf = ctypes.create_string_buffer(1 << 16)
    for h, v in ((4, 32), (8, 32)):
        score = (S.STen.rand([e, h]) * 8.0) - 4.0
        value, lf = S.STen.randn([N, h, v]), A.const(S.STen.randn([N, h * v]))
        run = lambda fused: step(score, value, lf, si, sj, h, csr, fused)
        for fused in (True, False):                       # warm-up of both forms
            for _ in range(3):
                run(fused)
        (ds_f, dv_f), (ds_c, dv_c) = run(True), run(False)
        for name, f, c in (("dscore", ds_f, ds_c), ("dvalue", dv_f, dv_c)):
            f, c = f.to_numpy(), c.to_numpy()
            print(f"H {h} V {v}: {name} fused vs composed max |diff| {np.abs(f - c).max():.3e} of max {np.abs(c).max():.3e}")
        ts = {True: [], False: []}
        for _ in range(a.windows):                        # alternate
            for fused in (True, False):
                ts[fused] += timed(lambda: run(fused), a.reps)
        lib.lamp_kernel_timer_report(buf, len(buf))       # clears the log
        lib.lamp_kernel_timer_enable(1)
        for _ in range(a.reps):
            run(True)
        lib.lamp_device_synchronize()
        lib.lamp_kernel_timer_enable(0)
        lib.lamp_kernel_timer_report(buf, len(buf))
        m_f, m_c = statistics.median(ts[True]), statistics.median(ts[False])
        q = lambda t: f"{1e3 * statistics.median(t):.3f} ms (min {1e3 * min(t):.3f}, p90 {1e3 * sorted(t)[int(0.9 * len(t))]:.3f})"
        print(f"H {h} V {v}: forward + backward fused {q(ts[True])}, composed {q(ts[False])}, composed / fused {m_c / m_f:.2f}")
        total_ms = total_bytes = 0.0
        for line in buf.value.decode().splitlines():
            f = line.split()
            if f[0] in KERNELS:
                ms, nbytes = float(f[2]) / int(f[1]), float(f[4])
                total_ms, total_bytes = total_ms + ms, total_bytes + nbytes
                print(f"H {h} V {v}: {f[0]} {ms:.3f} ms per launch, perfect gather {nbytes / 1e6:.1f} MB = {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s")
        print(f"H {h} V {v}: the three kernels {total_ms:.3f} ms, {total_bytes / 1e6:.1f} MB = {total_bytes / (total_ms * 1e-3) / 1e12:.2f} TB/s; "
              f"over the whole step (loss included) {total_bytes / m_f / 1e12:.2f} TB/s fused, {total_bytes / m_c / 1e12:.2f} TB/s composed")


if __name__ == "__main__":
    main()
