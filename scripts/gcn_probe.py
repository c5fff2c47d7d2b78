#!/usr/bin/env python3
"""GCN aggregation at ogbn-arxiv's size (example-arxiv: N = 169 343, E = 1 166 243, f32): forward + backward of the fused GcnAggregation
node against the composed IndexSelect / IndexAdd chain, D = 128 and 256.

A synthetic graph with the data set's counts: most endpoints uniform, a share drawn from a handful of hub nodes so that a few rows have
thousands of neighbours (the largest degree of ogbn-arxiv is about 13 000).  Both forms alternate inside one process, after a warm-up
of each; every repetition ends in a device synchronise; medians are reported.  The yardstick is the traffic of a perfect gather,
((2E + N) * D + N * D) * 4 bytes per direction (every neighbour row and the node's own row read once, the result written once), twice
that for forward + backward.

    python scripts/gcn_probe.py [--reps 30] [--windows 5]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lamp_amd import autograd as A, graph as G, sten as S   # noqa: E402
from lamp_amd._capi import lib                             # noqa: E402

N, E = 169_343, 1_166_243


def edges(seed=1, hubs=8, hub_share=0.09):
    rng = np.random.default_rng(seed)
    i = rng.integers(0, N, E)
    j = rng.integers(0, N, E)
    to_hub = rng.random(E) < hub_share
    j[to_hub] = rng.integers(0, hubs, int(to_hub.sum()))
    same = i == j
    j[same] = (j[same] + 1) % N
    return i.astype(np.int64), j.astype(np.int64)


def step(x, lf, adj, fused):
    prev = G.gcnFused(fused)
    try:
        xv = A.param(x)
        (G.gcnAggregation(xv, adj) * lf).sum().backprop()
        return xv.partialDerivative
    finally:
        G.gcnFused(prev)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        lib.lamp_device_synchronize()
        t0 = time.perf_counter()
        fn()
        lib.lamp_device_synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    i, j = edges()
    deg = np.bincount(np.concatenate([i, j]), minlength=N)
    print(f"N {N} E {E}: degree median {int(np.median(deg))} max {int(deg.max())}, rows above {G.longRow()}: {int((deg > G.longRow()).sum())}")
    si, sj = S.STen.from_numpy(i), S.STen.from_numpy(j)
    t0 = time.perf_counter()
    adj = G.computeAdjacency(si, sj, N, S.F32)
    lib.lamp_device_synchronize()
    print(f"adjacency (range check, sort, bincount, prefix sum): {1e3 * (time.perf_counter() - t0):.2f} ms, once per graph")
    for d in (128, 256):
        x, lf = S.STen.randn([N, d]), A.const(S.STen.randn([N, d]))
        for fused in (True, False):                       # warm-up of both forms
            for _ in range(3):
                step(x, lf, adj, fused)
        g_f, g_c = step(x, lf, adj, True).to_numpy(), step(x, lf, adj, False).to_numpy()
        print(f"D {d}: gradient fused vs composed max |diff| {np.abs(g_f - g_c).max():.3e} of max {np.abs(g_c).max():.3e}")
        ts = {True: [], False: []}
        for _ in range(a.windows):                        # alternate
            for fused in (True, False):
                ts[fused] += timed(lambda: step(x, lf, adj, fused), a.reps)
        # the aggregation kernel alone (two launches per step), from the kernel timer
        buf = __import__("ctypes").create_string_buffer(1 << 16)
        lib.lamp_kernel_timer_report(buf, len(buf))
        lib.lamp_kernel_timer_enable(1)
        for _ in range(a.reps):
            step(x, lf, adj, True)
        lib.lamp_device_synchronize()
        lib.lamp_kernel_timer_enable(0)
        lib.lamp_kernel_timer_report(buf, len(buf))
        kern = [l.split() for l in buf.value.decode().splitlines() if l.startswith("gcn_aggregate ")][0]
        k_ms = float(kern[2]) / int(kern[1])
        gather = ((2 * E + N) * d + N * d) * 4
        m_f, m_c = statistics.median(ts[True]), statistics.median(ts[False])
        q = lambda v: f"{1e3 * statistics.median(v):.3f} ms (min {1e3 * min(v):.3f}, p90 {1e3 * sorted(v)[int(0.9 * len(v))]:.3f})"
        print(f"D {d}: forward + backward fused {q(ts[True])}, composed {q(ts[False])}, composed / fused {m_c / m_f:.2f}")
        print(f"D {d}: perfect gather {gather / 1e6:.1f} MB per direction; the step (two directions + the loss's mul and sum) moves it at "
              f"{2 * gather / m_f / 1e12:.2f} TB/s fused, {2 * gather / m_c / 1e12:.2f} TB/s composed; gcn_aggregate alone {k_ms:.3f} ms per launch = "
              f"{gather / (k_ms * 1e-3) / 1e12:.2f} TB/s")


if __name__ == "__main__":
    main()
