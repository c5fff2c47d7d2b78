#!/usr/bin/env python3
"""MPNN's two data movements at ogbn-arxiv's size (N = 169 343, E = 1 166 243, f32): forward + backward of the fused MpnnMessage node
against the chain of IndexSelect / Concatenate nodes, and of the fused MpnnAggregate node (both normalisations, aggregateJ) against the
chain of Mult / IndexAdd / Add nodes, each at two widths: node features D = 64 and 128 with Fe = 8 edge features (messages of 136 and 264
columns), transformed messages of M = 64 and 128 columns.

The synthetic graph of scripts/gcn_probe.py (the data set's counts, a share of the edges drawn towards a handful of hub nodes so that a
few nodes have thousands of edges).  Both forms alternate inside one process, after a warm-up of each; every repetition is
(node(...) * l).sum().backprop() with the node's inputs as parameters and ends in a device synchronise; medians are reported.  The
yardstick is the traffic of a perfect gather per kernel (every row an edge needs read once, every result written once; the kernel
timer's byte counts), and the fused kernels' rates come from the kernel timer.

    python scripts/mpnn_probe.py [--reps 30] [--windows 5]
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

FE = 8


def message_step(x, ef, lf, si, sj, csr, fused):
    prev = G.mpnnFused(fused)
    try:
        xv, ev = A.param(x), A.param(ef)
        (G.mpnnMessage(xv, ev, si, sj, csr) * lf).sum().backprop()
        return {"dx": xv.partialDerivative, "dedge": ev.partialDerivative}
    finally:
        G.mpnnFused(prev)


def aggregate_step(msg, lf, si, sj, csr, cache, fused):
    prev = G.mpnnFused(fused)
    try:
        mv = A.param(msg)
        (G.mpnnAggregate(N, mv, si, sj, True, True, True, csr, cache) * lf).sum().backprop()
        return {"dmsg": mv.partialDerivative}
    finally:
        G.mpnnFused(prev)


def measure(tag, run, kernels, reps, windows):
    buf = ctypes.create_string_buffer(1 << 16)
    for fused in (True, False):                       # warm-up of both forms
        for _ in range(3):
            run(fused)
    f, c = run(True), run(False)
    for name in f:
        a, b = f[name].to_numpy(), c[name].to_numpy()
        print(f"{tag}: {name} fused vs composed max |diff| {np.abs(a - b).max():.3e} of max {np.abs(b).max():.3e}")
    ts = {True: [], False: []}
    for _ in range(windows):                          # alternate
        for fused in (True, False):
            ts[fused] += timed(lambda: run(fused), reps)
    lib.lamp_kernel_timer_report(buf, len(buf))       # clears the log
    lib.lamp_kernel_timer_enable(1)
    for _ in range(reps):
        run(True)
    lib.lamp_device_synchronize()
    lib.lamp_kernel_timer_enable(0)
    lib.lamp_kernel_timer_report(buf, len(buf))
    m_f, m_c = statistics.median(ts[True]), statistics.median(ts[False])
    q = lambda t: f"{1e3 * statistics.median(t):.3f} ms (min {1e3 * min(t):.3f}, p90 {1e3 * sorted(t)[int(0.9 * len(t))]:.3f})"
    print(f"{tag}: forward + backward fused {q(ts[True])}, composed {q(ts[False])}, composed / fused {m_c / m_f:.2f}")
    total_ms = total_bytes = 0.0
    for line in buf.value.decode().splitlines():
        w = line.split()
        if w[0] in kernels:
            ms, nbytes = float(w[2]) / int(w[1]), float(w[4])
            total_ms, total_bytes = total_ms + ms, total_bytes + nbytes
            print(f"{tag}: {w[0]} {ms:.3f} ms per launch, perfect gather {nbytes / 1e6:.1f} MB = {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s")
    print(f"{tag}: its kernels {total_ms:.3f} ms, {total_bytes / 1e6:.1f} MB = {total_bytes / (total_ms * 1e-3) / 1e12:.2f} TB/s; "
          f"over the whole step (loss included) {total_bytes / m_f / 1e12:.2f} TB/s fused, {total_bytes / m_c / 1e12:.2f} TB/s composed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    i, j = edges()
    e = i.shape[0]
    deg = np.bincount(j, minlength=N) + np.bincount(i, minlength=N)
    print(f"N {N} E {e}: edges per node median {int(np.median(deg))} max {int(deg.max())}, nodes above {G.mpnnLongRow()}: {int((deg > G.mpnnLongRow()).sum())}")
    si, sj = S.STen.from_numpy(i), S.STen.from_numpy(j)
    t0 = time.perf_counter()
    csr = G.computeEdgeCsr(si, sj, N)
    lib.lamp_device_synchronize()
    print(f"edge CSR, both groupings (range check, sort, bincount, prefix sum each): {1e3 * (time.perf_counter() - t0):.2f} ms, once per graph")
    cache = {}
    for d in (64, 128):
        x, ef, lf = S.STen.randn([N, d]), S.STen.randn([e, FE]), A.const(S.STen.randn([e, FE + 2 * d]))
        measure(f"message Fe {FE} D {d}", lambda fused: message_step(x, ef, lf, si, sj, csr, fused),
                ("mpnn_message", "mpnn_message_backward_x", "mpnn_message_backward_edge"), a.reps, a.windows)
        del x, ef, lf
    for m in (64, 128):
        msg, lf = S.STen.randn([e, m]), A.const(S.STen.randn([N, m]))
        measure(f"aggregate M {m}", lambda fused: aggregate_step(msg, lf, si, sj, csr, cache, fused), ("mpnn_aggregate", "mpnn_aggregate_backward"), a.reps, a.windows)
        del msg, lf


if __name__ == "__main__":
    main()
