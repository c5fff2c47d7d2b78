#!/usr/bin/env python3
"""BERT's input embedding, forward + backward: the fused BertEmbedding node (csrc/kernels/bert.hip) against the reference's chain of
Embedding, Embedding, Add, Slice and Add nodes, and a full BertLoss training step with either.

Shapes: BERT-base's (B 64, T 512, D 768, V 30522, Vs 2; f32 and bf16) and example-bert's own (T 32, D 32, V 4000, a batch of 64; f32).
Tokens follow a Zipf-like law over the vocabulary (a few ids thousands of times, most never) with a quarter of every sequence padding
(id 0), segments are 0 then 1.  Both forms alternate inside one process, after a warm-up of each; every repetition is
(node(...) * l).sum().backprop() with the three tables as parameters and ends in a device synchronise; medians are reported.  The
kernel timer then gives each form's own kernels: launches and device time per repetition.  The composed chain is the code every earlier
revision runs for these nodes, so its column is also the number to hold a later revision against.

    python scripts/bert_probe.py [--reps 30] [--windows 5]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lamp_amd import autograd as A, bert as B, nn, sten as S   # noqa: E402
from lamp_amd._capi import lib                               # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        lib.lamp_device_synchronize()
        t0 = time.perf_counter()
        fn()
        lib.lamp_device_synchronize()
        out.append(time.perf_counter() - t0)
    return out


def ids(b, t, v, rng):
    ranks = np.arange(1, v, dtype=np.float64)
    p = 1.0 / ranks
    tokens = rng.choice(np.arange(1, v), size=(b, t), p=p / p.sum()).astype(np.int64)
    tokens[:, t - t // 4:] = 0
    segments = np.zeros((b, t), dtype=np.int64)
    segments[:, t // 3:t - t // 4] = 1
    return tokens, segments


def kernel_report(run, reps):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.lamp_device_synchronize()
    lib.lamp_kernel_timer_report(buf, len(buf))       # clears the log
    lib.lamp_kernel_timer_enable(1)
    for _ in range(reps):
        run()
    lib.lamp_device_synchronize()
    lib.lamp_kernel_timer_enable(0)
    lib.lamp_kernel_timer_report(buf, len(buf))
    rows = []
    for line in buf.value.decode().splitlines():
        w = line.split()
        rows.append((w[0], int(w[1]) / reps, float(w[2]) / reps))
    return rows


def q(t):
    return f"{1e3 * statistics.median(t):.3f} ms (min {1e3 * min(t):.3f}, p90 {1e3 * sorted(t)[int(0.9 * len(t))]:.3f})"


def measure(tag, run, reps, windows, kernels=True):
    for fused in (True, False):                       # warm-up of both forms
        for _ in range(3):
            run(fused)
    ts = {True: [], False: []}
    for _ in range(windows):                          # alternate
        for fused in (True, False):
            ts[fused] += timed(lambda: run(fused), reps)
    m_f, m_c = statistics.median(ts[True]), statistics.median(ts[False])
    print(f"{tag}: fused {q(ts[True])}, composed {q(ts[False])}, composed / fused {m_c / m_f:.2f}")
    if kernels:
        for fused in (True, False):
            rows = kernel_report(lambda: run(fused), reps)
            total = sum(r[2] for r in rows)
            print(f"{tag}: {'fused' if fused else 'composed'} kernels per repetition: {sum(r[1] for r in rows):.0f} launches, {total:.3f} ms: "
                  + ", ".join(f"{n} {c:g} x {ms / max(c, 1e-9):.4f}" for n, c, ms in sorted(rows, key=lambda r: -r[2])[:8]))
    return m_f, m_c


def embedding_probe(b, t, d, v, vs, dtype, name, reps, windows, rng):
    tokens, segments = ids(b, t, v, rng)
    counts = np.bincount(tokens.reshape(-1), minlength=v)[1:]
    print(f"{name}: B {b} T {t} D {d} V {v} Vs {vs}: {int((counts > 0).sum())} ids occur, {int((counts > B.bertLongRow()).sum())} more than "
          f"{B.bertLongRow()} times (max {int(counts.max())}), {int((tokens == 0).sum())} padding positions")
    tw, sw, pe = (S.STen.randn([v, d]).castToType(dtype), S.STen.randn([vs, d]).castToType(dtype), S.STen.randn([1, t, d]).castToType(dtype))
    lf = A.const(S.STen.randn([b, t, d]).castToType(dtype))
    tk, sg = A.const(S.STen.from_numpy(tokens)), A.const(S.STen.from_numpy(segments))
    res = {}

    def run(fused):
        prev = B.bertFused(fused)
        try:
            p = [A.param(x) for x in (tw, sw, pe)]
            (B.bertEmbedding(tk, sg, *p) * lf).sum().backprop()
            res[fused] = [x.partialDerivative for x in p]
        finally:
            B.bertFused(prev)

    def forward(fused):
        prev = B.bertFused(fused)
        try:
            B.bertEmbedding(tk, sg, A.const(tw), A.const(sw), A.const(pe))
        finally:
            B.bertFused(prev)

    run(True); run(False)
    for key, f, c in zip(("dToken", "dSegment", "dPositional"), res[True], res[False]):
        x, y = f.castToType(S.F64).to_numpy(), c.castToType(S.F64).to_numpy()
        print(f"{name}: {key} fused vs composed max |diff| {np.abs(x - y).max():.3e} of max {np.abs(y).max():.3e}")
    measure(f"{name} forward", forward, reps, windows, kernels=False)
    return measure(f"{name} forward + backward", run, reps, windows)


def loss_probe(reps, windows, rng):
    """example-bert's configuration: maxLength 32, width 32, four heads, two blocks, a vocabulary of 4000"""
    maxlen, vocab, batch = 32, 4000, 64
    tokens, segments = ids(batch, maxlen, vocab, rng)
    npos = int(maxlen * 0.15)
    m = B.BertLoss(maxlen, vocab, 2, 32, 32, 2, 32, 8, 4, 128, 0.0, 0, S.F32, 0, False)
    opt = nn.AdamW([p.value for p in m.parameters], weightDecay=0.0, learningRate=1e-4)
    tk, sg = A.const(S.STen.from_numpy(tokens)), A.const(S.STen.from_numpy(segments))
    pos = S.STen.from_numpy(rng.integers(1, maxlen - maxlen // 4, size=(batch, npos)).astype(np.int64))
    target = S.STen.from_numpy(rng.integers(4, vocab, size=(batch, npos)).astype(np.int64))
    lengths = S.STen.from_numpy(np.full(batch, maxlen - maxlen // 4, dtype=np.int64))
    whole = S.STen.from_numpy(rng.integers(0, 2, size=batch).astype(np.float32))

    def run(fused):
        prev = B.bertFused(fused)
        try:
            opt.step(m.gradients(m.forward(tk, sg, pos, lengths, target, whole)))
        finally:
            B.bertFused(prev)
    return measure(f"BertLoss step (maxLength {maxlen}, D 32, V {vocab}, batch {batch})", run, reps, windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    pairs = []
    pairs.append(embedding_probe(64, 512, 768, 30522, 2, S.F32, "base f32", a.reps, a.windows, rng))
    pairs.append(embedding_probe(64, 512, 768, 30522, 2, S.BF16, "base bf16", a.reps, a.windows, rng))
    pairs.append(embedding_probe(64, 32, 32, 4000, 2, S.F32, "example f32", a.reps, a.windows, rng))
    loss_probe(a.reps, a.windows, rng)
    verdict = all(f <= c for f, c in pairs)
    print(f"fused no slower than composed at every embedding shape: {verdict}")


if __name__ == "__main__":
    main()
