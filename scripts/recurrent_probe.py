#!/usr/bin/env python3
"""One training step of example-timemachine's model at the example's size, fused nodes vs the composed chain.

Embedding(V = 128, 20) -> LSTM(20 -> 1024) -> relu -> SeqLinear(1024 -> V) -> logSoftMax, SequenceNLL, AdamW(clip = 1), B = 256, T = 100,
f32 and f64.  The two forms alternate in windows inside one process (lamp_recurrent_fused); per form: median ms / step over the windows,
their spread (min .. max), tokens / s, and the per-class kernel timer table of one extra step.

Usage: python scripts/recurrent_probe.py [--windows 5] [--steps 3] [--T 100] [--B 256] [--H 1024] [--dtypes f32,f64]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lamp_amd._capi import lib  # noqa: E402
lib.load()
import numpy as np  # noqa: E402
from lamp_amd import nn, recurrent as RC, sten as S, transformer as TF  # noqa: E402


def class_table():
    buf = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_report(buf, len(buf))
    rows = [l.split() for l in buf.value.decode().splitlines()]
    return sorted(((r[0], int(r[1]), float(r[2])) for r in rows), key=lambda r: -r[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5); ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--T", type=int, default=100); ap.add_argument("--B", type=int, default=256); ap.add_argument("--H", type=int, default=1024)
    ap.add_argument("--V", type=int, default=128); ap.add_argument("--dtypes", default="f32,f64")
    a = ap.parse_args()
    for name in a.dtypes.split(","):
        dt = {"f32": S.F32, "f64": S.F64}[name]
        m = RC.statefulSequence(TF.Embedding(a.V, 20, dt), RC.LSTM(20, a.H, dt), nn.Fun("relu"), RC.SeqLinear(a.H, a.V, dt), nn.Fun("logsoftmax", 2))
        model = nn.SupervisedModel(m, RC.SEQUENCE_NLL, S.STen.from_numpy(np.ones(a.V, dtype=np.float32 if name == "f32" else np.float64)))
        opt = nn.AdamW([p.value for p in m.parameters], weightDecay=0.0, learningRate=1e-4, clip=1.0)
        tok = S.STen.from_numpy(((np.arange(a.T * a.B).reshape(a.T, a.B) * 7 + 3) % a.V).astype(np.int64))
        tgt = S.STen.from_numpy(((np.arange(a.T * a.B).reshape(a.T, a.B) * 11 + 5) % a.V).astype(np.int64))
        times = {True: [], False: []}
        for fused in (True, False):                      # warm-up of both forms
            RC.recurrentFused(fused); model.train_step(opt, tok, tgt); lib.lamp_device_synchronize()
        for _ in range(a.windows):
            for fused in (True, False):
                RC.recurrentFused(fused)
                lib.lamp_device_synchronize(); t0 = time.perf_counter()
                for _ in range(a.steps):
                    model.train_step(opt, tok, tgt)
                lib.lamp_device_synchronize()
                times[fused].append((time.perf_counter() - t0) * 1e3 / a.steps)
        for fused in (True, False):
            ts = times[fused]; med = statistics.median(ts)
            print(f"{name} {'fused   ' if fused else 'composed'} median {med:9.2f} ms/step  windows min {min(ts):9.2f} max {max(ts):9.2f}  "
                  f"{a.T * a.B / med * 1e3:12.0f} tokens/s")
        print(f"{name} ratio composed / fused = {statistics.median(times[False]) / statistics.median(times[True]):.2f}")
        for fused in (True, False):
            RC.recurrentFused(fused); class_table(); lib.lamp_kernel_timer_enable(1)
            model.train_step(opt, tok, tgt); lib.lamp_device_synchronize(); lib.lamp_kernel_timer_enable(0)
            print(f"{name} {'fused' if fused else 'composed'}: kernel classes of one step (launches, ms)")
            for tag, n, ms in class_table():
                print(f"    {tag:28s} {n:6d} {ms:10.3f}")
        RC.recurrentFused(True)


if __name__ == "__main__":
    main()
