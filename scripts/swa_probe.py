#!/usr/bin/env python3
"""The three whole-state operations of the training drivers (loops.epochs / swaEpochs) at the sizes they run at: the snapshot, the
running mean of the weight average and Module.load on the CIFAR ResNet's 74 state tensors (f32 and bf16) and on a language model's
state (12 blocks of width 768, bf16), with stateKernelsFused on (one multi-tensor launch per 40 tensors per dtype) and off (the
reference's per-tensor clone, three-operator chain and copyFrom).

Both forms alternate inside one process, after a warm-up of each; a window is `--reps` operations back to back and ends in a device
synchronise, so it holds the launches and their host cost, which is what an epoch pays; medians over the windows are reported, with
the extremes.  The launch counts come from the kernel timer, which sees kernels only: the per-tensor copies of the unfused snapshot and
load are hipMemcpyAsync calls and count as 0 there.  A ratio printed here is a figure against the chain at the same commit, not a gate.

    python scripts/swa_probe.py [--windows 7] [--reps 200]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lamp_amd import nn, sten as S, transformer as TR                                # noqa: E402
from lamp_amd._capi import lib                                                        # noqa: E402


def timer_counts(fn):
    lib.lamp_device_synchronize()
    buf = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_report(buf, len(buf))
    lib.lamp_kernel_timer_enable(1)
    fn()
    lib.lamp_device_synchronize()
    lib.lamp_kernel_timer_enable(0)
    lib.lamp_kernel_timer_report(buf, len(buf))
    return {l.split()[0]: int(l.split()[1]) for l in buf.value.decode().splitlines()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    n = C.c_int(0); lib.lamp_has_gpu(C.byref(n))
    if n.value != 1:
        raise SystemExit("swa_probe: no MI355X visible; nothing is measured without the GPU")
    models = [("resnet f32", lambda: nn.resnet(100, 0.0, S.F32, 0)), ("resnet bf16", lambda: nn.resnet(100, 0.0, S.BF16, 0)),
              ("language model bf16", lambda: TR.LanguageModelModule(384, 256, 12, 768, 64, 12, 3072, 0.0, S.BF16, 0))]
    for name, make in models:
        module = make()
        state = [v.value for v in module.state]
        nbytes = sum(t.numel * {S.F32: 4, S.F64: 8, S.BF16: 2, S.F16: 2}[t.dtype] for t in state)
        print(f"{name}: {len(state)} state tensors, {nbytes / 1e6:.2f} MB")
        held = {}

        def snapshot():
            held["avg"] = nn.stateSnapshot(state)

        def average():
            held["avg"] = nn.swaAverage(held["avg"], state, 3)

        def load():
            module.load(held["avg"])

        def window(fn, fused):
            prev = nn.stateKernelsFused(fused)
            try:
                lib.lamp_device_synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    fn()
                lib.lamp_device_synchronize()
                return (time.perf_counter() - t0) / a.reps
            finally:
                nn.stateKernelsFused(prev)

        for what, fn in (("snapshot", snapshot), ("average", average), ("load", load)):
            for fused in (True, False):                       # warm-up of both forms
                window(fn, fused)
            ts = {True: [], False: []}
            for _ in range(a.windows):                        # alternate
                for fused in (True, False):
                    ts[fused].append(window(fn, fused))
            counts = {}
            for fused in (True, False):
                prev = nn.stateKernelsFused(fused)
                try:
                    counts[fused] = timer_counts(fn)
                finally:
                    nn.stateKernelsFused(prev)
            q = lambda v: f"{1e6 * statistics.median(v):.1f} us (min {1e6 * min(v):.1f}, max {1e6 * max(v):.1f})"
            print(f"  {what}: fused {q(ts[True])}, {sum(counts[True].values())} launches {counts[True]}; chain {q(ts[False])}, "
                  f"{sum(counts[False].values())} timed launches {counts[False]}; chain / fused {statistics.median(ts[False]) / statistics.median(ts[True]):.2f}")


if __name__ == "__main__":
    main()
