#!/usr/bin/env python3
"""Conv1D / Conv2DTransposed layers, forward, input gradient and weight gradient: the general matrix-core kernels (kernels/conv_gen.hip)
against the direct kernels, the two arms of lamp_convolution_matrix_path.  With the switch off the direct arm is what every earlier
revision runs for these layers, so its column is also the number to hold a later revision against.

Shapes (typical users of the modules; the reference has no example that uses them), each in bf16 and f32:
    conv1d-tcn     Conv1D           64 x 256 -> 256 x L 4096, k 3, dilation 2, padding 2
    conv1d-k5      Conv1D           128 x 300 -> 128 x L 512, k 5, padding 2
    convT-128      Conv2DTransposed 64 x 256 -> 128, 16^2 -> 32^2, k 4, stride 2, padding 1
    convT-rgb      Conv2DTransposed 256 x 64 -> 3, 16^2 -> 32^2, k 4, stride 2, padding 1

Every (shape, dtype, pass) is timed in a process of its own under its own time limit (--limit seconds; the direct weight gradient at
these sizes may need seconds per launch); the first one that fails or runs out of time ends the probe.  Inside it the two arms
alternate, after a warm-up of each; a repetition is one C-ABI call, and its time is the device time of the conv_* kernel classes it
launched, from the kernel timer's HIP events.  Reported: median, min .. max (the spread), TFLOP/s from conv_flops, and the share of the
bounding peak: min(matrix peak, arithmetic intensity x HBM bandwidth) with 2516.8 TF bf16, 157.3 TF f32 and 8 TB/s.

    python scripts/conv_modules_probe.py [--reps 7] [--limit 120]
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (transposed, N, C_x, spatial, C_y, k, stride, padding, dilation)
SHAPES = {
    "conv1d-tcn": (False, 64, 256, (4096,), 256, 3, 1, 2, 2),
    "conv1d-k5": (False, 128, 300, (512,), 128, 5, 1, 2, 1),
    "convT-128": (True, 64, 256, (16, 16), 128, 4, 2, 1, 1),
    "convT-rgb": (True, 256, 64, (16, 16), 3, 4, 2, 1, 1),
}
PASSES = ("forward", "dgrad", "wgrad")
PEAK_TF = {"bf16": 2516.8, "f32": 157.3}
HBM_TBS = 8.0


def child(shape, dtn, pass_, reps):
    from lamp_amd import nn, sten as S
    from lamp_amd._capi import lib, i64_array
    transposed, N, cx, spatial, cy, k, s, p, d = SHAPES[shape]
    n = len(spatial)
    dt = S.BF16 if dtn == "bf16" else S.F32
    lib.lamp_manual_seed(11)
    x = S.STen.randn([N, cx, *spatial]).castToType(dt)
    w = (S.STen.randn([cx, cy] + [k] * n if transposed else [cy, cx] + [k] * n) * 0.05).castToType(dt)
    b = S.STen.randn([cy]).castToType(dt)
    geo = (i64_array([s] * n), i64_array([p] * n), i64_array([d] * n))
    zero = i64_array([0] * n)
    o = C.c_void_p()
    lib.lamp_convolution(C.byref(o), x, w, b, *geo, n, int(transposed), zero, 1)
    y = S.STen(o)
    gy = S.STen.randn(y.shape).castToType(dt)
    mask = (C.c_uint8 * 3)(int(pass_ == "dgrad"), int(pass_ == "wgrad"), 0)
    buf = C.create_string_buffer(1 << 16)

    def call():
        if pass_ == "forward":
            r = C.c_void_p()
            lib.lamp_convolution(C.byref(r), x, w, b, *geo, n, int(transposed), zero, 1)
            return S.STen(r)
        out = (C.c_void_p * 3)()
        lib.lamp_convolution_backward(out, gy, x, w, *geo, n, int(transposed), zero, 1, mask)
        return [S.STen(h) for h in out if h]

    def once(on):
        """(device ms of the conv_* classes, flops, bytes, classes) of one call with the switch set to `on`"""
        prev = nn.convolutionMatrixPath(on)
        try:
            lib.lamp_device_synchronize()
            lib.lamp_kernel_timer_report(buf, len(buf))      # clears the log
            lib.lamp_kernel_timer_enable(1)
            call()
            lib.lamp_device_synchronize()
            lib.lamp_kernel_timer_enable(0)
            lib.lamp_kernel_timer_report(buf, len(buf))
        finally:
            nn.convolutionMatrixPath(prev)
        rows = [ln.split() for ln in buf.value.decode().splitlines() if ln.startswith("conv_")]
        main = max(rows, key=lambda r: float(r[3]))
        return sum(float(r[2]) for r in rows), float(main[3]), float(main[4]), "+".join(r[0] for r in rows)

    for on in (True, False):
        for _ in range(2):
            once(on)
    ms = {True: [], False: []}
    info = {}
    for _ in range(reps):
        for on in (True, False):
            t, flops, nbytes, classes = once(on)
            ms[on].append(t)
            info[on] = (flops, nbytes, classes)
    for on in (True, False):
        flops, nbytes, classes = info[on]
        med = statistics.median(ms[on])
        tf = flops / (med * 1e-3) / 1e12
        bound = min(PEAK_TF[dtn], flops / nbytes * HBM_TBS)
        print(f"{shape} {dtn} {pass_} {'matrix' if on else 'direct'}: median {med:.4f} ms (min {min(ms[on]):.4f} .. max {max(ms[on]):.4f}), "
              f"{tf:.2f} TFLOP/s, {100 * tf / bound:.1f} % of the bounding {bound:.0f} TF [{classes}]")
    m, dct = statistics.median(ms[True]), statistics.median(ms[False])
    spread = max(max(v) - min(v) for v in ms.values())
    verdict = "ok" if m <= dct + spread else "SLOWER"
    print(f"{shape} {dtn} {pass_}: direct / matrix {dct / m:.2f}, spread {spread:.4f} ms: {verdict}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds for one (shape, dtype, pass)")
    ap.add_argument("--child", nargs=3, metavar=("SHAPE", "DTYPE", "PASS"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.child[2], a.reps)
        return 0
    for shape in SHAPES:
        for dtn in ("bf16", "f32"):
            for pass_ in PASSES:
                cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", shape, dtn, pass_]
                try:
                    r = subprocess.run(cmd, timeout=a.limit)
                except subprocess.TimeoutExpired:
                    print(f"{shape} {dtn} {pass_}: no result within {a.limit:g} s - stopping here", flush=True)
                    return 124
                if r.returncode != 0:
                    print(f"{shape} {dtn} {pass_}: exit status {r.returncode} - stopping here", flush=True)
                    return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
