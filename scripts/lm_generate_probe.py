#!/usr/bin/env python3
"""Generation speed of the example-autoregressivelm model: decode kernels against the reference's chain.

The model of the example: 12 blocks x 768 x 12 heads, context 384, vocabulary 256, bf16, random weights (speed does not depend on them).
For B in {1, 16}: a prefix of 32 tokens, 256 generated tokens, so every token after the first is a cached step.  Per configuration one
warm-up generation, then `--reps` timed generations of each path, alternating fused / chain, a host clock around one generation that
ends in one device synchronisation; the median is reported with the spread.  The launches per token come from a generation of their own
under the kernel timer (tagged launches only; the timer slows the host, so that run is not timed).  One JSON line per configuration.

Usage: python scripts/lm_generate_probe.py [--reps 5] [--length 256] [--prefix 32] [--batches 1,16] [--out FILE]
Needs an MI355X: there is no CPU path.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def launches(lib):
    buf = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_report(buf, len(buf))
    return {l.split()[0]: int(l.split()[1]) for l in buf.value.decode().splitlines() if l.strip()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--length", type=int, default=256)
    ap.add_argument("--prefix", type=int, default=32)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--context", type=int, default=384)
    ap.add_argument("--vocabulary", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    from lamp_amd._capi import lib
    lib.load()
    n = C.c_int(0); lib.lamp_has_gpu(C.byref(n))
    if n.value != 1:
        raise SystemExit("lm_generate_probe: no MI355X visible; generation has no CPU path and nothing is measured without the GPU")
    import numpy as np
    from lamp_amd import sten as S, transformer as TR, languagemodel as L

    model = TR.LanguageModelModule(a.context, a.vocabulary, a.blocks, a.dim, a.dim // a.heads, a.heads, 4 * a.dim, 0.0, S.BF16, 0)
    weight_bytes = sum(int(np.prod(v.value.shape)) for v in model.state) * 2
    lines = []
    for B in [int(b) for b in a.batches.split(",")]:
        prefix = ((np.arange(B * a.prefix).reshape(B, a.prefix) * 7 + 3) % a.vocabulary).astype(np.int64)

        def generate(fused):
            L.languageModelFused(fused)
            L.manualSeed(1)
            t0 = time.perf_counter()
            out = L.autoregressiveInference(model, a.context, S.STen.from_numpy(prefix), a.length, 1.0)
            S.synchronize()
            dt = time.perf_counter() - t0
            assert L.languageModelGeneratePath() == ("fused" if fused else "chain")
            return dt, out

        times = {True: [], False: []}
        for fused in (True, False):
            generate(fused)                                   # warm-up: code objects, allocator, packed weights
        for _ in range(a.reps):
            for fused in (True, False):
                times[fused].append(generate(fused)[0])
        per_token = {}
        lib.lamp_kernel_timer_enable(1)
        for fused in (True, False):
            launches(lib)
            generate(fused)
            per_token[fused] = sum(launches(lib).values()) / a.length
        lib.lamp_kernel_timer_enable(0)
        L.languageModelFused(True)
        med = {f: statistics.median(times[f]) for f in times}
        line = {"B": B, "prefix": a.prefix, "length": a.length, "reps": a.reps, "blocks": a.blocks, "dim": a.dim, "heads": a.heads, "context": a.context,
                "vocabulary": a.vocabulary, "dtype": "bf16", "weight_bytes": weight_bytes,
                "fused_tokens_per_s": B * a.length / med[True], "chain_tokens_per_s": B * a.length / med[False],
                "fused_us_per_step": 1e6 * med[True] / a.length, "chain_us_per_step": 1e6 * med[False] / a.length,
                "fused_s_min_max": [min(times[True]), max(times[True])], "chain_s_min_max": [min(times[False]), max(times[False])],
                "fused_tagged_launches_per_token": per_token[True], "chain_tagged_launches_per_token": per_token[False],
                "fused_not_slower": med[True] <= med[False]}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
