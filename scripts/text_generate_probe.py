#!/usr/bin/env python3
"""Generation speed of the example-timemachine model: the recurrent decode kernels against the reference's chain.

The model of the example: Embedding(vocabulary 50, 20) -> cell(20, hidden) -> relu -> SeqLinear(hidden, 50) -> logSoftMax, f32, random weights
(speed does not depend on them).  For cell in {lstm, gru, rnn} x hidden in {256, 1024} x B in {1, 16}: a prefix of 20 tokens, `--steps`
generated tokens through sequencePrediction.  Per configuration one warm-up generation of each path, then `--reps` timed generations,
alternating fused / chain, a host clock around one generation that ends in one device synchronisation; the median is reported with the
spread.  The launches per token come from a generation of their own under the kernel timer (tagged launches only; not timed).  Beam: k = 3,
the same model at B = 1, steps per second.  One JSON line per configuration.

Usage: python scripts/text_generate_probe.py [--reps 5] [--steps 128] [--hidden 256,1024] [--batches 1,16] [--out FILE]
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
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--prefix", type=int, default=20)
    ap.add_argument("--hidden", default="256,1024")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--cells", default="lstm,gru,rnn")
    ap.add_argument("--vocabulary", type=int, default=50)
    ap.add_argument("--embedding", type=int, default=20)
    ap.add_argument("--beam-steps", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    from lamp_amd._capi import lib
    lib.load()
    n = C.c_int(0); lib.lamp_has_gpu(C.byref(n))
    if n.value != 1:
        raise SystemExit("text_generate_probe: no MI355X visible; generation has no CPU path and nothing is measured without the GPU")
    import numpy as np
    from lamp_amd import nn, recurrent as RC, sten as S, text as TX, transformer as TF

    cells = {"lstm": RC.LSTM, "gru": RC.GRU, "rnn": RC.RNN}
    V, E = a.vocabulary, a.embedding
    lines = []

    def timed(run, path):
        t0 = time.perf_counter()
        run()
        S.synchronize()
        dt = time.perf_counter() - t0
        assert TX.textGeneratePath() == path
        return dt

    def measure(run, count):
        """median seconds of each path, tagged launches per `count`"""
        times = {True: [], False: []}
        for fused in (True, False):
            TX.textGenerationFused(fused); timed(run, "fused" if fused else "chain")           # warm-up: code objects, allocator
        for _ in range(a.reps):
            for fused in (True, False):
                TX.textGenerationFused(fused); times[fused].append(timed(run, "fused" if fused else "chain"))
        per = {}
        lib.lamp_kernel_timer_enable(1)
        for fused in (True, False):
            TX.textGenerationFused(fused); launches(lib); timed(run, "fused" if fused else "chain")
            per[fused] = sum(launches(lib).values()) / count
        lib.lamp_kernel_timer_enable(0)
        TX.textGenerationFused(True)
        return times, per

    for cell in a.cells.split(","):
        for H in [int(h) for h in a.hidden.split(",")]:
            model = RC.statefulSequence(TF.Embedding(V, E, S.F32, 0), cells[cell](E, H, S.F32, 0), nn.Fun("relu"), RC.SeqLinear(H, V, S.F32, 0),
                                        nn.Fun("logsoftmax", 2))
            for B in [int(b) for b in a.batches.split(",")]:
                prefix = S.STen.from_numpy(((np.arange(a.prefix * B).reshape(a.prefix, B) * 7 + 3) % V).astype(np.int64))
                times, per = measure(lambda: TX.sequencePrediction(prefix, 0, model, a.steps), a.steps)
                med = {f: statistics.median(times[f]) for f in times}
                line = {"what": "sequencePrediction", "cell": cell, "hidden": H, "B": B, "prefix": a.prefix, "steps": a.steps, "reps": a.reps,
                        "vocabulary": V, "embedding": E, "dtype": "f32",
                        "fused_tokens_per_s": B * a.steps / med[True], "chain_tokens_per_s": B * a.steps / med[False],
                        "fused_us_per_step": 1e6 * med[True] / a.steps, "chain_us_per_step": 1e6 * med[False] / a.steps,
                        "fused_s_min_max": [min(times[True]), max(times[True])], "chain_s_min_max": [min(times[False]), max(times[False])],
                        "fused_tagged_launches_per_token": per[True], "chain_tagged_launches_per_token": per[False],
                        "fused_not_slower": med[True] <= med[False]}
                print(json.dumps(line), flush=True)
                lines.append(line)
            first = [int(v) for v in (np.arange(a.prefix) * 7 + 3) % V]
            times, per = measure(lambda: TX.sequencePredictionBeam(first, 0, model, a.beam_steps, -1, -2, 3), a.beam_steps)
            med = {f: statistics.median(times[f]) for f in times}
            line = {"what": "sequencePredictionBeam", "cell": cell, "hidden": H, "k": 3, "prefix": a.prefix, "steps": a.beam_steps, "reps": a.reps,
                    "dtype": "f32", "fused_steps_per_s": a.beam_steps / med[True], "chain_steps_per_s": a.beam_steps / med[False],
                    "fused_s_min_max": [min(times[True]), max(times[True])], "chain_s_min_max": [min(times[False]), max(times[False])],
                    "fused_tagged_launches_per_step": per[True], "chain_tagged_launches_per_step": per[False],
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
