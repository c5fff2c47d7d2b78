#!/usr/bin/env python3
"""Minibatches of small graphs at a size a user would run: 4096 graphs of 10 - 40 nodes (about 2.2 edges per node), F = 64, f32,
minibatch 128.  Measures one epoch of batches alone (batches / s) and a training step of two gcn layers + VertexPooling(Mean) + Linear
+ logSoftMax + NLL + AdamW per batch, with graphBatchFused on (the collate kernels, the batch's groupings carried along, SegmentPool)
and off (the reference's fold out of existing operators, groupings sorted per batch, the composed VertexPooling).

Both forms alternate inside one process, after a warm-up of each; every window ends in a device synchronise; medians are reported.  The
launch counts per batch come from the kernel timer.

    python scripts/graph_batch_probe.py [--graphs 4096] [--windows 5]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lamp_amd import graph as G, nn, sten as S                                        # noqa: E402
from lamp_amd._capi import lib                                                         # noqa: E402
from lamp_amd.data import JavaRandom                                                   # noqa: E402
from lamp_amd.graphbatch import GraphBatchStream, GraphSet, graphBatchFused            # noqa: E402

F, MB = 64, 128


def graphs(count, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(10, 41))
        e = int(2.2 * n)
        i = rng.integers(0, n, e)
        j = (i + 1 + rng.integers(0, n - 1, e)) % n
        out.append(GraphBatchStream.Graph(S.STen.from_numpy(rng.standard_normal((n, F)).astype(np.float32)), S.STen.from_numpy(np.ones(e, dtype=np.float32)),
                                          S.STen.from_numpy(i.astype(np.int64)), S.STen.from_numpy(j.astype(np.int64))))
    return out


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
    ap.add_argument("--graphs", type=int, default=4096)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    graphSet = GraphSet(graphs(a.graphs))
    target = S.STen.from_numpy((np.arange(a.graphs) % 2).astype(np.int64))
    print(f"{a.graphs} graphs, {graphSet.numNodes} nodes, {graphSet.numEdges} edges, F {F}, minibatch {MB}")
    t0 = time.perf_counter()
    graphSet.adjacency(), graphSet.edgeCsr()
    lib.lamp_device_synchronize()
    print(f"set-wide groupings (three range checks, sorts, bincounts, prefix sums): {1e3 * (time.perf_counter() - t0):.2f} ms, once per data set")
    stream = GraphBatchStream.smallGraphStream(MB, graphSet, target, JavaRandom(1), groupings=("adjacency",))
    layers, head = [G.gcn(F, F, S.F32, 0), G.gcn(F, F, S.F32, 0)], nn.Linear(F, 2, S.F32, 0)
    params = [p for m in layers + [head] for p in m.parameters]
    opt = nn.AdamW([p.value for p in params], 0.0, 1e-3)
    weights = S.STen.ones([2], S.F32)

    def batches():
        stream.reset()
        for _ in stream:
            pass

    def train():
        stream.reset()
        for g, t in stream:
            for m in layers + [head]:
                m.zeroGrad()
            for layer in layers:
                g = layer.forward(g)
            loss = head.forward(G.VertexPooling(g, "Mean")).logSoftMax(1).nllLoss(t, weights)
            loss.backprop()
            opt.step([p.partialDerivative for p in params])

    def epoch(fn, fused):
        prev = graphBatchFused(fused)
        try:
            lib.lamp_device_synchronize()
            t0 = time.perf_counter()
            fn()
            lib.lamp_device_synchronize()
            return time.perf_counter() - t0
        finally:
            graphBatchFused(prev)

    nb = stream.numBatches
    for name, fn in (("batches alone", batches), ("training step", train)):
        for fused in (True, False):                       # warm-up of both forms
            epoch(fn, fused)
        ts = {True: [], False: []}
        for _ in range(a.windows):                        # alternate
            for fused in (True, False):
                ts[fused].append(epoch(fn, fused) / nb)
        m_f, m_c = statistics.median(ts[True]), statistics.median(ts[False])
        q = lambda v: f"{1e3 * statistics.median(v):.3f} ms per batch (min {1e3 * min(v):.3f}, max {1e3 * max(v):.3f}) = {1.0 / statistics.median(v):.0f} batches/s"
        print(f"{name}: fused {q(ts[True])}; chain {q(ts[False])}; chain / fused {m_c / m_f:.2f}")
        for fused in (True, False):
            prev = graphBatchFused(fused)
            try:
                counts = timer_counts(fn)
            finally:
                graphBatchFused(prev)
            print(f"{name}, {'fused' if fused else 'chain'}: {sum(counts.values()) / nb:.1f} launches per batch; "
                  + ", ".join(f"{k} {v / nb:.1f}" for k, v in sorted(counts.items(), key=lambda kv: -kv[1])[:8]))


if __name__ == "__main__":
    main()
