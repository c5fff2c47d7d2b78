"""lamp.data.GraphBatchStream over the C ABI: minibatches of many small graphs with one target per graph, as block-diagonal
lamp_amd.graph.Graph values.

Reference: lamp-data/src/main/scala/lamp/data/GraphBatchStream.scala.  Its smallGraphStream folds the graphs of a batch together with
four element-wise launches per graph and five cats, and hands the layers a fresh Graph, whose groupings (Graph.adjacency(),
Graph.edgeCsr()) every batch then sorts anew with three host synchronisations.  A batch of whole graphs is block-diagonal, so none of
that is needed: `GraphSet` packs the data set once (all node rows, all edge rows, endpoints with set-wide ids, `nodePtr` / `edgePtr`)
and groups it once; graph g's entries of the set-wide groupings are contiguous and already in the order a grouping of any batch would
give them.  `graphBatchPlan` computes, on the host and once per epoch, where every graph's rows come from and go to; a batch is then
two ragged row copies (`lamp_graph_batch_rows`), at most two launches for every integer array (`lamp_graph_batch_nodes`,
`lamp_graph_batch_edges`) and one gather of the targets, with no sort, no host read and no atomics, and the batch Graph's caches are
filled, so stacked layers build nothing.  Its `graphPtr` lets VertexPooling sum consecutive rows (the SegmentPool node).

`graph.graphBatchFused(False)` is the reference's fold out of existing operators, a Graph with empty caches and the composed
VertexPooling: the fallback for other types than f32 / f64 and the yardstick of scripts/graph_batch_probe.py.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

from ._capi import lib
from .autograd import const
from . import graph as G
from .graph import graphBatchFused  # noqa: F401  (the switch lives beside VertexPooling, which reads it)
from .sten import STen, F32, F64, I64

GraphBatchPlan = namedtuple("GraphBatchPlan", ["table", "offsets", "totals"])
GraphBatchPlan.__doc__ = """table int64 [len(order), 4]: per graph of the epoch, in the epoch's order, (srcNodeBase, dstNodeBase, srcEdgeBase, dstEdgeBase):
the first row of its nodes / edges in the packed set and in its batch.  offsets int64 [numBatches]: a batch's first row of the table.
totals int64 [numBatches, 3]: its (B, Nb, Eb), the numbers of graphs, nodes and edges."""


def graphBatchPlan(nodeCounts: Sequence[int], edgeCounts: Sequence[int], order: Sequence[int], minibatchSize: int) -> GraphBatchPlan:
    """the host plan of an epoch: `order` (graph ids, repeats allowed) cut into groups of minibatchSize, the last possibly short, as
    `grouped` cuts them in the reference.  Pure numpy."""
    nodeCounts, edgeCounts = np.asarray(nodeCounts, dtype=np.int64).reshape(-1), np.asarray(edgeCounts, dtype=np.int64).reshape(-1)
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    mb, n = int(minibatchSize), len(order)
    assert mb >= 1, f"minibatchSize = {minibatchSize}"
    assert len(nodeCounts) == len(edgeCounts), f"{len(nodeCounts)} node counts, {len(edgeCounts)} edge counts"
    assert n == 0 or (order.min() >= 0 and order.max() < len(nodeCounts)), f"the order names graphs outside [0, {len(nodeCounts)})"
    nodePtr = np.concatenate([[0], np.cumsum(nodeCounts)]).astype(np.int64)
    edgePtr = np.concatenate([[0], np.cumsum(edgeCounts)]).astype(np.int64)
    offsets = np.arange(0, n, mb, dtype=np.int64)
    table, totals = np.zeros((n, 4), dtype=np.int64), np.zeros((len(offsets), 3), dtype=np.int64)
    table[:, 0], table[:, 2] = nodePtr[order], edgePtr[order]
    nc, ec = nodeCounts[order], edgeCounts[order]
    for k, off in enumerate(offsets):
        sl = slice(off, min(off + mb, n))
        table[sl, 1] = np.cumsum(nc[sl]) - nc[sl]
        table[sl, 3] = np.cumsum(ec[sl]) - ec[sl]
        totals[k] = (sl.stop - sl.start, nc[sl].sum(), ec[sl].sum())
    return GraphBatchPlan(table, offsets, totals)


class GraphSet:
    """a data set of small graphs packed on the device: nodeFeatures [sum N, F], edgeFeatures [sum E, ...], edgeI / edgeJ [sum E] with
    set-wide node ids, nodePtr / edgePtr [G + 1] (also on the host: hostNodePtr, hostEdgePtr).  Checked once, here: every graph has a
    node (none needs an edge), all agree in feature widths and types, 2 * sum E < 2^31, and every endpoint of graph g lies in [0, N_g) -
    one comparison kernel and one host read; a cross-graph edge would otherwise rebase out of its batch.  The set-wide Adjacency (per
    feature type) and EdgeCsr are built on first use, once, and shared by every stream over the set."""

    def __init__(self, graphs: Sequence["GraphBatchStream.Graph"], device: int = 0):
        graphs = list(graphs)
        assert len(graphs) >= 1, "a graph set needs a graph"
        first = graphs[0]
        nodeShape, edgeShape = first.nodeFeatures.shape, first.edgeFeatures.shape
        assert len(nodeShape) == 2, f"nodeFeatures must be [N, F], graph 0 has {nodeShape}"
        for k, g in enumerate(graphs):
            ns, es = g.nodeFeatures.shape, g.edgeFeatures.shape
            assert len(ns) == 2 and ns[0] >= 1, f"graph {k}: nodeFeatures {ns} must be [N, F] with at least one node"
            assert ns[1:] == nodeShape[1:] and len(es) >= 1 and es[1:] == edgeShape[1:], \
                f"graph {k}: feature widths {ns[1:]} / {es[1:]} differ from graph 0's {nodeShape[1:]} / {edgeShape[1:]}"
            assert g.nodeFeatures.dtype == first.nodeFeatures.dtype and g.edgeFeatures.dtype == first.edgeFeatures.dtype, \
                f"graph {k}: feature types differ from graph 0's"
            assert g.edgeI.dtype == I64 and g.edgeJ.dtype == I64 and len(g.edgeI.shape) == 1 and len(g.edgeJ.shape) == 1, \
                f"graph {k}: edgeI and edgeJ must be int64 vectors"
            assert g.edgeI.shape[0] == g.edgeJ.shape[0] == es[0], f"graph {k}: edgeI [{g.edgeI.shape[0]}], edgeJ [{g.edgeJ.shape[0]}], edgeFeatures {es} differ in length"
            for t in (g.nodeFeatures, g.edgeFeatures, g.edgeI, g.edgeJ):
                assert t.device == device, f"graph {k}: a tensor lives on device {t.device}, the set on {device} (host-resident sets are not supported)"
        self.device, self.numGraphs = device, len(graphs)
        self.nodeCounts = np.array([g.nodeFeatures.shape[0] for g in graphs], dtype=np.int64)
        self.edgeCounts = np.array([g.edgeI.shape[0] for g in graphs], dtype=np.int64)
        self.hostNodePtr = np.concatenate([[0], np.cumsum(self.nodeCounts)]).astype(np.int64)
        self.hostEdgePtr = np.concatenate([[0], np.cumsum(self.edgeCounts)]).astype(np.int64)
        self.numNodes, self.numEdges = int(self.hostNodePtr[-1]), int(self.hostEdgePtr[-1])
        assert 2 * self.numEdges < 2 ** 31, f"too many edges: {self.numEdges}"
        self.nodeDtype, self.edgeDtype = first.nodeFeatures.dtype, first.edgeFeatures.dtype
        self.nodePtr, self.edgePtr = STen.from_numpy(self.hostNodePtr, device), STen.from_numpy(self.hostEdgePtr, device)
        self.nodeFeatures = STen.cat([g.nodeFeatures for g in graphs], 0)
        withEdges = [g for g in graphs if g.edgeI.shape[0]]
        if withEdges:
            self.edgeFeatures = STen.cat([g.edgeFeatures for g in withEdges], 0)
            # local ids to set-wide ids: one add of the owning graph's first node row per edge
            base = STen.from_numpy(np.repeat(self.hostNodePtr[:-1], self.edgeCounts), device)
            self.edgeI = STen.cat([g.edgeI for g in withEdges], 0) + base
            self.edgeJ = STen.cat([g.edgeJ for g in withEdges], 0) + base
            bad = C.c_void_p()
            lib.lamp_graph_set_check(C.byref(bad), self.edgeI.h, self.edgeJ.h, self.nodePtr.h, self.edgePtr.h)
            assert int(STen(bad).to_numpy()[0]) == 0, "an edge endpoint lies outside [0, N) of its own graph"
        else:
            self.edgeFeatures = STen.zeros([0] + list(edgeShape[1:]), self.edgeDtype, device)
            self.edgeI, self.edgeJ = STen.zeros([0], I64, device), STen.zeros([0], I64, device)
        self._groupings = {}

    @property
    def fusable(self) -> bool:
        """whether the collate kernels serve this set: f32 / f64 node features (anything else takes the chain)"""
        return self.nodeDtype in (F32, F64)

    def adjacency(self) -> G.Adjacency:
        key = ("adjacency", self.nodeDtype)
        if key not in self._groupings:
            self._groupings[key] = G.computeAdjacency(self.edgeI, self.edgeJ, self.numNodes, self.nodeDtype)
        return self._groupings[key]

    def edgeCsr(self) -> G.EdgeCsr:
        if "edgeCsr" not in self._groupings:
            self._groupings["edgeCsr"] = G.computeEdgeCsr(self.edgeI, self.edgeJ, self.numNodes)
        return self._groupings["edgeCsr"]

    def collate(self, plan: STen, offset: int, B: int, Nb: int, Eb: int, groupings: Sequence[str] = ("adjacency", "edgeCsr")) -> G.Graph:
        """the batch of the graphs that rows [offset, offset + B) of `plan` (the uploaded table of graphBatchPlan) name, with Nb nodes and
        Eb edges: at most four launches, no host read.  Its caches hold the groupings asked for, under Graph.adjacency()'s and
        Graph.edgeCsr()'s keys."""
        assert self.fusable, "the collate kernels serve f32 / f64 node features"
        assert all(g in ("adjacency", "edgeCsr") for g in groupings), groupings
        adj = self.adjacency() if "adjacency" in groupings else None
        csr = self.edgeCsr() if "edgeCsr" in groupings else None
        of = lambda owner, name: getattr(owner, name).h if owner is not None else None      # a set-wide array, or NULL
        ref = lambda o, owner: C.byref(o) if owner is not None else None                  # its output, or NULL
        nodes, edges, pool, gptr, arp, dinv, irp, orp, ei, ej, col, ipm, opm = (C.c_void_p() for _ in range(13))
        where = (plan.h, int(offset), int(B))
        lib.lamp_graph_batch_rows(C.byref(nodes), self.nodeFeatures.h, *where, int(Nb), 0)
        lib.lamp_graph_batch_rows(C.byref(edges), self.edgeFeatures.h, *where, int(Eb), 1)
        lib.lamp_graph_batch_nodes(C.byref(pool), C.byref(gptr), ref(arp, adj), ref(dinv, adj), ref(irp, csr), ref(orp, csr), *where, int(Nb), int(Eb),
                                   of(adj, "rowptr"), of(adj, "dinv"), of(csr, "inRowptr"), of(csr, "outRowptr"))
        lib.lamp_graph_batch_edges(C.byref(ei), C.byref(ej), ref(col, adj), ref(ipm, csr), ref(opm, csr), *where, int(Nb), int(Eb),
                                   self.edgeI.h, self.edgeJ.h, of(adj, "col"), of(csr, "inPerm"), of(csr, "outPerm"))
        edgeI, edgeJ = STen(ei), STen(ej)
        caches = {}
        if adj is not None:
            caches[(int(Nb), self.nodeDtype)] = G.Adjacency(STen(arp), STen(col), STen(dinv), edgeI, edgeJ, int(Nb))
        if csr is not None:
            caches[("edgeCsr", int(Nb))] = G.EdgeCsr(STen(irp), STen(ipm), STen(orp), STen(opm), edgeI, edgeJ, int(Nb))
        return G.Graph(const(STen(nodes)), const(STen(edges)), edgeI, edgeJ, STen(pool), caches, STen(gptr))

    def collateComposed(self, ids: Sequence[int]) -> G.Graph:
        """the reference's fold (GraphBatchStream.scala:42-113) out of existing operators: per graph two adds and the graph index, then five
        cats; a Graph with empty caches and no graphPtr"""
        nodes, edges, eis, ejs, idx, offset = [], [], [], [], [], 0
        for b, g in enumerate(ids):
            n0, e0, n, e = int(self.hostNodePtr[g]), int(self.hostEdgePtr[g]), int(self.nodeCounts[g]), int(self.edgeCounts[g])
            nodes.append(self.nodeFeatures.narrow(0, n0, n))
            idx.append(STen.zeros([n], I64, self.device) + b)
            if e:
                edges.append(self.edgeFeatures.narrow(0, e0, e))
                eis.append(self.edgeI.narrow(0, e0, e) + (offset - n0))
                ejs.append(self.edgeJ.narrow(0, e0, e) + (offset - n0))
            offset += n
        if eis:
            edgeFeatures, edgeI, edgeJ = STen.cat(edges, 0), STen.cat(eis, 0), STen.cat(ejs, 0)
        else:
            edgeFeatures = STen.zeros([0] + self.edgeFeatures.shape[1:], self.edgeDtype, self.device)
            edgeI, edgeJ = STen.zeros([0], I64, self.device), STen.zeros([0], I64, self.device)
        return G.Graph(const(STen.cat(nodes, 0)), const(edgeFeatures), edgeI, edgeJ, STen.cat(idx, 0))


class _SmallGraphStream:
    """the stream smallGraphStream returns: (Graph, target) pairs.  The order is fixed at construction; reset() replays it."""

    def __init__(self, graphSet: GraphSet, targetPerGraph: STen, order: Sequence[int], minibatchSize: int, groupings: Sequence[str]):
        assert targetPerGraph.shape[0] == graphSet.numGraphs, f"targetPerGraph {targetPerGraph.shape} does not have a row per graph ({graphSet.numGraphs})"
        assert targetPerGraph.device == graphSet.device, "targetPerGraph lives on another device than the set"
        self.set, self.target, self.groupings = graphSet, targetPerGraph, tuple(groupings)
        self.order = np.asarray(order, dtype=np.int64).reshape(-1)
        self.plan = graphBatchPlan(graphSet.nodeCounts, graphSet.edgeCounts, self.order, minibatchSize)
        # the whole epoch's table and order, uploaded once: a batch hands the kernels a slice
        self._table = STen.from_numpy(np.ascontiguousarray(self.plan.table), graphSet.device)
        self._order = STen.from_numpy(np.ascontiguousarray(self.order), graphSet.device)
        self._next = 0

    @property
    def numBatches(self) -> int: return len(self.plan.offsets)

    def nextBatch(self) -> Optional[Tuple[G.Graph, STen]]:
        k = self._next
        if k >= self.numBatches:
            return None
        self._next = k + 1
        off, (B, Nb, Eb) = int(self.plan.offsets[k]), (int(v) for v in self.plan.totals[k])
        target = self.target.indexSelect(0, self._order.narrow(0, off, B))
        if G._batch_fused and self.set.fusable:
            return self.set.collate(self._table, off, B, Nb, Eb, self.groupings), target
        return self.set.collateComposed(self.order[off:off + B].tolist()), target

    def reset(self) -> None: self._next = 0

    def __iter__(self) -> Iterator[Tuple[G.Graph, STen]]:
        while True:
            b = self.nextBatch()
            if b is None:
                return
            yield b


class _SingleStream:
    """BatchStream.single: one batch"""

    def __init__(self, batch): self._batch, self._done = batch, False

    @property
    def numBatches(self) -> int: return 1

    def nextBatch(self):
        if self._done:
            return None
        self._done = True
        return self._batch

    def reset(self) -> None: self._done = False

    def __iter__(self):
        while True:
            b = self.nextBatch()
            if b is None:
                return
            yield b


class GraphBatchStream:
    """object GraphBatchStream (GraphBatchStream.scala)"""

    class Graph:
        """GraphBatchStream.Graph(nodeFeatures, edgeFeatures, edgeI, edgeJ): one graph as plain tensors, edge ids local to it; edgeFeatures
        is [E] or [E, ...]"""

        def __init__(self, nodeFeatures: STen, edgeFeatures: STen, edgeI: STen, edgeJ: STen):
            self.nodeFeatures, self.edgeFeatures, self.edgeI, self.edgeJ = nodeFeatures, edgeFeatures, edgeI, edgeJ

        def toVariable(self) -> G.Graph:
            """GraphBatchStream.scala:15-21, with the reference's dummy vertexPoolingIndices = zeros([1]) (f32, as STen.zeros gives it there)"""
            return G.Graph(const(self.nodeFeatures), const(self.edgeFeatures), self.edgeI, self.edgeJ, STen.zeros([1], F32, self.nodeFeatures.device))

    @staticmethod
    def smallGraphStream(minibatchSize: int, graphNodesAndEdges, targetPerGraph: STen, rng, transferBufferSize: Optional[int] = None, device: int = 0,
                         groupings: Sequence[str] = ("adjacency", "edgeCsr")) -> _SmallGraphStream:
        """minibatches of whole graphs with one target per graph (GraphBatchStream.scala:29-182): a stream of (lamp_amd.graph.Graph, target)
        with numBatches, nextBatch(), reset() and iteration.  graphNodesAndEdges: a list of GraphBatchStream.Graph, or a GraphSet (to share
        one packed set and its groupings among streams).  The order is rng.shuffle(range(G)) (data.JavaRandom or anything with shuffle), or
        0 .. G - 1 without an rng, fixed here and cut into groups of minibatchSize, the last possibly short.  `groupings` names what the
        batch Graph's caches are filled with.  transferBufferSize is accepted for the reference's signature and unused: the set is
        resident in device memory, nothing is staged through a transfer buffer."""
        graphSet = graphNodesAndEdges if isinstance(graphNodesAndEdges, GraphSet) else GraphSet(graphNodesAndEdges, device)
        ids = list(range(graphSet.numGraphs))
        order = rng.shuffle(ids) if rng is not None else ids
        return _SmallGraphStream(graphSet, targetPerGraph, order, minibatchSize, groupings)

    @staticmethod
    def singleLargeGraph(graph: "GraphBatchStream.Graph", targetPerNode: STen) -> _SingleStream:
        """one full batch of one big graph with a target per node (GraphBatchStream.scala:188-196)"""
        return _SingleStream((graph.toVariable(), targetPerNode))
