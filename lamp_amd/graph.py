"""lamp.nn.graph over the C ABI: Graph, GCN, gcn, gcnAggregation, VertexPooling (and nn.ResidualModule, which gcn needs), GraphAttention,
multiheadGraphAttention, MPNN.  Minibatches of many small graphs are lamp_amd.graphbatch's.

Reference: lamp-core/src/main/scala/lamp/nn/graph/{Graph,GCN,VertexPooling,GraphAttention}.scala.  GCN.computeSparseAdjacency builds a sparse COO
tensor and gcnAggregation multiplies it with `mm`; here the adjacency is a CSR (`lamp_gcn_adjacency`) and the product one gather-only
kernel (`lamp_gcn_aggregate`, the autograd node `GcnAggregation`), forward and backward.  The same mathematics out of IndexSelect,
IndexAdd and the broadcasting operators (`gcnAggregationComposed`) is the fallback for other types than f32 / f64 and the yardstick
of scripts/gcn_probe.py; `gcnFused` switches between the two.

GraphAttention.multiheadGraphAttention scores every edge and then takes, per destination, the softmax of the scores and the sum of the
sources' values under it.  The scoring is a composition of existing nodes (on the fused path its two key gathers are GraphGather nodes,
whose gradient is summed over the edge CSR without atomics); everything after it is one node, `GraphAttentionAggregate`
(`lamp_gat_forward` / `lamp_gat_backward` over the two groupings of `Graph.edgeCsr()`), or the reference's own chain of exp, indexAdd,
log, indexSelect and Mult (`graphAttentionAggregateComposed`); `graphAttentionFused` switches between the two.

MPNN's two data movements are a node each: `MpnnMessage` writes cat(edgeFeatures, x[edgeI], x[edgeJ]) in one launch and hands x the true
gradient, `MpnnAggregate` is MPNN.aggregate (`lamp_mpnn_*` over `Graph.edgeCsr()` and the degree factors the graph caches); the chains of
IndexSelect / Concatenate and Mult / IndexAdd / Add nodes (`mpnnMessageComposed`, `mpnnAggregateComposed`) are the fallback, `mpnnFused`
switches between the two.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

from ._capi import lib
from .autograd import Variable, apply_op, const, param
from . import nn
from .sten import STen, F32, F64

_fused = True


def gcnFused(on: bool) -> bool:
    """process-wide: gcnAggregation as one GcnAggregation node over the CSR kernel (True, the default) or as the composed chain of
    IndexSelect / IndexAdd / Mult nodes; returns the previous setting."""
    global _fused
    prev, _fused = _fused, bool(on)
    return prev


def longRow() -> int:
    """rows of more neighbours than this are split across the waves of a workgroup (lamp_gcn_long_row)"""
    n = C.c_int64(); lib.lamp_gcn_long_row(C.byref(n)); return n.value


class Adjacency:
    """A + A' as a CSR with multiplicity and D^-1/2 of A + A' + I (the self loop is implicit): what computeSparseAdjacency returns,
    in the form the kernel reads.  Keeps the edge list for the composed chain."""

    def __init__(self, rowptr: STen, col: STen, dinv: STen, edgeI: STen, edgeJ: STen, numNodes: int):
        self.rowptr, self.col, self.dinv, self.edgeI, self.edgeJ, self.numNodes = rowptr, col, dinv, edgeI, edgeJ, numNodes

    @property
    def dtype(self): return self.dinv.dtype

    @property
    def tensors(self): return [self.rowptr, self.col, self.dinv]


def computeAdjacency(edgeI: STen, edgeJ: STen, numNodes: int, dtype=F32) -> Adjacency:
    """GCN.computeSparseAdjacency (GCN.scala:30-114); an endpoint outside [0, numNodes) raises"""
    r, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p()
    lib.lamp_gcn_adjacency(C.byref(r), C.byref(c), C.byref(d), edgeI.h, edgeJ.h, int(numNodes), int(dtype))
    return Adjacency(STen(r), STen(c), STen(d), edgeI, edgeJ, int(numNodes))


def gcnAggregationComposed(nodeFeatures: Variable, edgeI: STen, edgeJ: Optional[STen] = None) -> Variable:
    """degrees * ((A + A' + I) mm (nodeFeatures * degrees)) out of the plain operators: the rows x[j] * d[j] gathered for the entries of
    A + A' + I (IndexSelect over the 2E directed entries and the N self loops), summed per target (IndexAdd), scaled again.  The self
    loops are index entries, not a second use of the scaled features: IndexSelect's backward closure doubles a gradient its input has
    already received (ops.scala's `out += out.indexAdd(...)`, mirrored in host/ops.cpp), so its input must have no other consumer.
    `edgeI` may be an Adjacency."""
    if isinstance(edgeI, Adjacency):
        edgeI, edgeJ = edgeI.edgeI, edgeI.edgeJ
    x = nodeFeatures.value
    n = x.shape[0]
    if edgeI.numel == 0:
        return nodeFeatures                                            # every degree is 1: the identity
    nodes = STen.arange(0, n, 1, edgeI.dtype, edgeI.device)
    counts = STen.cat([edgeI, edgeJ], 0).bincount(None, n) + 1         # GCN.scala:52-60
    degrees = const(counts.castToType(x.dtype).pow(-0.5).unsqueeze(1))
    target, source = STen.cat([edgeI, edgeJ, nodes], 0), STen.cat([edgeJ, edgeI, nodes], 0)
    return (nodeFeatures * degrees).indexSelect(0, const(source)).indexAdd(const(target), 0, n) * degrees


def gcnAggregation(nodeFeatures: Variable, edgeI, edgeJ: Optional[STen] = None) -> Variable:
    """GCN.gcnAggregation(nodeFeatures, edgeI, edgeJ) (GCN.scala:127-136) or, with an Adjacency in place of the edge list, the overload
    over a precomputed adjacency (GCN.scala:137-145)."""
    dt = nodeFeatures.value.dtype
    if not _fused or dt not in (F32, F64):
        return gcnAggregationComposed(nodeFeatures, edgeI, edgeJ)
    adj = edgeI if isinstance(edgeI, Adjacency) else computeAdjacency(edgeI, edgeJ, nodeFeatures.value.shape[0], dt)
    return apply_op("GcnAggregation", [nodeFeatures], tensors=adj.tensors)


class EdgeCsr:
    """the edge ids grouped by destination (`incoming`: rowptr and perm of edgeJ) and by source (`outgoing`: of edgeI), each group in the
    order of the edge list (lamp_graph_edge_csr): what lamp_gat_forward and lamp_gat_backward read"""

    def __init__(self, inRowptr: STen, inPerm: STen, outRowptr: STen, outPerm: STen, edgeI: STen, edgeJ: STen, numNodes: int):
        self.inRowptr, self.inPerm, self.outRowptr, self.outPerm = inRowptr, inPerm, outRowptr, outPerm
        self.edgeI, self.edgeJ, self.numNodes = edgeI, edgeJ, numNodes

    @property
    def incoming(self): return [self.inRowptr, self.inPerm]

    @property
    def outgoing(self): return [self.outRowptr, self.outPerm]

    @property
    def tensors(self): return [self.edgeI, self.edgeJ, self.inRowptr, self.inPerm, self.outRowptr, self.outPerm]


def _edge_csr(index: STen, numNodes: int):
    r, p = C.c_void_p(), C.c_void_p()
    lib.lamp_graph_edge_csr(C.byref(r), C.byref(p), index.h, int(numNodes))
    return STen(r), STen(p)


def computeEdgeCsr(edgeI: STen, edgeJ: STen, numNodes: int) -> EdgeCsr:
    """both groupings of an edge list; an endpoint outside [0, numNodes) raises"""
    return EdgeCsr(*_edge_csr(edgeJ, numNodes), *_edge_csr(edgeI, numNodes), edgeI, edgeJ, int(numNodes))


class Graph:
    """Graph(nodeFeatures, edgeFeatures, edgeI, edgeJ, vertexPoolingIndices) (Graph.scala).  The adjacency of the edge list, its
    grouping by endpoint and MPNN's degree factors (keyed by N, type, exponent and side) are built on first use and shared by every
    copy(nodeFeatures = ...), so stacked GCN, GraphAttention or MPNN layers over one graph build them once.  `graphPtr` (int64 [B + 1], the
    node offsets of the graphs of a collated minibatch, lamp_amd.graphbatch) says that vertexPoolingIndices is sorted: VertexPooling then sums
    consecutive rows."""

    def __init__(self, nodeFeatures: Variable, edgeFeatures: Optional[Variable], edgeI: STen, edgeJ: STen, vertexPoolingIndices: Optional[STen] = None,
                 _adjacencies: Optional[dict] = None, graphPtr: Optional[STen] = None):
        self.nodeFeatures, self.edgeFeatures, self.edgeI, self.edgeJ, self.vertexPoolingIndices = nodeFeatures, edgeFeatures, edgeI, edgeJ, vertexPoolingIndices
        self._adjacencies = _adjacencies if _adjacencies is not None else {}
        self.graphPtr = graphPtr

    def copy(self, nodeFeatures: Optional[Variable] = None) -> "Graph":
        return Graph(nodeFeatures if nodeFeatures is not None else self.nodeFeatures, self.edgeFeatures, self.edgeI, self.edgeJ, self.vertexPoolingIndices,
                     self._adjacencies, self.graphPtr)

    def adjacency(self, dtype=None) -> Adjacency:
        x = self.nodeFeatures.value
        key = (x.shape[0], x.dtype if dtype is None else dtype)
        if key not in self._adjacencies:
            self._adjacencies[key] = computeAdjacency(self.edgeI, self.edgeJ, key[0], key[1])
        return self._adjacencies[key]

    def edgeCsr(self) -> EdgeCsr:
        key = ("edgeCsr", self.nodeFeatures.value.shape[0])
        if key not in self._adjacencies:
            self._adjacencies[key] = computeEdgeCsr(self.edgeI, self.edgeJ, key[1])
        return self._adjacencies[key]


class _OverTransform:
    """a module whose state, training mode and load are those of `self.transform`"""
    transform: nn.Module

    @property
    def state(self) -> List[Variable]: return self.transform.state

    @property
    def parameters(self) -> List[Variable]: return self.transform.parameters

    def zeroGrad(self): self.transform.zeroGrad()
    def asEval(self): self.transform.asEval(); return self
    def asTraining(self): self.transform.asTraining(); return self
    def load(self, tensors: Sequence[STen]): self.transform.load(tensors)


class ResidualModule(_OverTransform):
    """ResidualModule(transform) (nn/ResidualModule.scala): transform(x) + x where the shapes agree, transform(x) otherwise"""

    def __init__(self, transform):
        self.transform = transform

    def forward(self, x: Variable) -> Variable:
        n = self.transform.forward(x)
        return n + x if n.shape == x.shape else n


class GCN(_OverTransform):
    """GCN(transform) (GCN.scala:10-26): forward(graph) = graph.copy(nodeFeatures = transform(gcnAggregation(graph)))"""

    def __init__(self, transform):
        self.transform = transform

    def forward(self, x: Graph) -> Graph:
        dt = x.nodeFeatures.value.dtype
        if _fused and dt in (F32, F64):
            message = gcnAggregation(x.nodeFeatures, x.adjacency())
        else:
            message = gcnAggregationComposed(x.nodeFeatures, x.edgeI, x.edgeJ)
        return x.copy(nodeFeatures=self.transform.forward(message))


def gcn(in_: int, out: int, dtype=F32, device=0, dropout=0.0, nonLinearity=True) -> GCN:
    """GCN.gcn (GCN.scala:158-186): GCN(ResidualModule(Linear(bias = false) -> BatchNorm [-> relu -> Dropout]))"""
    mods = [nn.Linear(in_, out, dtype, device, bias=False), nn.BatchNorm(out, dtype, device)]
    if nonLinearity:
        mods += [nn.Fun("relu"), nn.Dropout(dropout)]
    return GCN(ResidualModule(nn.Sequential(*mods)))


_batch_fused = True


def graphBatchFused(on: bool) -> bool:
    """process-wide: minibatches of small graphs collated by the graph_batch kernels out of the data set's own groupings, and pooled by the
    SegmentPool node (True, the default), or the reference's fold out of existing operators into a Graph with empty caches and the composed
    VertexPooling; returns the previous setting."""
    global _batch_fused
    prev, _batch_fused = _batch_fused, bool(on)
    return prev


def VertexPooling(x: Graph, pooling: str) -> Variable:
    """VertexPooling(graph, Sum | Mean) (VertexPooling.scala): node features summed (averaged) per value of vertexPoolingIndices.  A
    collated batch (graphPtr set) in f32 / f64 with graphBatchFused(True): one SegmentPool node over the consecutive rows of every graph,
    no atomics and no host read; otherwise IndexAdd after a host read of the largest index."""
    assert pooling in ("Sum", "Mean"), pooling
    idx = x.vertexPoolingIndices
    if x.graphPtr is not None and _batch_fused and x.nodeFeatures.value.dtype in (F32, F64):
        return apply_op("SegmentPool", [x.nodeFeatures], tensors=[x.graphPtr, idx], i=[int(pooling == "Mean")])
    maxi = int(idx.castToDouble().maxAll().item()) + 1              # the max reduction exists for floating types; exact below 2^53
    total = x.nodeFeatures.indexAdd(const(idx), 0, maxi)
    if pooling == "Sum":
        return total
    v = x.nodeFeatures.value
    ones = const(STen.ones([v.shape[0], 1], v.dtype, v.device))
    return total / ones.indexAdd(const(idx), 0, maxi)


# ---- graph attention (GraphAttention.scala) ----------------------------------------------------------------------------------------------------
_gat_fused = True


def graphAttentionFused(on: bool) -> bool:
    """process-wide: everything after the scores as one GraphAttentionAggregate node over the edge CSR (True, the default) or as the
    reference's chain of Exp / IndexAdd / Log / IndexSelect / Mult nodes; returns the previous setting."""
    global _gat_fused
    prev, _gat_fused = _gat_fused, bool(on)
    return prev


def gatLongRow() -> int:
    """destinations (sources) of more edges than this are split across the waves of a workgroup (lamp_gat_long_row)"""
    n = C.c_int64(); lib.lamp_gat_long_row(C.byref(n)); return n.value


def graphAttentionAggregateComposed(activations: Variable, nodeValue: Variable, edgeI: STen, edgeJ: STen, numHeads: int) -> Variable:
    """GraphAttention.scala:172-197 as written: activations [E, H] or [E, H, 1], nodeValue [N, H, V] -> [N, H * V].  The exponentials
    are taken against one global maximum, and the sums per destination are IndexAdds."""
    n = nodeValue.shape[0]
    c = const(activations.value.maxAll())
    e = (activations - c).exp()
    lse = e.indexAdd(const(edgeJ), 0, n).log() + c
    lseBroadCast = lse.indexSelect(0, const(edgeJ))
    logsoftmax = activations - lseBroadCast
    a = logsoftmax.exp().view([-1, numHeads, 1])
    nodeValueScatter = nodeValue.indexSelect(0, const(edgeI))
    shape = nodeValueScatter.shape
    return (a * nodeValueScatter).reshape([-1, shape[1] * shape[2]]).indexAdd(const(edgeJ), 0, n)


def graphAttentionAggregate(activations: Variable, nodeValue: Variable, edgeI: STen, edgeJ: STen, numHeads: int, csr: Optional[EdgeCsr] = None) -> Variable:
    """the softmax of activations [E, H] (or [E, H, 1]) over the edges that share a destination and the sum of the sources' rows of
    nodeValue [N, H, V] under it: [N, H * V].  f32 / f64 with graphAttentionFused(True): one GraphAttentionAggregate node over `csr`
    (built here if not given); otherwise the composed chain."""
    dt = nodeValue.value.dtype
    if not _gat_fused or dt not in (F32, F64):
        return graphAttentionAggregateComposed(activations, nodeValue, edgeI, edgeJ, numHeads)
    if csr is None:
        csr = computeEdgeCsr(edgeI, edgeJ, nodeValue.shape[0])
    score = activations if len(activations.shape) == 2 else activations.view([-1, numHeads])
    return apply_op("GraphAttentionAggregate", [score, nodeValue], tensors=[edgeI, edgeJ] + csr.incoming + csr.outgoing, i=[numHeads])


def _attention_scores(nodeFeatures, edgeFeatures, edgeI, edgeJ, wNodeKey1, wNodeKey2, wEdgeKey, wNodeValue, wAttention, numHeads, csr=None):
    """GraphAttention.scala:132-171: (activations, nodeValue) out of existing nodes.  The two key gathers are IndexSelect nodes, whose closure
    is an IndexAdd: atomic sums that land in the order the hardware schedules them.  With `csr` (the fused path) they are GraphGather nodes:
    the same values, and a gradient summed per node over the grouping in its order, a function of the input alone."""
    assert wNodeValue.shape[1] % numHeads == 0, f"wNodeValue and numHeads size do not align {wNodeValue.shape[1]} {numHeads}"

    def mm(a, b):
        return a.mm(b).view([a.shape[0], numHeads, b.shape[1] // numHeads])

    def keys(w, index, grouping):
        if csr is None:
            return mm(nodeFeatures, w).indexSelect(0, const(index))
        gathered = apply_op("GraphGather", [nodeFeatures.mm(w)], tensors=[index] + grouping)
        return gathered.view([index.shape[0], numHeads, w.shape[1] // numHeads])

    edgeKey, nodeValue = mm(edgeFeatures, wEdgeKey), mm(nodeFeatures, wNodeValue)
    ni, nj = keys(wNodeKey1, edgeI, csr.outgoing if csr is not None else None), keys(wNodeKey2, edgeJ, csr.incoming if csr is not None else None)
    if wAttention is not None:
        ninjeij = apply_op("Concatenate", [ni, nj, edgeKey], i=[2])
        k = ninjeij.shape[2]
        activations = ninjeij.transpose(0, 1).bmm(wAttention.view([k, numHeads, 1]).transpose(0, 1)).tanh().transpose(0, 1).view([-1, numHeads])
    else:
        prod = (ni * nj) * (1.0 / math.sqrt(float(ni.shape[1])))        # the reference scales by shape(1), the number of heads: kept
        activations = prod.sum([2], True) + edgeKey.reshape([-1, numHeads, 1])
    return activations, nodeValue


def multiheadGraphAttention(nodeFeatures: Variable, edgeFeatures: Variable, edgeI: STen, edgeJ: STen, wNodeKey1: Variable, wNodeKey2: Variable,
                            wEdgeKey: Variable, wNodeValue: Variable, wAttention: Optional[Variable], numHeads: int, csr: Optional[EdgeCsr] = None) -> Variable:
    """GraphAttention.multiheadGraphAttention (GraphAttention.scala:119-198): the next node representation [N, H * V], without
    non-linearity or dropout.  Self edges must be present in the edge list.  With wAttention the score of an edge is tanh of the
    concatenated keys times wAttention per head, without it the scaled dot product of the node keys plus the edge key."""
    if _gat_fused and nodeFeatures.value.dtype in (F32, F64):
        if csr is None:
            csr = computeEdgeCsr(edgeI, edgeJ, nodeFeatures.shape[0])
    else:
        csr = None
    activations, nodeValue = _attention_scores(nodeFeatures, edgeFeatures, edgeI, edgeJ, wNodeKey1, wNodeKey2, wEdgeKey, wNodeValue, wAttention, numHeads, csr)
    return graphAttentionAggregate(activations, nodeValue, edgeI, edgeJ, numHeads, csr)


def multiheadGraphAttentionComposed(nodeFeatures: Variable, edgeFeatures: Variable, edgeI: STen, edgeJ: STen, wNodeKey1: Variable, wNodeKey2: Variable,
                                    wEdgeKey: Variable, wNodeValue: Variable, wAttention: Optional[Variable], numHeads: int) -> Variable:
    """the same with the reference's own chain after the scores, whatever graphAttentionFused says"""
    activations, nodeValue = _attention_scores(nodeFeatures, edgeFeatures, edgeI, edgeJ, wNodeKey1, wNodeKey2, wEdgeKey, wNodeValue, wAttention, numHeads)
    return graphAttentionAggregateComposed(activations, nodeValue, edgeI, edgeJ, numHeads)


def _init_linear(in_: int, out: int, dtype, device) -> Variable:
    """nn.initLinear (nn/package.scala:102-109)"""
    return param(STen.normal(0.0, math.sqrt(2.0 / (out + in_)), [in_, out], dtype, device))


class GraphAttention:
    """GraphAttention (GraphAttention.scala:8-54): forward(graph) = graph.copy(nodeFeatures = [graph.nodeFeatures +] f(attention)) with
    f = dropout(swish1(.)) if nonLinearity; the residual applies only where the shapes agree.  State: wNodeKey1, wNodeKey2, wEdgeKey,
    wNodeValue[, wAttention].  The positional constructor takes the weights; GraphAttention.apply(...) initialises them."""

    def __init__(self, wNodeKey1: Variable, wNodeKey2: Variable, wEdgeKey: Variable, wNodeValue: Variable, wAttention: Optional[Variable],
                 nonLinearity: bool, dropout: float, numHeads: int, training: bool = True):
        self.wNodeKey1, self.wNodeKey2, self.wEdgeKey, self.wNodeValue, self.wAttention = wNodeKey1, wNodeKey2, wEdgeKey, wNodeValue, wAttention
        self.nonLinearity, self.dropout, self.numHeads, self.training = bool(nonLinearity), float(dropout), int(numHeads), bool(training)

    @staticmethod
    def apply(nodeDim: int, edgeDim: int, attentionKeyHiddenDimPerHead: int, attentionNumHeads: int, valueDimPerHead: int, dropout: float = 0.0,
              dtype=F32, device=0, dotProductAttention: bool = False, nonLinearity: bool = True) -> "GraphAttention":
        """GraphAttention.apply (GraphAttention.scala:58-106)"""
        keys = attentionKeyHiddenDimPerHead * attentionNumHeads
        return GraphAttention(
            _init_linear(nodeDim, keys, dtype, device), _init_linear(nodeDim, keys, dtype, device),
            _init_linear(edgeDim, attentionNumHeads if dotProductAttention else keys, dtype, device),
            _init_linear(nodeDim, valueDimPerHead * attentionNumHeads, dtype, device),
            None if dotProductAttention else _init_linear(attentionKeyHiddenDimPerHead * 3, attentionNumHeads, dtype, device),
            nonLinearity, dropout, attentionNumHeads)

    def forward(self, x: Graph) -> Graph:
        dt = x.nodeFeatures.value.dtype
        csr = x.edgeCsr() if _gat_fused and dt in (F32, F64) else None
        activation = multiheadGraphAttention(x.nodeFeatures, x.edgeFeatures, x.edgeI, x.edgeJ, self.wNodeKey1, self.wNodeKey2, self.wEdgeKey,
                                             self.wNodeValue, self.wAttention, self.numHeads, csr)
        nxt = (activation * activation.sigmoid()).dropout(self.dropout, self.training) if self.nonLinearity else activation      # swish1, Dropout
        return x.copy(nodeFeatures=x.nodeFeatures + nxt if nxt.shape == x.nodeFeatures.shape else nxt)

    @property
    def state(self) -> List[Variable]:
        return [self.wNodeKey1, self.wNodeKey2, self.wEdgeKey, self.wNodeValue] + ([self.wAttention] if self.wAttention is not None else [])

    @property
    def parameters(self) -> List[Variable]: return [v for v in self.state if v.needsGrad]

    def zeroGrad(self):
        for v in self.state:
            v.zeroGrad()

    def asEval(self): self.training = False; return self
    def asTraining(self): self.training = True; return self

    def load(self, tensors: Sequence[STen]):
        st = self.state
        assert len(st) == len(tensors), f"state has {len(st)} tensors, got {len(tensors)}"
        for v, t in zip(st, tensors):
            v.value.copyFrom(t)


# ---- message passing (MPNN.scala) ----------------------------------------------------------------------------------------------------------------
_mpnn_fused = True


def mpnnFused(on: bool) -> bool:
    """process-wide: MPNN's message and MPNN.aggregate as one MpnnMessage / MpnnAggregate node each over the edge CSR (True, the default) or
    as chains of IndexSelect / Concatenate and Mult / IndexAdd / Add nodes; returns the previous setting."""
    global _mpnn_fused
    prev, _mpnn_fused = _mpnn_fused, bool(on)
    return prev


def mpnnLongRow() -> int:
    """nodes of more edges than this are split across the waves of a workgroup (lamp_mpnn_long_row)"""
    n = C.c_int64(); lib.lamp_mpnn_long_row(C.byref(n)); return n.value


def countOccurences(t: STen, elems: int) -> STen:
    """MPNN.countOccurences (MPNN.scala:75-81): how often each of 0 .. elems - 1 occurs in the long vector t, as a long vector (the
    reference adds ones into zeros with indexAdd; a bincount gives the same counts)"""
    return t.bincount(None, int(elems))


def mpnnDegreeFactor(rowptr: STen, p: float, dtype) -> STen:
    """countOccurences(index, N).pow(p).castToType(dtype) from the rowptr of index's grouping: [N], computed in f32 whatever dtype is (the
    pow of a long tensor is an f32 tensor in the reference) and then cast; a node that does not occur gets inf"""
    o = C.c_void_p(); lib.lamp_mpnn_degree_factor(C.byref(o), rowptr.h, float(p), int(dtype)); return STen(o)


def _mpnn_factors(csr: EdgeCsr, dtype, degreeNormalizeI: bool, degreeNormalizeJ: bool, cache: Optional[dict] = None):
    """(fI, fJ): the factor vectors of MPNN.aggregate, None where the normalisation is off; kept in `cache` under (N, dtype, p, side)"""
    p = -0.5 if degreeNormalizeI and degreeNormalizeJ else -1.0

    def build(rowptr):               # the kernel writes f32 / f64; any other type (the composed chain's) is a cast of the f32 vector
        return mpnnDegreeFactor(rowptr, p, dtype) if dtype in (F32, F64) else mpnnDegreeFactor(rowptr, p, F32).castToType(dtype)

    def factor(side, rowptr):
        key = ("mpnnFactor", csr.numNodes, dtype, p, side)
        if cache is None:
            return build(rowptr)
        if key not in cache:
            cache[key] = build(rowptr)
        return cache[key]
    return (factor("I", csr.outRowptr) if degreeNormalizeI else None, factor("J", csr.inRowptr) if degreeNormalizeJ else None)


def _check_csr(csr: EdgeCsr, edgeI: STen, edgeJ: STen, numNodes: int):
    """a grouping handed in beside an edge list must be that edge list's: the same node count and edge count (its contents are not
    compared; the kernels index with edgeI and edgeJ, whose range the grouping's construction checked)"""
    assert csr.numNodes == int(numNodes), f"the edge CSR belongs to a graph of {csr.numNodes} nodes, not {numNodes}"
    assert csr.edgeI.numel == edgeI.numel and csr.edgeJ.numel == edgeJ.numel, \
        f"the edge CSR was built from {csr.edgeI.numel} edges, the edge list has {edgeI.numel} / {edgeJ.numel}"


def mpnnMessageComposed(nodeFeatures: Variable, edgeFeatures: Variable, edgeI: STen, edgeJ: STen) -> Variable:
    """cat(edgeFeatures, nodeFeatures[edgeI], nodeFeatures[edgeJ]) (MPNN.scala:21-25) out of IndexSelect and Concatenate.  Each gather
    goes through a `view` of nodeFeatures of its own: IndexSelect's backward closure doubles a gradient its input has already received
    (ops.scala's `out += out.indexAdd(...)`, mirrored in host/ops.cpp), and nodeFeatures has other consumers (the second gather, and in
    MPNN.forward the vertex transform's input and the residual), so IndexSelect's input must be a node no one else reads; View's closure
    then adds to nodeFeatures and the chain gives the true gradient."""
    shape = nodeFeatures.shape
    vI = nodeFeatures.view(shape).indexSelect(0, const(edgeI))
    vJ = nodeFeatures.view(shape).indexSelect(0, const(edgeJ))
    return apply_op("Concatenate", [edgeFeatures, vI, vJ], i=[1])


def mpnnMessage(nodeFeatures: Variable, edgeFeatures: Variable, edgeI: STen, edgeJ: STen, csr: Optional[EdgeCsr] = None) -> Variable:
    """the message of every edge, [E, Fe + 2 D].  f32 / f64 with mpnnFused(True): one MpnnMessage node over `csr` (built here if not
    given: that is where the endpoints' range is checked); otherwise the composed chain.  Either way nodeFeatures receives the true
    gradient, not the doubled one of the reference's literal chain."""
    dt = nodeFeatures.value.dtype
    if not _mpnn_fused or dt not in (F32, F64):
        return mpnnMessageComposed(nodeFeatures, edgeFeatures, edgeI, edgeJ)
    if csr is None:
        csr = computeEdgeCsr(edgeI, edgeJ, nodeFeatures.shape[0])
    _check_csr(csr, edgeI, edgeJ, nodeFeatures.shape[0])
    return apply_op("MpnnMessage", [nodeFeatures, edgeFeatures], tensors=[edgeI, edgeJ] + csr.incoming + csr.outgoing)


def mpnnAggregateComposed(numVertices: int, message: Variable, edgeI: STen, edgeJ: STen, degreeNormalizeI: bool, degreeNormalizeJ: bool,
                          aggregateJ: bool, csr: Optional[EdgeCsr] = None, _cache: Optional[dict] = None) -> Variable:
    """MPNN.aggregate (MPNN.scala:84-126) as the reference writes it: up to two broadcast Mults, an IndexAdd per direction, an Add.  The
    factor vectors alone do not come from the chain: the library has no pow of a long tensor, so they are lamp_mpnn_degree_factor's (the
    same f32 arithmetic) from the groupings' row pointers."""
    normalized = message
    if degreeNormalizeI or degreeNormalizeJ:
        if csr is None:
            csr = computeEdgeCsr(edgeI, edgeJ, numVertices)
        fI, fJ = _mpnn_factors(csr, message.value.dtype, degreeNormalizeI, degreeNormalizeJ, _cache)
        if fI is not None:
            normalized = normalized * const(fI.indexSelect(0, edgeI).view(-1, 1))
        if fJ is not None:
            normalized = normalized * const(fJ.indexSelect(0, edgeJ).view(-1, 1))
    aggI = normalized.indexAdd(const(edgeJ), 0, numVertices)
    if aggregateJ:
        return aggI + normalized.indexAdd(const(edgeI), 0, numVertices)
    return aggI


def mpnnAggregate(numVertices: int, message: Variable, edgeI: STen, edgeJ: STen, degreeNormalizeI: bool, degreeNormalizeJ: bool, aggregateJ: bool,
                  csr: Optional[EdgeCsr] = None, _cache: Optional[dict] = None) -> Variable:
    """MPNN.aggregate: message [E, M] -> [numVertices, M], every message scaled by count(edgeI)^p of its source and count(edgeJ)^p of its
    destination where those normalisations are on (p = -0.5 with both, else -1), summed per destination and, with aggregateJ, per source
    too.  f32 / f64 with mpnnFused(True): one MpnnAggregate node over `csr` (built here if not given); otherwise the composed chain."""
    dt = message.value.dtype
    if not _mpnn_fused or dt not in (F32, F64):
        return mpnnAggregateComposed(numVertices, message, edgeI, edgeJ, degreeNormalizeI, degreeNormalizeJ, aggregateJ, csr, _cache)
    if csr is None:
        csr = computeEdgeCsr(edgeI, edgeJ, numVertices)
    _check_csr(csr, edgeI, edgeJ, numVertices)
    fI, fJ = _mpnn_factors(csr, dt, degreeNormalizeI, degreeNormalizeJ, _cache)
    return apply_op("MpnnAggregate", [message], tensors=[edgeI, edgeJ] + csr.incoming + csr.outgoing + [f for f in (fI, fJ) if f is not None],
                    i=[int(bool(aggregateJ)), int(fI is not None), int(fJ is not None)])


class MPNN:
    """MPNN(messageTransform, vertexTransform, degreeNormalizeI, degreeNormalizeJ, aggregateJ) (MPNN.scala:8-48): forward(graph) =
    graph.copy(nodeFeatures = [graph.nodeFeatures +] vertexTransform(cat(graph.nodeFeatures, aggregate(messageTransform(message))))); the
    residual applies only where the widths agree.  State: the message transform's followed by the vertex transform's."""

    def __init__(self, messageTransform, vertexTransform, degreeNormalizeI: bool = True, degreeNormalizeJ: bool = True, aggregateJ: bool = True):
        self.messageTransform, self.vertexTransform = messageTransform, vertexTransform
        self.degreeNormalizeI, self.degreeNormalizeJ, self.aggregateJ = bool(degreeNormalizeI), bool(degreeNormalizeJ), bool(aggregateJ)

    def forward(self, x: Graph) -> Graph:
        assert x.edgeFeatures is not None, "MPNN needs edge features"
        n = x.nodeFeatures.shape[0]
        # built whatever the form and the type, on purpose: its construction is the endpoints' range check, and the degree factors come from
        # its row pointers in the composed chain too; the cost is two sorts per graph, once (the graph caches it)
        csr = x.edgeCsr()
        message = mpnnMessage(x.nodeFeatures, x.edgeFeatures, x.edgeI, x.edgeJ, csr)
        messageTx = self.messageTransform.forward(message)
        aggregated = mpnnAggregate(n, messageTx, x.edgeI, x.edgeJ, self.degreeNormalizeI, self.degreeNormalizeJ, self.aggregateJ, csr, x._adjacencies)
        updated = self.vertexTransform.forward(apply_op("Concatenate", [x.nodeFeatures, aggregated], i=[1]))
        return x.copy(nodeFeatures=x.nodeFeatures + updated if updated.shape[1] == x.nodeFeatures.shape[1] else updated)

    @property
    def state(self) -> List[Variable]: return list(self.messageTransform.state) + list(self.vertexTransform.state)

    @property
    def parameters(self) -> List[Variable]: return [v for v in self.state if v.needsGrad]

    def zeroGrad(self): self.messageTransform.zeroGrad(); self.vertexTransform.zeroGrad()
    def asEval(self): self.messageTransform.asEval(); self.vertexTransform.asEval(); return self
    def asTraining(self): self.messageTransform.asTraining(); self.vertexTransform.asTraining(); return self

    def load(self, tensors: Sequence[STen]):
        """Load.compose: the first len(messageTransform.state) tensors go to the message transform, the rest to the vertex transform"""
        tensors = list(tensors)
        k, m = len(self.messageTransform.state), len(self.vertexTransform.state)
        assert len(tensors) == k + m, f"state has {k + m} tensors, got {len(tensors)}"
        self.messageTransform.load(tensors[:k])
        self.vertexTransform.load(tensors[k:])
