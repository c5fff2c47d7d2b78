"""lamp.nn.graph's GCN path over the C ABI: Graph, GCN, gcn, gcnAggregation, VertexPooling (and nn.ResidualModule, which gcn needs).

Reference: lamp-core/src/main/scala/lamp/nn/graph/{Graph,GCN,VertexPooling}.scala.  GCN.computeSparseAdjacency builds a sparse COO
tensor and gcnAggregation multiplies it with `mm`; here the adjacency is a CSR (`lamp_gcn_adjacency`) and the product one gather-only
kernel (`lamp_gcn_aggregate`, the autograd node `GcnAggregation`), forward and backward.  The same mathematics out of IndexSelect,
IndexAdd and the broadcasting operators (`gcnAggregationComposed`) is the fallback for other types than f32 / f64 and the yardstick
of scripts/gcn_probe.py; `gcnFused` switches between the two.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

from ._capi import lib
from .autograd import Variable, apply_op, const
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


class Graph:
    """Graph(nodeFeatures, edgeFeatures, edgeI, edgeJ, vertexPoolingIndices) (Graph.scala).  The adjacency of the edge list is built on
    first use and shared by every copy(nodeFeatures = ...), so stacked GCN layers over one graph build it once."""

    def __init__(self, nodeFeatures: Variable, edgeFeatures: Optional[Variable], edgeI: STen, edgeJ: STen, vertexPoolingIndices: Optional[STen] = None,
                 _adjacencies: Optional[dict] = None):
        self.nodeFeatures, self.edgeFeatures, self.edgeI, self.edgeJ, self.vertexPoolingIndices = nodeFeatures, edgeFeatures, edgeI, edgeJ, vertexPoolingIndices
        self._adjacencies = _adjacencies if _adjacencies is not None else {}

    def copy(self, nodeFeatures: Optional[Variable] = None) -> "Graph":
        return Graph(nodeFeatures if nodeFeatures is not None else self.nodeFeatures, self.edgeFeatures, self.edgeI, self.edgeJ, self.vertexPoolingIndices,
                     self._adjacencies)

    def adjacency(self, dtype=None) -> Adjacency:
        x = self.nodeFeatures.value
        key = (x.shape[0], x.dtype if dtype is None else dtype)
        if key not in self._adjacencies:
            self._adjacencies[key] = computeAdjacency(self.edgeI, self.edgeJ, key[0], key[1])
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


def VertexPooling(x: Graph, pooling: str) -> Variable:
    """VertexPooling(graph, Sum | Mean) (VertexPooling.scala): node features summed (averaged) per value of vertexPoolingIndices"""
    assert pooling in ("Sum", "Mean"), pooling
    idx = x.vertexPoolingIndices
    maxi = int(idx.castToDouble().maxAll().item()) + 1              # the max reduction exists for floating types; exact below 2^53
    total = x.nodeFeatures.indexAdd(const(idx), 0, maxi)
    if pooling == "Sum":
        return total
    v = x.nodeFeatures.value
    ones = const(STen.ones([v.shape[0], 1], v.dtype, v.device))
    return total / ones.indexAdd(const(idx), 0, maxi)
