"""lamp.data.GraphBatchStream on the GPU (lamp_amd.graphbatch): the collated batch against the reference's fold out of existing
operators, bit for bit, with the groupings it carries against computeAdjacency / computeEdgeCsr on the fold's edge list; the graph
layers on a collated batch against the same layers on a Graph built from its raw edge lists; the launch budget; the SegmentPool node
against the f64 restatement; a small training run; the reference's known answer; singleLargeGraph.

SegmentPool's bound is the project's rule e_f <= 4 * e_c + FLOOR_EPS * eps (tests/test_graph_gpu.py): e_c / e_f are the max-abs errors of
the composed VertexPooling (IndexAdd) and of the fused node against tests/graph_ref.py::vertex_pooling in f64, over the restatement's
max magnitude.  The floor starts from that file's 2 eps; the fused form's own roundings beyond the sum are at most one, Mean's division.
Measured on an MI355X (test_segment_pool prints the figures with -s), max over value and gradient, "needed" = (e_f - 4 e_c) / eps where
positive; "long" is graphs of longRow(), longRow() + 1, 2 longRow() + 3 and 1 nodes:
  case       pooling  f32 e_c   f32 e_f   needed   f64 e_c   f64 e_f   needed
  n5_1_4_w6  Sum      8.03e-08  4.72e-08  0.00     7.03e-17  0.00e+00  0.00
  n5_1_4_w6  Mean     7.20e-08  4.29e-08  0.00     6.39e-17  0.00e+00  0.00
  long_w1    Sum      8.90e-07  5.20e-07  0.00     1.42e-15  1.18e-15  0.00
  long_w1    Mean     2.52e-08  6.89e-09  0.00     1.52e-17  1.36e-17  0.00
  long_w6    Sum      9.50e-07  5.97e-07  0.00     2.97e-15  1.46e-15  0.00
  long_w6    Mean     5.13e-09  5.32e-09  0.00     1.71e-17  1.33e-17  0.00
  long_w65   Sum      1.37e-06  5.85e-07  0.00     2.86e-15  2.96e-15  0.00
  long_w65   Mean     1.89e-08  1.62e-08  0.00     4.39e-17  4.09e-17  0.00
  long_w260  Sum      2.67e-06  8.02e-07  0.00     4.49e-15  1.44e-15  0.00
  long_w260  Mean     2.05e-08  1.16e-08  0.00     4.42e-17  1.48e-17  0.00
No case needs a floor, so twice the measured need is 0 and the floor stays at 2 eps, for a shape on which the chain happens to be exact
while the fused form rounds (Sum's gradient is a copy in both forms: both errors are exactly 0).

One check here asks for bitwise equality against a yardstick that is itself not reproducible on an MI355X, because it runs IndexAdd,
whose additions are atomic and land in the order the hardware schedules them:
  - test_training_loss_is_the_chain_s_bit_for_bit: with the pooling forced to the composed path (IndexAdd), five runs of the chain gave
    two loss sequences (the seventh loss 0.518619955 three times, 0.518619895 twice) and five runs over collated batches the same two
    plus a third (the fifth loss 0.576894403 once).  With the SegmentPool node, five runs over collated batches gave one sequence, the
    chain's more frequent one.
It is kept at the bound it states, zero; it passes when the atomics happen to land in the same order in both runs.
test_training_is_reproducible_with_segment_pool checks the same claim on the kernels that have no atomics.
GraphAttention's gradients had the same trouble while its two key gathers were IndexSelect nodes, whose closure is an IndexAdd (four backward
passes over one raw Graph differed from the first by up to 4.2e-09 in the gradients of nodeFeatures and wNodeKey2); on the fused path they
are GraphGather nodes now, summed over the edge CSR in its order, and test_layer_gradients_on_a_collated_batch holds bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from lamp_amd import autograd as A, graph as G, nn, sten as S
from lamp_amd._capi import lib
from lamp_amd.data import JavaRandom
from lamp_amd.graphbatch import GraphBatchStream, GraphSet, graphBatchFused, graphBatchPlan
from tests import graph_batch_ref as BR, graph_ref as R
from tests.test_graph_batch import check_kat, kat_graphs
from tests.util import closed_form, to_sten, to_torch, TORCH2LAMP

pytestmark = pytest.mark.gpu
F64 = torch.float64
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
FLOOR_EPS = 2


class Order:
    """an `rng` whose shuffle returns a given order (smallGraphStream takes anything with shuffle)"""

    def __init__(self, order): self.order = list(order)

    def shuffle(self, xs): return list(self.order)


def _edges(n, e, salt=0):
    """e edges among n >= 2 nodes without self loops, unsorted, with repeats"""
    k = torch.arange(e, dtype=torch.int64) + salt
    i = (k * 3 + 1) % n
    return i, (i + 1 + k % (n - 1)) % n


def _hub(n):
    """node 0 joined to all n - 1 others, directions alternating"""
    k = torch.arange(1, n, dtype=torch.int64)
    zero = torch.zeros_like(k)
    return torch.where(k % 2 == 1, zero, k), torch.where(k % 2 == 1, k, zero)


def _graphs(nodes, edges, width, dt, edgeShape=(), hub=None):
    """per graph (nodeFeatures [n, width], edgeFeatures [e, *edgeShape], edgeI, edgeJ) in torch, closed-form features; graph `hub` is a star"""
    out = []
    for g, (n, e) in enumerate(zip(nodes, edges)):
        i, j = _hub(n) if g == hub else (_edges(n, e, g) if e else (torch.zeros(0, dtype=torch.int64),) * 2)
        assert i.numel() == e
        out.append((closed_form((n, width), 11 + g, 2.0, dt), closed_form((e,) + tuple(edgeShape), 101 + g, 2.0, dt), i, j))
    return out


def _set(graphs):
    return GraphSet([GraphBatchStream.Graph(*(to_sten(t) for t in g)) for g in graphs])


def _stream(graphSet, order, mb, fused, target=None):
    prev = graphBatchFused(fused)
    try:
        target = target if target is not None else to_sten(torch.arange(graphSet.numGraphs, dtype=F64) * 0.5)
        return list(GraphBatchStream.smallGraphStream(mb, graphSet, target, Order(order)))
    finally:
        graphBatchFused(prev)


def _assert_same_batch(fused, chain, what):
    (fg, ft), (cg, ct) = fused, chain
    n = cg.nodeFeatures.value.shape[0]
    dt = cg.nodeFeatures.value.dtype
    eq = lambda a, b, name: (a.shape == b.shape and torch.equal(to_torch(a), to_torch(b))) or pytest.fail(f"{what}: {name} differs: {a.shape} vs {b.shape}")
    eq(fg.nodeFeatures.value, cg.nodeFeatures.value, "nodeFeatures")
    eq(fg.edgeFeatures.value, cg.edgeFeatures.value, "edgeFeatures")
    eq(fg.edgeI, cg.edgeI, "edgeI")
    eq(fg.edgeJ, cg.edgeJ, "edgeJ")
    eq(fg.vertexPoolingIndices, cg.vertexPoolingIndices, "vertexPoolingIndices")
    eq(ft, ct, "target")
    assert cg.graphPtr is None and cg._adjacencies == {}, what
    # the groupings are in the batch's caches already, under the keys Graph.adjacency() / Graph.edgeCsr() use
    assert set(fg._adjacencies) == {(n, dt), ("edgeCsr", n)}, (what, list(fg._adjacencies))
    adj, ref = fg.adjacency(), G.computeAdjacency(cg.edgeI, cg.edgeJ, n, dt)
    for name in ("rowptr", "col", "dinv"):
        eq(getattr(adj, name), getattr(ref, name), "adjacency " + name)
    csr, ref = fg.edgeCsr(), G.computeEdgeCsr(cg.edgeI, cg.edgeJ, n)
    for name in ("inRowptr", "inPerm", "outRowptr", "outPerm"):
        eq(getattr(csr, name), getattr(ref, name), "edgeCsr " + name)
    pool = to_torch(fg.vertexPoolingIndices)
    counts = torch.bincount(pool) if pool.numel() else torch.zeros(0, dtype=torch.int64)
    assert to_torch(fg.graphPtr).tolist() == [0] + torch.cumsum(counts, 0).tolist(), what


def _check(graphs, order, mb, what):
    graphSet = _set(graphs)
    fused, chain = _stream(graphSet, order, mb, True), _stream(graphSet, order, mb, False)
    plan = graphBatchPlan([g[0].shape[0] for g in graphs], [g[2].numel() for g in graphs], order, mb)
    assert len(fused) == len(chain) == len(plan.offsets)
    for k, (f, c) in enumerate(zip(fused, chain)):
        _assert_same_batch(f, c, f"{what} batch {k}")
        b, nb, eb = plan.totals[k].tolist()
        assert f[0].nodeFeatures.value.shape[0] == nb and f[0].edgeI.shape == [eb] and f[1].shape[0] == b, (what, k)
        # and against the torch restatement of the fold
        ids = list(order)[int(plan.offsets[k]):int(plan.offsets[k]) + b]
        ref = BR.fold(graphs, ids, torch.arange(len(graphs), dtype=F64) * 0.5)
        assert torch.equal(to_torch(f[0].edgeI), ref["edgeI"]) and torch.equal(to_torch(f[0].nodeFeatures.value), ref["nodeFeatures"]), (what, k)
        assert torch.equal(to_torch(f[1]), ref["target"]), (what, k)
    return fused, chain


def test_collate_one_graph(gpu):
    _check(_graphs((4,), (3,), 4, torch.float32, (2,)), [0], 1, "B = 1")


def test_collate_out_of_order(gpu):
    _check(_graphs((5, 1, 4), (5, 0, 3), 4, torch.float32, (2,)), [2, 0, 1], 3, "out of order")


def test_collate_no_edges_at_all(gpu):
    _check(_graphs((3, 1, 2), (0, 0, 0), 4, torch.float32, (2,)), [1, 2, 0], 3, "no edges")


def test_collate_same_graph_twice(gpu):
    _check(_graphs((5, 1, 4), (5, 0, 3), 4, torch.float32, (2,)), [2, 2, 0], 3, "a graph twice")


def test_collate_hub_beside_one_node(gpu):
    n = 2 * G.longRow() + 4
    _check(_graphs((n, 1), (n - 1, 0), 4, torch.float32, (2,), hub=0), [1, 0], 2, "hub")


@pytest.mark.parametrize("dt,width", [(torch.float32, w) for w in (1, 3, 4, 65, 260)] + [(torch.float64, w) for w in (1, 2, 3, 130)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_collate_widths(gpu, dt, width):
    """packet widths 1 / 2 / 4 of either type, and rows of more packets than a wave has lanes"""
    _check(_graphs((5, 1, 4), (5, 0, 3), width, dt, (width,)), [2, 0, 1], 3, f"width {width}")


@pytest.mark.parametrize("edgeShape", [(), (3,)], ids=["E", "Ex3"])
def test_collate_edge_feature_shapes(gpu, edgeShape):
    fused, _ = _check(_graphs((5, 1, 4), (5, 0, 3), 2, torch.float64, edgeShape), [0, 1, 2], 3, f"edge features {edgeShape}")
    assert fused[0][0].edgeFeatures.value.shape == [8] + list(edgeShape)


def test_collate_every_batch_of_an_epoch(gpu):
    """seven graphs in a shuffled order, minibatch 3: two full batches and a short last one, each against the chain and the plan"""
    nodes, edges = (5, 1, 4, 7, 2, 3, 6), (5, 0, 3, 9, 1, 0, 8)
    order = JavaRandom(3).shuffle(list(range(7)))
    fused, _ = _check(_graphs(nodes, edges, 3, torch.float32, ()), order, 3, "epoch")
    assert [f[1].shape[0] for f in fused] == [3, 3, 1]


def test_stream_protocol(gpu):
    """numBatches, nextBatch() to the end, reset() replays the same order; without an rng the order is 0 .. G - 1"""
    graphs = _graphs((5, 1, 4, 2), (5, 0, 3, 1), 2, torch.float32, ())
    target = to_sten(torch.tensor([10.0, 11.0, 12.0, 13.0]))
    stream = GraphBatchStream.smallGraphStream(3, [GraphBatchStream.Graph(*(to_sten(t) for t in g)) for g in graphs], target, None, transferBufferSize=10000)
    assert stream.numBatches == 2
    first = [to_torch(t).tolist() for _, t in stream]
    assert first == [[10.0, 11.0, 12.0], [13.0]] and stream.nextBatch() is None
    stream.reset()
    assert [to_torch(t).tolist() for _, t in stream] == first
    shuffled = GraphBatchStream.smallGraphStream(3, stream.set, target, JavaRandom(5))
    want = JavaRandom(5).shuffle(list(range(4)))
    assert [v for _, t in shuffled for v in to_torch(t).tolist()] == [10.0 + g for g in want]


def test_bad_graph_sets_are_errors(gpu):
    """rejected on the host, before any kernel sees them (an out-of-range endpoint is checked by a comparison kernel that dereferences
    nothing through it, and deliberately not fed to the GPU here)"""
    mk = lambda n, f, e, dt=torch.float32, edt=torch.int64: GraphBatchStream.Graph(to_sten(torch.zeros(n, f, dtype=dt)), to_sten(torch.zeros(e, dtype=dt)),
                                                                                  to_sten(torch.zeros(e, dtype=edt)), to_sten(torch.zeros(e, dtype=edt)))
    good = mk(3, 2, 2)
    with pytest.raises(AssertionError, match="at least one node"):
        GraphSet([good, mk(0, 2, 0)])
    with pytest.raises(AssertionError, match="feature widths"):
        GraphSet([good, mk(3, 4, 2)])
    with pytest.raises(AssertionError, match="feature types"):
        GraphSet([good, mk(3, 2, 2, torch.float64)])
    with pytest.raises(AssertionError, match="int64 vectors"):
        GraphSet([good, mk(3, 2, 2, torch.float32, torch.float32)])
    with pytest.raises(AssertionError, match="differ in length"):
        GraphSet([GraphBatchStream.Graph(good.nodeFeatures, good.edgeFeatures, good.edgeI, to_sten(torch.zeros(3, dtype=torch.int64)))])
    with pytest.raises(AssertionError, match="a row per graph"):
        GraphBatchStream.smallGraphStream(2, [good, good], to_sten(torch.zeros(3)), None)


# ---- the layers on a collated batch -------------------------------------------------------------------------------------------------------------
def _layer_batch():
    n = 2 * G.longRow() + 4
    graphs = _graphs((5, n, 4), (6, n - 1, 5), 8, torch.float32, (2,), hub=1)
    return _stream(_set(graphs), [2, 1, 0], 3, True)[0][0]


def _run_layer(layer, batch, raw):
    """forward and backward of `layer` over the batch (its caches filled) or over a Graph of the batch's raw edge lists -> out, dx, parameter gradients"""
    x = A.param(batch.nodeFeatures.value)
    graph = G.Graph(x, batch.edgeFeatures, batch.edgeI, batch.edgeJ, None) if raw else batch.copy(nodeFeatures=x)
    layer.zeroGrad()
    out = layer.forward(graph).nodeFeatures
    (out * A.const(to_sten(closed_form(tuple(out.shape), 77, 1.0, torch.float32)))).sum().backprop()
    return [to_torch(out.value), to_torch(x.partialDerivative)] + [to_torch(p.partialDerivative) for p in layer.parameters]


@functools.lru_cache(maxsize=None)
def _layer_results(kind):
    """-> (over the collated batch, over the raw Graph), each [out, dx, parameter gradients ...]: one forward and backward pass each"""
    lib.lamp_manual_seed(11)
    if kind == "GCN":
        layer = G.GCN(G.ResidualModule(nn.Linear(8, 8, S.F32, 0, bias=False)))
    elif kind == "GraphAttention":
        layer = G.GraphAttention.apply(8, 2, 4, 2, 4)
    else:
        layer = G.MPNN(nn.Linear(2 + 16, 8, S.F32, 0, bias=False), nn.Linear(8 + 8, 8, S.F32, 0, bias=False))
    batch = _layer_batch()
    got, want = _run_layer(layer, batch, raw=False), _run_layer(layer, batch, raw=True)
    assert len(got) == len(want) >= 3
    return got, want


@pytest.mark.parametrize("kind", ["GCN", "GraphAttention", "MPNN"])
def test_layer_values_on_a_collated_batch(gpu, kind):
    """the groupings are equal and the kernels deterministic, so the values are equal bit for bit"""
    got, want = _layer_results(kind)
    assert torch.isfinite(got[0]).all() and torch.equal(got[0], want[0]), f"{kind}: values differ by {(got[0] - want[0]).abs().max().item():.3e}"


@pytest.mark.parametrize("kind", ["GCN", "GraphAttention", "MPNN"])
def test_layer_gradients_on_a_collated_batch(gpu, kind):
    """and so are the gradients of the node features and of every parameter (GraphAttention's key gathers are GraphGather nodes on the fused
    path: no IndexAdd anywhere in the three layers)"""
    got, want = _layer_results(kind)
    for k, (a, b) in enumerate(zip(got[1:], want[1:])):
        assert torch.isfinite(a).all() and torch.equal(a, b), f"{kind}: gradient {k} differs by {(a - b).abs().max().item():.3e}"


def test_attention_node_gradients_on_a_collated_batch(gpu):
    """the GraphAttentionAggregate node alone (the kernels that read the groupings; no IndexAdd) over the batch's collated EdgeCsr and over
    one computed from its raw edge lists: value and both gradients bit for bit"""
    batch = _layer_batch()
    n, e, heads, v = batch.nodeFeatures.value.shape[0], batch.edgeI.shape[0], 2, 4
    results = []
    for csr in (batch.edgeCsr(), G.computeEdgeCsr(batch.edgeI, batch.edgeJ, n)):
        score = A.param(to_sten(closed_form((e, heads), 41, 2.0, torch.float32)))
        value = A.param(to_sten(closed_form((n, heads, v), 43, 2.0, torch.float32)))
        out = G.graphAttentionAggregate(score, value, batch.edgeI, batch.edgeJ, heads, csr)
        (out * A.const(to_sten(closed_form((n, heads * v), 47, 1.0, torch.float32)))).sum().backprop()
        results.append([to_torch(out.value), to_torch(score.partialDerivative), to_torch(value.partialDerivative)])
    for a, b in zip(*results):
        assert torch.isfinite(a).all() and a.abs().max() > 0 and torch.equal(a, b)


# ---- the launch budget ------------------------------------------------------------------------------------------------------------------------
def _timer_counts(fn):
    lib.lamp_device_synchronize()
    buf = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_report(buf, len(buf))            # clears the log
    lib.lamp_kernel_timer_enable(1)
    try:
        fn()
        lib.lamp_device_synchronize()
    finally:
        lib.lamp_kernel_timer_enable(0)
    lib.lamp_kernel_timer_report(buf, len(buf))
    counts = {}
    for line in buf.value.decode().splitlines():
        f = line.split()
        counts[f[0]] = int(f[1])
    return counts


GROUPING_KERNELS = ("gcn_index_range", "gcn_rowptr_dinv", "graph_index_range", "graph_edge_rowptr")


@pytest.mark.parametrize("B", [64, 3])
def test_launch_budget(gpu, B):
    """one nextBatch(): two row gathers, at most two index launches, at most five kernels in all whatever B, and a gcn layer over the batch
    builds nothing; with graphBatchFused(False) no graph_batch kernel runs and the layer groups the batch itself"""
    nodes = [3 + k % 5 for k in range(B)]
    graphSet = _set(_graphs(nodes, [n + 1 for n in nodes], 8, torch.float32, (2,)))
    graphSet.adjacency(), graphSet.edgeCsr()                # once per data set, not per batch
    target = to_sten(torch.arange(B, dtype=torch.float32))
    layer = G.gcn(8, 8, S.F32, 0)
    stream = GraphBatchStream.smallGraphStream(B, graphSet, target, JavaRandom(1))
    got = []
    counts = _timer_counts(lambda: got.append(stream.nextBatch()))
    print(f"B = {B}: nextBatch {counts}")
    assert counts.get("graph_batch_rows", 0) == 2 and 1 <= counts.get("graph_batch_index", 0) <= 2, counts
    assert sum(counts.values()) <= 5, counts
    forward = _timer_counts(lambda: layer.forward(got[0][0]))
    assert forward.get("gcn_aggregate", 0) == 1 and not any(k in forward for k in GROUPING_KERNELS), forward
    prev = graphBatchFused(False)
    try:
        stream.reset()
        chain = _timer_counts(lambda: got.append(stream.nextBatch()))
        forward = _timer_counts(lambda: layer.forward(got[1][0]))
    finally:
        graphBatchFused(prev)
    assert not any(k.startswith("graph_batch") for k in chain), chain
    assert forward.get("gcn_rowptr_dinv", 0) == 1 and forward.get("gcn_aggregate", 0) == 1, forward


# ---- SegmentPool ------------------------------------------------------------------------------------------------------------------------------
def _pool_sizes(name):
    if name == "n5_1_4":
        return (5, 1, 4)
    l = G.longRow()
    return (l, l + 1, 2 * l + 3, 1)


POOL_CASES = [("n5_1_4", 6)] + [("long", w) for w in (1, 6, 65, 260)]


@functools.lru_cache(maxsize=None)
def _pool_problem(name, width, dt, pooling):
    sizes = _pool_sizes(name)
    n = sum(sizes)
    rd = lambda t: t.to(dt).to(F64)
    x, lf = rd(closed_form((n, width), 5, 2.0, F64)), rd(closed_form((len(sizes), width), 303, 1.0, F64))
    idx = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    xr = x.clone().requires_grad_(True)
    out = R.vertex_pooling(xr, idx, pooling)
    (out * lf).sum().backward()
    return sizes, x, lf, idx, {"out": out.detach(), "dx": xr.grad.detach()}


def _pool_library(name, width, dt, pooling, fused):
    sizes, x, lf, idx, _ = _pool_problem(name, width, dt, pooling)
    xv = A.param(to_sten(x.to(dt)))
    ptr = to_sten(torch.tensor([0] + np.cumsum(sizes).tolist())) if fused else None
    one = to_sten(torch.tensor([0]))
    out = G.VertexPooling(G.Graph(xv, None, one, one, to_sten(idx), graphPtr=ptr), pooling)
    (out * A.const(to_sten(lf.to(dt)))).sum().backprop()
    return {"out": to_torch(out.value), "dx": to_torch(xv.partialDerivative)}


def _err(got, ref):
    assert list(got.shape) == list(ref.shape), f"shape {list(got.shape)} vs {list(ref.shape)}"
    den = ref.abs().max().item()
    return (got.double() - ref).abs().max().item() / (den if den > 0 else 1.0)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("pooling", ["Sum", "Mean"])
@pytest.mark.parametrize("name,width", POOL_CASES, ids=[f"{n}_w{w}" for n, w in POOL_CASES])
def test_segment_pool(gpu, name, width, pooling, dt):
    """value and gradient: e_f <= 4 * e_c + FLOOR_EPS * eps, and the fused node's bits are the same from run to run.  Figures are printed (-s)."""
    ref = _pool_problem(name, width, dt, pooling)[-1]
    comp, fus, again = (_pool_library(name, width, dt, pooling, f) for f in (False, True, True))
    floor = FLOOR_EPS * EPS[dt]
    for key, r in ref.items():
        e_c, e_f = _err(comp[key], r), _err(fus[key], r)
        print(f"POOL {name}_w{width} {pooling} {key} {str(dt)[6:]}: e_c {e_c:.3e} e_f {e_f:.3e} needed {max(0.0, e_f - 4 * e_c) / EPS[dt]:.2f} eps")
        assert e_f <= 4 * e_c + floor, f"{key}: fused error {e_f:.3e} > 4 * composed error {e_c:.3e} + {floor:.1e}"
        assert torch.equal(fus[key], again[key]), f"{key}: two runs of the fused node differ"


def test_segment_pool_needs_graph_ptr(gpu):
    """with graphPtr the SegmentPool kernels run and no index_add; without it, or with graphBatchFused(False), the composed path runs"""
    fused = _timer_counts(lambda: _pool_library("n5_1_4", 6, torch.float32, "Mean", True))
    assert fused.get("segment_pool", 0) == 1 and fused.get("segment_pool_backward", 0) == 1 and "index_add" not in fused, fused
    composed = _timer_counts(lambda: _pool_library("n5_1_4", 6, torch.float32, "Mean", False))
    assert composed.get("index_add", 0) >= 1 and not any(k.startswith("segment_pool") for k in composed), composed
    prev = graphBatchFused(False)
    try:
        off = _timer_counts(lambda: _pool_library("n5_1_4", 6, torch.float32, "Mean", True))
    finally:
        graphBatchFused(prev)
    assert off.get("index_add", 0) >= 1 and not any(k.startswith("segment_pool") for k in off), off


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def _planted_graphs():
    """64 graphs of 6 - 12 nodes, two classes: class 0 a ring with features of unit noise - 0.5, class 1 a star with + 0.5; fixed seed"""
    g = torch.Generator().manual_seed(31)
    graphs, labels = [], []
    for k in range(64):
        n, label = 6 + int(torch.randint(0, 7, (1,), generator=g)), k % 2
        x = torch.randn(n, 8, generator=g) + (label - 0.5)
        a = torch.arange(n, dtype=torch.int64)
        i, j = (a, (a + 1) % n) if label == 0 else (torch.zeros(n - 1, dtype=torch.int64), a[1:])
        graphs.append((x.float(), torch.ones(i.numel()), i, j))
        labels.append(label)
    return graphs, torch.tensor(labels)


def _train(fused, composedPooling, epochs=6):
    graphs, labels = _planted_graphs()
    prev = graphBatchFused(fused)
    try:
        lib.lamp_manual_seed(7)
        layers, head = [G.gcn(8, 16, S.F32, 0), G.gcn(16, 16, S.F32, 0)], nn.Linear(16, 2, S.F32, 0)
        params = [p for m in layers + [head] for p in m.parameters]
        opt = nn.AdamW([p.value for p in params], 0.0, 0.01)
        stream = GraphBatchStream.smallGraphStream(16, _set(graphs), to_sten(labels), JavaRandom(9))
        weights = S.STen.ones([2], S.F32)

        def logits(batch):
            g = batch
            for layer in layers:
                g = layer.forward(g)
            if composedPooling:     # the same pooling code whatever collated the batch
                g = G.Graph(g.nodeFeatures, g.edgeFeatures, g.edgeI, g.edgeJ, g.vertexPoolingIndices, g._adjacencies)
            return head.forward(G.VertexPooling(g, "Mean")).logSoftMax(1)

        losses = []
        for _ in range(epochs):
            stream.reset()
            for batch, target in stream:
                for m in layers + [head]:
                    m.zeroGrad()
                loss = logits(batch).nllLoss(target, weights)
                loss.backprop()
                opt.step([p.partialDerivative for p in params])
                losses.append(loss.value.item())
        stream.reset()
        hits = sum(int((to_torch(logits(batch).value).argmax(1) == to_torch(target)).sum()) for batch, target in stream)
        return losses, hits / 64.0
    finally:
        graphBatchFused(prev)


def test_small_graph_training(gpu):
    """smallGraphStream(16) -> two gcn layers -> VertexPooling(Mean) -> Linear -> logSoftMax, NLL, AdamW, f32: the loss falls and the training
    accuracy exceeds the majority class (the classes are balanced: 0.5)"""
    losses, acc = _train(True, False)
    first, last = float(np.mean(losses[:4])), float(np.mean(losses[-4:]))
    print(f"epoch loss {first:.4f} -> {last:.4f}, training accuracy {acc:.3f}")
    assert len(losses) == 24 and all(np.isfinite(losses)) and last < first, losses
    assert acc > 0.5, acc


def test_training_loss_is_the_chain_s_bit_for_bit(gpu):
    """with the pooling forced to the composed path in both runs, the collated batches give the loss sequence of the reference's fold, bit for
    bit.  The composed pooling is an IndexAdd, whose atomics do not repeat their own bits from run to run, chain against chain included:
    see the head of the file for the figures."""
    fused, _ = _train(True, True, epochs=2)
    chain, _ = _train(False, True, epochs=2)
    assert fused == chain, [(a, b) for a, b in zip(fused, chain) if a != b][:3]


def test_training_is_reproducible_with_segment_pool(gpu):
    """collated batches pooled by the SegmentPool node: no kernel of the step has an atomic, so two runs give the same losses bit for bit"""
    first, _ = _train(True, False, epochs=2)
    again, _ = _train(True, False, epochs=2)
    assert first == again, [(a, b) for a, b in zip(first, again) if a != b][:3]


def test_reference_known_answer(gpu):
    """gcn.test.scala "small graph mode batchstream" through smallGraphStream(2, ..., rng); holds for either order of the two graphs"""
    for fused in (True, False):
        prev = graphBatchFused(fused)
        try:
            graphs = [GraphBatchStream.Graph(*(to_sten(t) for t in g)) for g in kat_graphs()]
            stream = GraphBatchStream.smallGraphStream(2, graphs, to_sten(torch.tensor([0.0, 1.0], dtype=F64)), JavaRandom(1234), 10000)
            graph, target = stream.nextBatch()
            assert stream.nextBatch() is None and stream.numBatches == 1
            check_kat({"nodeFeatures": to_torch(graph.nodeFeatures.value), "edgeI": to_torch(graph.edgeI),
                       "vertexPoolingIndices": to_torch(graph.vertexPoolingIndices), "target": to_torch(target)})
            assert (graph.graphPtr is not None) == fused
        finally:
            graphBatchFused(prev)


def test_single_large_graph(gpu):
    """one batch, holding the graph's tensors and the target unchanged"""
    x, e, i, j = (to_sten(t) for t in _graphs((6,), (7,), 3, torch.float32, ())[0])
    target = to_sten(torch.arange(6, dtype=torch.float32))
    stream = GraphBatchStream.singleLargeGraph(GraphBatchStream.Graph(x, e, i, j), target)
    assert stream.numBatches == 1
    graph, t = stream.nextBatch()
    assert stream.nextBatch() is None
    assert graph.nodeFeatures.value.data_ptr == x.data_ptr and graph.edgeFeatures.value.data_ptr == e.data_ptr
    assert graph.edgeI is i and graph.edgeJ is j and t is target and graph.graphPtr is None
    assert graph.vertexPoolingIndices.shape == [1] and to_torch(graph.vertexPoolingIndices).tolist() == [0.0]
    stream.reset()
    assert stream.nextBatch()[1] is target
