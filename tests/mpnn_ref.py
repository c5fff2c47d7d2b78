"""f64 torch restatement of MPNN's message and MPNN.aggregate (lamp-core/src/main/scala/lamp/nn/graph/MPNN.scala:21-25, 75-126).  The
degree factors are computed as the reference computes them: the count is an integer tensor, its pow is an f32 tensor (torch's type
promotion, the same in ATen), and that is cast to the message's type.  Gradients come from torch's autograd, which gives the true
gradient of nodeFeatures as the source of both gathers."""
import torch

F64 = torch.float64


def count_occurences(t, elems):
    """MPNN.countOccurences: ones added into zeros(elems) at t, in t's (integer) type"""
    return torch.zeros(elems, dtype=t.dtype).index_add(0, t, torch.ones_like(t))


def message(x, edgeFeatures, edgeI, edgeJ):
    """cat(edgeFeatures, x[edgeI], x[edgeJ]) along the columns: [E, Fe + 2 D]"""
    return torch.cat([edgeFeatures, x[edgeI.long()], x[edgeJ.long()]], 1)


def degree_factor(index, n, p, dtype=F64):
    """countOccurences(index, n).pow(p).castToType(dtype); the pow of a long tensor is f32"""
    f = count_occurences(index.long(), n).pow(p)
    assert f.dtype == torch.float32
    return f.to(dtype)


def aggregate(numVertices, msg, edgeI, edgeJ, degreeNormalizeI, degreeNormalizeJ, aggregateJ, dtype=None):
    """MPNN.aggregate in f64; `dtype` is the type the factors are cast to before they are widened (the type of the library's message)"""
    p = -0.5 if degreeNormalizeI and degreeNormalizeJ else -1.0
    dtype = dtype or msg.dtype
    ei, ej = edgeI.long(), edgeJ.long()
    m = msg.to(F64)
    if degreeNormalizeI:
        m = m * degree_factor(ei, numVertices, p, dtype).to(F64)[ei].view(-1, 1)
    if degreeNormalizeJ:
        m = m * degree_factor(ej, numVertices, p, dtype).to(F64)[ej].view(-1, 1)
    zeros = torch.zeros(numVertices, m.shape[1], dtype=F64)
    out = zeros.index_add(0, ej, m)
    if aggregateJ:
        out = out + zeros.index_add(0, ei, m)
    return out
