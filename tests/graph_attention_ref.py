"""f64 torch restatement of GraphAttention.multiheadGraphAttention (GraphAttention.scala:119-198): the two scoring branches, and the
softmax per destination taken against that destination's own maximum (not the reference's global one: the result is the same in exact
arithmetic, and a destination far below the global maximum does not underflow).  Gradients come from torch's autograd."""
import math

import torch

F64 = torch.float64


def attention_weights(score, edgeJ, n):
    """score [E, H] -> the softmax over the edges that share a destination, [E, H]; the maximum is a constant of the graph (the
    softmax does not depend on it)"""
    e, h = score.shape
    idx = edgeJ.long().unsqueeze(1).expand(e, h)
    m = torch.full((n, h), -math.inf, dtype=F64).scatter_reduce(0, idx, score.detach().to(F64), "amax", include_self=True)
    p = (score.to(F64) - m[edgeJ.long()]).exp()
    s = torch.zeros(n, h, dtype=F64).index_add(0, edgeJ.long(), p)
    return p / s[edgeJ.long()]


def attention_aggregate(score, value, edgeI, edgeJ):
    """score [E, H], value [N, H, V] -> [N, H * V]: per destination the sum of the sources' values under the softmax of the scores; a
    destination without an incoming edge gets zeros"""
    n, h, v = value.shape
    w = attention_weights(score, edgeJ, n)
    return torch.zeros(n, h, v, dtype=F64).index_add(0, edgeJ.long(), w.unsqueeze(2) * value.to(F64)[edgeI.long()]).reshape(n, h * v)


def scores(nodeFeatures, edgeFeatures, edgeI, edgeJ, wNodeKey1, wNodeKey2, wEdgeKey, wNodeValue, wAttention, numHeads):
    """-> (activations [E, H], nodeValue [N, H, V])"""
    mm = lambda a, b: (a.to(F64) @ b.to(F64)).reshape(a.shape[0], numHeads, b.shape[1] // numHeads)
    k1, k2, ek, nv = mm(nodeFeatures, wNodeKey1), mm(nodeFeatures, wNodeKey2), mm(edgeFeatures, wEdgeKey), mm(nodeFeatures, wNodeValue)
    ni, nj = k1[edgeI.long()], k2[edgeJ.long()]
    if wAttention is not None:
        cat = torch.cat([ni, nj, ek], 2)                                          # [E, H, K]
        act = torch.tanh(torch.einsum("ehk,kh->eh", cat, wAttention.to(F64)))
    else:
        act = (ni * nj * (1.0 / math.sqrt(float(numHeads)))).sum(2) + ek.reshape(-1, numHeads)
    return act, nv


def multihead_graph_attention(nodeFeatures, edgeFeatures, edgeI, edgeJ, wNodeKey1, wNodeKey2, wEdgeKey, wNodeValue, wAttention, numHeads):
    act, nv = scores(nodeFeatures, edgeFeatures, edgeI, edgeJ, wNodeKey1, wNodeKey2, wEdgeKey, wNodeValue, wAttention, numHeads)
    return attention_aggregate(act, nv, edgeI, edgeJ)
