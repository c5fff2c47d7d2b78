"""f64 torch restatement of lamp.nn.graph's GCN path (GCN.scala:30-145, VertexPooling.scala): a dense A + A' + I built with
index_put_(accumulate=True), the degrees, the product; gradients come from torch's autograd."""
import torch

F64 = torch.float64


def dense_adjacency(edgeI, edgeJ, n):
    """A + A' + I, duplicate pairs and pairs given in both directions counted as often as they occur"""
    a = torch.zeros(n, n, dtype=F64)
    if edgeI.numel():
        a.index_put_((edgeI.long(), edgeJ.long()), torch.ones(edgeI.numel(), dtype=F64), accumulate=True)
    return a + a.t() + torch.eye(n, dtype=F64)


def degrees(edgeI, edgeJ, n):
    """(occurrences in edgeI ++ edgeJ) + 1"""
    return torch.bincount(torch.cat([edgeI.long(), edgeJ.long()]), minlength=n).to(F64) + 1.0


def gcn_aggregation(x, edgeI, edgeJ):
    """degrees^-1/2 * ((A + A' + I) mm (x * degrees^-1/2))"""
    n = x.shape[0]
    d = degrees(edgeI, edgeJ, n).pow(-0.5).unsqueeze(1)
    return d * (dense_adjacency(edgeI, edgeJ, n) @ (x.to(F64) * d))


def gcn_linear_relu(x, edgeI, edgeJ, weight, bias):
    """GCN(ResidualModule(Linear(weight, bias) -> relu)): the residual applies only where the shapes agree"""
    m = gcn_aggregation(x, edgeI, edgeJ)
    y = torch.relu(m @ weight.to(F64) + bias.to(F64))
    return y + m if y.shape == m.shape else y


def vertex_pooling(x, index, pooling):
    n = int(index.max().item()) + 1
    total = torch.zeros(n, x.shape[1], dtype=F64).index_add(0, index.long(), x.to(F64))
    if pooling == "Sum":
        return total
    counts = torch.zeros(n, 1, dtype=F64).index_add(0, index.long(), torch.ones(x.shape[0], 1, dtype=F64))
    return total / counts
