"""A torch restatement of the reference's minibatch fold (lamp-data GraphBatchStream.smallGraphStream, GraphBatchStream.scala:42-123):
per selected graph the edge ids plus the running node offset and a vector of the graph's index, then the five cats and the targets of
the selected graphs.  Graphs are (nodeFeatures, edgeFeatures, edgeI, edgeJ) tuples of torch tensors with local edge ids."""
import torch


def fold(graphs, ids, target):
    """-> dict(nodeFeatures, edgeFeatures, edgeI, edgeJ, vertexPoolingIndices, target) of the batch of graphs[i] for i in ids, in that order"""
    offset, edgeI, edgeJ, index = 0, [], [], []
    for b, i in enumerate(ids):
        nodes, _, ei, ej = graphs[i]
        edgeI.append(ei + offset)
        edgeJ.append(ej + offset)
        index.append(torch.zeros(nodes.shape[0], dtype=torch.int64) + b)
        offset += nodes.shape[0]
    return {"nodeFeatures": torch.cat([graphs[i][0] for i in ids], 0), "edgeFeatures": torch.cat([graphs[i][1] for i in ids], 0),
            "edgeI": torch.cat(edgeI, 0), "edgeJ": torch.cat(edgeJ, 0), "vertexPoolingIndices": torch.cat(index, 0),
            "target": target[torch.tensor(list(ids), dtype=torch.int64)]}


def batches(order, minibatchSize):
    """`grouped`: the order cut into groups of minibatchSize, the last possibly short"""
    order = list(order)
    return [order[k:k + minibatchSize] for k in range(0, len(order), minibatchSize)]
