"""f64 torch restatement of lamp.nn.bert (lamp-core/src/main/scala/lamp/nn/bert/bert.scala).

The input embedding, the masked-language-model gather and the two losses are plain torch functions whose gradients come from torch's
autograd: `F.embedding(..., padding_idx=0)` for both tables (the padding id the reference's Embedding op passes, so row 0 receives no
gradient), the positional table sliced to the sequence, and the gather of `encoded.view(-1, D)` at `positions.view(-1)` exactly as
bert.scala:317-331 writes it - no b * T offset - with the intended per-row form beside it.  The transformer blocks are the oracle's
TransformerEncoderBlock (oracle/lamp_transformer_oracle.py), as tests/test_transformer.py uses it; `TorchOp` carries a torch function
into the oracle's graph so that one backprop runs through both."""
import torch
import torch.nn.functional as TF

from oracle import lamp_oracle as O
from oracle import lamp_transformer_oracle as T

F64 = torch.float64


# ---- plain torch -----------------------------------------------------------------------------------------------------------------------------------
def embedding(tokens, segments, tokenWeight, segmentWeight, positional):
    """(tokenWeight[tokens] + segmentWeight[segments]) + positional[:, :T]; positional is [1, L, D]"""
    t = tokens.shape[1]
    return (TF.embedding(tokens, tokenWeight, padding_idx=0) + TF.embedding(segments, segmentWeight, padding_idx=0)) + positional[:, :t]


def embedding_with_any_index(tokens, segments, tokenWeight, segmentWeight, positional):
    """the same with the library's rule for an index: a negative one wraps once, one that is still outside reads as a row of zeros, and
    in the gradient only an index inside [0, V) that is not 0 counts (lamp_embedding_backward compares without wrapping)"""
    def rows(idx, w):
        wrapped = torch.where(idx < 0, idx + w.shape[0], idx)
        inside = (wrapped >= 0) & (wrapped < w.shape[0])
        value = w.detach()[wrapped.clamp(0, w.shape[0] - 1)] * inside.unsqueeze(-1)
        counted = (idx > 0) & (idx < w.shape[0])
        grad_path = w[idx.clamp(0, w.shape[0] - 1)] * counted.unsqueeze(-1)
        return value + (grad_path - grad_path.detach())
    return (rows(tokens, tokenWeight) + rows(segments, segmentWeight)) + positional[:, :tokens.shape[1]]


def embedding_gradients(dout, tokens, segments, V, Vs, L, longRow=None):
    """the three gradients of `embedding_with_any_index` given dout [B, T, D], every sum written out in ascending order of the flat position
    (the tables) and of the batch row (the positional table), so that the order of the additions is part of the restatement:
    (dToken [V, D], dSegment [Vs, D], dPositional [1, L, D]), in dout's type.  longRow: a row of more occurrences is the sum, in chunk
    order, of the ascending sums of its chunks of longRow positions - the order of the library's fused kernels."""
    b, t, d = dout.shape
    flat = dout.reshape(-1, d)

    def table(idx, rows):
        idx = idx.reshape(-1)
        g = torch.zeros(rows, d, dtype=dout.dtype)
        where = {}
        for n in torch.nonzero((idx > 0) & (idx < rows)).view(-1).tolist():
            where.setdefault(int(idx[n]), []).append(n)
        for r, ns in where.items():
            chunk = longRow if longRow is not None and len(ns) > longRow else len(ns)
            for start in range(0, len(ns), chunk):
                part = torch.zeros(d, dtype=dout.dtype)
                for n in ns[start:start + chunk]:
                    part += flat[n]
                g[r] += part
        return g
    dpos = torch.zeros(1, L, d, dtype=dout.dtype)
    for row in range(b):
        dpos[0, :t] += dout[row]
    return table(tokens, V), table(segments, Vs), dpos


def mlm_gather(encoded, positions, perRowPositions=False):
    """encoded [B, T, D], positions [B, P] -> [B, P, D].  As written (bert.scala:319-329): rows positions.view(-1) of encoded.view(-1, D),
    so every batch row reads among the first T rows, which are batch row 0's.  perRowPositions: row b reads its own rows."""
    b, t, d = encoded.shape
    index = positions + (torch.arange(b).view(b, 1) * t if perRowPositions else 0)
    return encoded.reshape(-1, d).index_select(0, index.reshape(-1)).view(b, positions.shape[1], d)


class TorchOp(O.Op):
    """fn(*tensors) with torch's own gradient as one node of the oracle's graph"""
    def __init__(self, fn, inputs):
        leaves = [v.value.detach().clone().requires_grad_(True) for v in inputs]
        with torch.enable_grad():
            out = fn(*leaves)
        cache = {}

        def back(i):
            def f(p, o):
                if "g" not in cache:
                    cache["g"] = torch.autograd.grad(out, leaves, p, allow_unused=True)
                if cache["g"][i] is not None:
                    o.add_(cache["g"][i])
            return f
        self.params = [(v, back(i)) for i, v in enumerate(inputs)]
        self.value = O.Variable(out.detach(), self)


# ---- modules -----------------------------------------------------------------------------------------------------------------------------------------
class BertEncoder(O.Module):          # bert.scala:385-407
    def __init__(self, tokenWeight, segmentWeight, positional, blocks):
        self.tokenWeight, self.segmentWeight, self.positional, self.blocks = tokenWeight, segmentWeight, positional, blocks

    def state(self): return [self.tokenWeight, self.segmentWeight, self.positional] + [s for b in self.blocks for s in b.state()]

    def forward(self, tokens, segments, maxLength=None):
        x = TorchOp(lambda tw, sw, pe: embedding(tokens, segments, tw, sw, pe), [self.tokenWeight, self.segmentWeight, self.positional]).value
        if maxLength is not None and maxLength.dim() == 1:
            # one length per sequence (the batch builder's tokenMaxLength): the same length for every query, the [B, T] form that
            # multiheadAttention's repeat(numHeads, 1) is written for (a 1-D tensor would become [numHeads, B], which no mask accepts)
            maxLength = maxLength.view(-1, 1).expand(tokens.shape[0], tokens.shape[1]).contiguous()
        for b in self.blocks:
            x = b.forward(x, maxLength)
        return x


class MaskedLanguageModel(O.Module):  # bert.scala:312-359: Linear -> relu -> LayerNorm (no scale, no bias) -> Linear
    def __init__(self, w1, b1, w2, b2, perRowPositions=False):
        self.w1, self.b1, self.w2, self.b2, self.perRowPositions = w1, b1, w2, b2, perRowPositions

    def state(self): return [self.w1, self.b1, self.w2, self.b2]

    def forward(self, encoded, positions):
        at = TorchOp(lambda e: mlm_gather(e, positions, self.perRowPositions), [encoded]).value
        h = (self.b1 + T.mm1(at, self.w1)).relu()
        return self.b2 + T.mm1(T.layer_norm(h, [h.shape[-1]]), self.w2)


class BertPretrain(O.Module):         # bert.scala:209-230
    def __init__(self, encoder, mlm, c1, cb1, c2, cb2):
        self.encoder, self.mlm, self.c1, self.cb1, self.c2, self.cb2 = encoder, mlm, c1, cb1, c2, cb2

    def state(self): return self.encoder.state() + self.mlm.state() + [self.c1, self.cb1, self.c2, self.cb2]

    def forward(self, tokens, segments, positions, maxLength=None):
        encoded = self.encoder.forward(tokens, segments, maxLength)
        scores = self.mlm.forward(encoded, positions).logSoftMax(2)
        cls = O.Select(encoded, 1, 0).value
        whole = (self.cb2 + (self.cb1 + cls.mm(self.c1)).tanh().mm(self.c2)).view([-1])
        return encoded, scores, whole


class BertLoss(O.Module):             # bert.scala:42-63, 129-139
    def __init__(self, pretrain, padToken):
        self.pretrain, self.padToken = pretrain, padToken

    def state(self): return self.pretrain.state()

    def forward(self, tokens, segments, positions, maxLength, mlmTarget, wholeSentenceTarget):
        _, scores, whole = self.pretrain.forward(tokens, segments, positions, maxLength)
        weights = torch.ones(scores.shape[-1], dtype=scores.value.dtype)
        l1 = scores.flatten(0, 1).nllLoss(mlmTarget.reshape(-1), weights, 1, self.padToken)
        l2 = TorchOp(lambda w: TF.binary_cross_entropy_with_logits(w, wholeSentenceTarget.to(w.dtype), reduction="mean"), [whole]).value
        return l1 + l2
