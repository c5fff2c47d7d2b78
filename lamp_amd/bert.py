"""lamp.nn.bert and lamp.data.bert over the host C ABI: BertEncoder, MaskedLanguageModelModule, BertPretrainModule, BertLoss, the fused
input embedding and its switch, and the pretraining batch builder.

Reference: lamp-core/src/main/scala/lamp/nn/bert/bert.scala, lamp-data/src/main/scala/lamp/data/bert/package.scala.  Modules whose input
is a tuple / case class in the reference take the same members here, `None` for an absent Option.

The encoder's input embedding tokenEmbedding(tokens) + segmentEmbedding(segments) + positionalEmbedding[:, :T] is one `BertEmbedding` node
over the kernels of csrc/kernels/bert.hip (`bertEmbedding`), or the reference's chain of Embedding, Embedding, Add, Slice and Add;
`bertFused` switches between the two for the node and for every module of this file.

The batch builder is host-side numpy.  It takes a numpy.random.Generator, so its draws differ from scala.util.Random's; its rules are
the reference's.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

from ._capi import lib
from .autograd import Variable, apply_op, const
from .nn import _mk
from .sten import STen, F32
from .transformer import _Multi, _forward_multi


def bertFused(on: bool) -> bool:
    """process-wide: the encoder's input embedding as one BertEmbedding node (True) or as the reference's chain of Embedding, Embedding,
    Add, Slice and Add nodes (False); returns the previous setting"""
    prev = C.c_int(0); lib.lamp_bert_fused(int(bool(on)), C.byref(prev)); return bool(prev.value)


def bertLongRow() -> int:
    """a table row of more occurrences than this is summed in chunks of this many positions (lamp_bert_long_row)"""
    n = C.c_int64(); lib.lamp_bert_long_row(C.byref(n)); return n.value


def bertEmbedding(tokens: Variable, segments: Variable, tokenWeight: Variable, segmentWeight: Variable, positional: Variable) -> Variable:
    """(tokenWeight[tokens] + segmentWeight[segments]) + positional[:, :T]: tokens / segments long [B, T] constants, tokenWeight [V, D],
    segmentWeight [Vs, D], positional [1, L, D] -> [B, T, D].  One BertEmbedding node with bertFused(True), the chain otherwise.  Row 0 of
    both tables receives no gradient either way (the padding id the reference's Embedding passes)."""
    return apply_op("BertEmbedding", [tokens, segments, tokenWeight, segmentWeight, positional])


def bertEmbeddingForward(tokenWeight: STen, segmentWeight: STen, positional: STen, tokens: STen, segments: STen) -> STen:
    o = C.c_void_p(); lib.lamp_bert_embedding_forward(C.byref(o), tokenWeight.h, segmentWeight.h, positional.h, tokens.h, segments.h); return STen(o)


def bertEmbeddingBackward(dout: STen, tokens: STen, segments: STen, V: int, Vs: int, L: int, paddingIdx: int = 0, dToken=True, dSegment=True,
                          dPositional=True) -> Tuple[Optional[STen], Optional[STen], Optional[STen]]:
    """(dToken [V, D], dSegment [Vs, D], dPositional [1, L, D]) of lamp_bert_embedding_backward; an output that is not asked for is None
    and costs no launch"""
    o = [C.c_void_p() for _ in range(3)]
    want = (dToken, dSegment, dPositional)
    lib.lamp_bert_embedding_backward(*[C.byref(p) if w else None for p, w in zip(o, want)], dout.h, tokens.h, segments.h, int(V), int(Vs), int(L),
                                     int(paddingIdx))
    return tuple(STen(p) if w else None for p, w in zip(o, want))


def _h(t: Optional[STen]):
    return t.h if t is not None else None


class BertEncoder(_Multi):
    """BertEncoder.apply (bert.scala:485-534); forward((tokens, segments, maxLength)) -> [B, T, embeddingDim].  State: token table, segment
    table, the positional table (a parameter, [1, maxLength, embeddingDim]; default PositionalEmbedding.vaswani in single precision cast
    to dtype), then the blocks (gptOrder = false, no causal mask)."""
    def __init__(self, maxLength, vocabularySize, segmentVocabularySize, numBlocks, embeddingDim, attentionHiddenPerHeadDim, attentionNumHeads,
                 mlpHiddenDim, dropout, dtype=F32, device=0, linearized=False, positionEmbedding: Optional[STen] = None):
        super().__init__(_mk("lamp_module_bert_encoder", maxLength, vocabularySize, segmentVocabularySize, numBlocks, embeddingDim,
                             attentionHiddenPerHeadDim, attentionNumHeads, mlpHiddenDim, float(dropout), dtype, device, int(linearized),
                             _h(positionEmbedding)))

    def forward(self, tokens: Variable, segments: Variable, maxLength: Optional[STen] = None) -> Variable:
        return _forward_multi(self, [tokens, segments], [maxLength])


class MaskedLanguageModelModule(_Multi):
    """MaskedLanguageModelModule.apply (bert.scala:347-359): Linear -> relu -> LayerNorm -> Linear over
    encoded.view(-1, D).indexSelect(0, positions.view(-1)); forward((encoderOutput, predictionPositions)) -> [B, P, vocabularySize].
    perRowPositions=False is the reference as written: the positions index the flattened rows directly, without a b * T offset, so every
    batch row reads batch row 0's region.  perRowPositions=True (not in the reference) gathers row b's positions from row b."""
    def __init__(self, inputDim, hiddenDim, vocabularySize, dtype=F32, device=0, perRowPositions=False):
        super().__init__(_mk("lamp_module_masked_language_model", inputDim, hiddenDim, vocabularySize, dtype, device, int(perRowPositions)))

    def forward(self, encoderOutput: Variable, predictionPositions: STen) -> Variable:
        return _forward_multi(self, [encoderOutput], [predictionPositions])


def _pretrain_forward(module, tokens: Variable, segments: Variable, positions: STen, maxLength: Optional[STen]):
    """lamp_bert_pretrain_forward on a BertPretrainModule or a BertLoss (the C entry accepts either) -> BertPretrainOutput's three members"""
    e, s, w = C.c_void_p(), C.c_void_p(), C.c_void_p()
    lib.lamp_bert_pretrain_forward(module.h, tokens.h, segments.h, positions.h, _h(maxLength), C.byref(e), C.byref(s), C.byref(w))
    return Variable(e), Variable(s), Variable(w)


class BertPretrainModule(_Multi):
    """BertPretrainModule.apply (bert.scala:244-285); forward(BertPretrainInput) -> (encoded, languageModelScores = logSoftMax(dim 2),
    wholeSentenceBinaryClassifierScore [B])."""
    def __init__(self, maxLength, vocabularySize, segmentVocabularySize, mlmHiddenDim, wholeSentenceHiddenDim, numBlocks, embeddingDim,
                 attentionHiddenPerHeadDim, attentionNumHeads, bertEncoderMlpHiddenDim, dropout, dtype=F32, device=0, linearized=False,
                 positionEmbedding: Optional[STen] = None, perRowPositions=False):
        super().__init__(_mk("lamp_module_bert_pretrain", maxLength, vocabularySize, segmentVocabularySize, mlmHiddenDim, wholeSentenceHiddenDim,
                             numBlocks, embeddingDim, attentionHiddenPerHeadDim, attentionNumHeads, bertEncoderMlpHiddenDim, float(dropout), dtype,
                             device, int(linearized), _h(positionEmbedding), int(perRowPositions)))

    def forward(self, tokens: Variable, segments: Variable, positions: STen, maxLength: Optional[STen] = None):
        return _pretrain_forward(self, tokens, segments, positions, maxLength)


class BertLoss(_Multi):
    """BertLoss.apply (bert.scala:96-140): NLL(mean, ignore = padToken, class weights of ones) on the flattened language model scores plus
    BCEWithLogits(mean) on the whole-sentence score; forward(BertLossInput) -> the loss.  One training step is
    `loss.backprop()` followed by `optimizer.step([p.partialDerivative for p in m.parameters])`."""
    def __init__(self, maxLength, vocabularySize, segmentVocabularySize, mlmHiddenDim, wholeSentenceHiddenDim, numBlocks, embeddingDim,
                 attentionHiddenPerHeadDim, attentionNumHeads, bertEncoderMlpHiddenDim, dropout, padToken, dtype=F32, device=0, linearized=False,
                 positionEmbedding: Optional[STen] = None, perRowPositions=False):
        super().__init__(_mk("lamp_module_bert_loss", maxLength, vocabularySize, segmentVocabularySize, mlmHiddenDim, wholeSentenceHiddenDim, numBlocks,
                             embeddingDim, attentionHiddenPerHeadDim, attentionNumHeads, bertEncoderMlpHiddenDim, float(dropout), int(padToken), dtype,
                             device, int(linearized), _h(positionEmbedding), int(perRowPositions)))

    def forward(self, tokens: Variable, segments: Variable, positions: STen, maxLength: Optional[STen], maskedLanguageModelTarget: STen,
                wholeSentenceTarget: STen) -> Variable:
        return _forward_multi(self, [tokens, segments], [positions, maxLength, maskedLanguageModelTarget, wholeSentenceTarget])

    def pretrain(self, tokens: Variable, segments: Variable, positions: STen, maxLength: Optional[STen] = None):
        return _pretrain_forward(self, tokens, segments, positions, maxLength)


# ---- batch builder (lamp.data.bert) --------------------------------------------------------------------------------------------------------------
def pad(v: Sequence[int], paddedLength: int, padElem: int) -> np.ndarray:
    v = np.asarray(v, dtype=np.int64)
    assert len(v) <= paddedLength, f"{len(v)} elements do not fit a padded length of {paddedLength}"
    return np.concatenate([v, np.full(paddedLength - len(v), padElem, dtype=np.int64)])


def makeMaskForMaskedLanguageModel(bertTokens: Sequence[int], maximumTokenId: int, clsToken: int, sepToken: int, maskToken: int,
                                   rng: np.random.Generator):
    """package.scala:18-55 -> (mlmPositions, mlmTarget, maskedBertTokens).  The positions are max(1, int(len * 0.15)) of the tokens that are
    neither cls nor sep, drawn without replacement (fewer if there are fewer); each is replaced by the mask token with probability 0.8, by
    integers(maximumTokenId) with 0.1 and left as it is with 0.1; the targets are the original tokens."""
    bertTokens = np.asarray(bertTokens, dtype=np.int64)
    candidates = np.flatnonzero((bertTokens != clsToken) & (bertTokens != sepToken))
    positions = rng.permutation(candidates)[:max(1, int(len(bertTokens) * 0.15))]
    masked = bertTokens.copy()
    for idx in positions:
        r = rng.random()
        if r < 0.8:
            masked[idx] = maskToken
        elif r < 0.9:
            masked[idx] = rng.integers(maximumTokenId)
    return positions.astype(np.int64), bertTokens[positions], masked


def prepareParagraph(paragraph: Sequence[Sequence[int]], maximumTokenId: int, clsToken: int, sepToken: int, padToken: int, maskToken: int,
                     maxLength: int, rng: np.random.Generator) -> List[tuple]:
    """package.scala:57-131: one example per sentence but the last -> (trueNextSentence, tokens [maxLength], segments [maxLength],
    positions [int(maxLength * 0.15)], targets [int(maxLength * 0.15)], unpadded length).  cls sentence sep next sep; a sentence longer than
    the window (maxLength - 3) // 2 is cut to a window at a random start; the next sentence is the true one with probability 1/2, else any
    sentence of the paragraph; segments 0 up to and including the first sep, 1 after it; tokens pad with padToken, segments and
    positions with 0, targets with padToken."""
    if maxLength < 7:
        raise ValueError(f"maxLength = {maxLength}: below 7 there is no room for a prediction position (int(maxLength * 0.15) = 0)")
    maxNumPredictionPositions = int(maxLength * 0.15)
    numSentences = len(paragraph)
    windowSize = (maxLength - 3) // 2

    def window(sentence):
        sentence = np.asarray(sentence, dtype=np.int64)
        if len(sentence) <= windowSize:
            return sentence
        start = int(rng.integers(len(sentence) - windowSize))
        return sentence[start:start + windowSize]

    out = []
    for sentenceIdx in range(numSentences - 1):
        trueNextSentence = bool(rng.integers(2))
        nextSentence0 = paragraph[sentenceIdx + 1] if trueNextSentence else paragraph[int(rng.integers(numSentences))]
        sentence, nextSentence = window(paragraph[sentenceIdx]), window(nextSentence0)
        bertTokens = np.concatenate([[clsToken], sentence, [sepToken], nextSentence, [sepToken]]).astype(np.int64)
        assert len(bertTokens) <= maxLength
        mlmPositions, mlmTarget, maskedBertTokens = makeMaskForMaskedLanguageModel(bertTokens, maximumTokenId, clsToken, sepToken, maskToken, rng)
        bertSegments = np.concatenate([np.zeros(len(sentence) + 2, dtype=np.int64), np.ones(len(nextSentence) + 1, dtype=np.int64)])
        out.append((trueNextSentence, pad(maskedBertTokens, maxLength, padToken), pad(bertSegments, maxLength, 0),
                    pad(mlmPositions, maxNumPredictionPositions, 0), pad(mlmTarget, maxNumPredictionPositions, padToken), len(bertTokens)))
    return out


def minibatchesFromParagraphs(minibatchSize: int, dropLast: bool, paragraphs: Sequence[Sequence[Sequence[int]]], maximumTokenId: int, clsToken: int,
                              sepToken: int, padToken: int, maskToken: int, maxLength: int, rng: np.random.Generator, device: int = 0) -> Iterator[dict]:
    """package.scala:133-228: the paragraphs are shuffled and taken minibatchSize at a time; with dropLast the last group is left out (as the
    reference's dropRight(1) does, whether or not it is full).  Every group yields one batch of device tensors, the arguments of
    BertLoss.forward by name: tokens and segments (constants, long [B, maxLength]), positions and maskedLanguageModelTarget (long
    [B, int(maxLength * 0.15)]), maxLength (long [B]: the unpadded lengths), wholeSentenceTarget (float [B]); B is the number of
    sentence pairs of the group's paragraphs."""
    if maxLength < 7:
        raise ValueError(f"maxLength = {maxLength}: below 7 there is no room for a prediction position (int(maxLength * 0.15) = 0)")
    order = rng.permutation(len(paragraphs))
    groups = [order[i:i + minibatchSize] for i in range(0, len(order), minibatchSize)]
    if dropLast:
        groups = groups[:-1]
    for group in groups:
        ps = [e for paragraphIdx in group
              for e in prepareParagraph(paragraphs[paragraphIdx], maximumTokenId, clsToken, sepToken, padToken, maskToken, maxLength, rng)]
        if not ps:
            continue
        dev = lambda a: STen.from_numpy(np.ascontiguousarray(a), device)
        yield {"tokens": const(dev(np.stack([p[1] for p in ps]))), "segments": const(dev(np.stack([p[2] for p in ps]))),
               "positions": dev(np.stack([p[3] for p in ps])), "maxLength": dev(np.array([p[5] for p in ps], dtype=np.int64)),
               "maskedLanguageModelTarget": dev(np.stack([p[4] for p in ps])),
               "wholeSentenceTarget": dev(np.array([1.0 if p[0] else 0.0 for p in ps], dtype=np.float32))}
