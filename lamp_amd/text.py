"""lamp.data.Text over the host C ABI: the text helpers, minibatchesFromText, sequencePrediction and sequencePredictionBeam.

Reference: lamp-data/src/main/scala/lamp/data/Text.scala.  The helpers are plain Python / numpy.  The two predictions need values, not a
graph: a module of the shape statefulSequence(Embedding, RNN | GRU | LSTM, [Fun("relu")], SeqLinear, [Fun("logsoftmax", 2)]) in f32 or f64 on
a device, with at most 16 rows, generates every token after the prefix with three launches (GRU four) of csrc/kernels/recurrent_decode.hip
and decode.hip (csrc/host/text.cpp); everything else runs the reference's chain (FreeRunningRNN, a forward per beam).  `textGenerationFused`
switches between the two, `textGeneratePath` says which one the last call took.  The kernels are also exposed one by one
(recurrentDecodePack, recurrentDecodeStep, logSoftMaxArgmaxRows).
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from ._capi import lib, handle_array
from .sten import STen, I64

RNN, GRU, LSTM = 0, 1, 2           # LAMP_RECURRENT_*
MAX_DECODE_ROWS = 16               # LAMP_DECODE_MAX_ROWS


def textGenerationFused(on: bool) -> bool:
    """process-wide, run-time only: sequencePrediction / sequencePredictionBeam over the decode kernels where the module allows it (True) or
    always as the reference's chain (False); returns the previous setting"""
    prev = C.c_int(0); lib.lamp_text_generation_fused(int(bool(on)), C.byref(prev)); return bool(prev.value)


def textGeneratePath() -> Optional[str]:
    """"fused" or "chain": the path the last sequencePrediction / sequencePredictionBeam of this process took (None before the first)"""
    p = C.c_int(-1); lib.lamp_text_generate_path(C.byref(p))
    return {1: "fused", 0: "chain"}.get(p.value)


# ---- text <-> integers (Text.scala:137-203, 298-315) -------------------------------------------------------------------------------------------
def charsToIntegers(text: str, chars: Optional[Dict[str, int]] = None) -> Union[Tuple[Dict[str, int], List[int]], List[int]]:
    """charsToIntegers(text): (vocabulary, tokens), the characters numbered by descending count (the reference leaves the order among equal
    counts open; here the character seen first comes first).  charsToIntegers(text, chars): the tokens under a given vocabulary."""
    if chars is not None:
        return [chars[c] for c in text]
    count: Dict[str, int] = {}
    for c in text:
        count[c] = count.get(c, 0) + 1
    order = sorted(count, key=lambda c: -count[c])          # stable: first occurrence among equals
    vocab = {c: i for i, c in enumerate(order)}
    return vocab, [vocab[c] for c in text]


def wordsToIntegers(text: str, minimumTokenId: int, minimumFrequency: int) -> Tuple[np.ndarray, Dict[str, int]]:
    """(tokens, vocabulary): the words of text.split("\\\\s+") that occur at least minimumFrequency times, numbered from minimumTokenId + 1 by
    descending count; every other word is minimumTokenId (the unknown id)"""
    words = re.split(r"\s+", text)
    while len(words) > 1 and words[-1] == "":               # String.split drops trailing empty strings
        words.pop()
    count: Dict[str, int] = {}
    for w in words:
        count[w] = count.get(w, 0) + 1
    kept = sorted((w for w in count if count[w] >= minimumFrequency), key=lambda w: -count[w])
    vocab = {w: i + minimumTokenId + 1 for i, w in enumerate(kept)}
    return np.array([vocab.get(w, minimumTokenId) for w in words], dtype=np.int32), vocab


def convertIntegersToText(tensor: Union[STen, np.ndarray], vocab: Dict[int, str]) -> List[str]:
    """a [time, batch] array of token ids -> one string per batch column"""
    a = tensor.to_numpy() if isinstance(tensor, STen) else np.asarray(tensor)
    assert a.ndim == 2, f"[time, batch] expected, got shape {a.shape}"
    return ["".join(vocab[int(v)] for v in a[:, b]) for b in range(a.shape[1])]


def convertLogitsToText(tensor: Union[STen, np.ndarray], vocab: Dict[int, str]) -> List[str]:
    """a [time, batch, vocabulary] array -> the text of its argmax(2)"""
    a = tensor.to_numpy() if isinstance(tensor, STen) else np.asarray(tensor)
    return convertIntegersToText(np.argmax(a, axis=2), vocab)


def sentenceToPaddedVec(sentence: str, maxLength: int, pad: int, vocabulary: Dict[str, int]) -> np.ndarray:
    ids = [vocabulary[c] for c in sentence][:maxLength]
    return np.array(ids + [pad] * (maxLength - len(ids)), dtype=np.int32)


def sentencesToPaddedMatrix(sentences: Sequence[str], maxLength: int, pad: int, vocabulary: Dict[str, int]) -> List[np.ndarray]:
    return [sentenceToPaddedVec(s, maxLength, pad, vocabulary) for s in sentences]


def makePredictionBatch(examples: Sequence[Sequence[int]], device: int = 0) -> STen:
    """examples x time, transposed to [time, batch], int64, on the device.  The reference wraps it in const(); here the modules and the
    predictions take the tensor (autograd.const(batch) makes the Variable)."""
    a = np.asarray(examples, dtype=np.int64)
    assert a.ndim == 2 and a.shape[1] >= 1, f"equal-length, non-empty examples expected, got shape {a.shape}"
    return STen.from_numpy(np.ascontiguousarray(a.T), device=device)


class TextBatchStream:
    """what minibatchesFromText returns: iterate for (features [time, batch], target [time, batch]) int64 STen pairs; loops.oneEpoch takes it
    as it takes a data.BatchStream (reset, iteration, numBatches)"""

    def __init__(self, text: np.ndarray, groups: List[np.ndarray], timeSteps: int, device: int):
        self._text, self._groups, self._T, self._device = text, groups, timeSteps, device
        self._at = 0

    @property
    def numBatches(self) -> int:
        return len(self._groups)

    def reset(self) -> None:
        self._at = 0

    def nextBatch(self) -> Optional[Tuple[STen, STen]]:
        if self._at >= len(self._groups):
            return None
        idx = self._groups[self._at]
        self._at += 1
        window = idx[:, None] + np.arange(self._T)[None, :]                    # [batch, time]
        features, target = self._text[window], self._text[window + 1]
        mk = lambda a: STen.from_numpy(np.ascontiguousarray(a.T.astype(np.int64)), device=self._device)
        return mk(features), mk(target)

    def __iter__(self) -> Iterator[Tuple[STen, STen]]:
        while True:
            b = self.nextBatch()
            if b is None:
                return
            yield b


def minibatchesFromText(text: Sequence[int], minibatchSize: int, timeSteps: int, rng, device: int = 0) -> TextBatchStream:
    """Text.scala:226-296.  Drops a random number (< timeSteps) of leading tokens, cuts the rest into (size - 1) / timeSteps windows of
    timeSteps tokens, shuffles the windows with `rng` (an object with nextInt(bound) and shuffle(list), data.JavaRandom), groups them by
    minibatchSize and drops the last group, as the reference does (the ragged one, or a full one when the count divides).  A batch is
    (features [timeSteps, minibatchSize], target = features shifted by one token), int64 on `device`."""
    a = np.asarray(text, dtype=np.int64)
    assert a.ndim == 1 and timeSteps >= 1 and minibatchSize >= 1
    dropped = a[rng.nextInt(timeSteps):]
    numSamples = (len(dropped) - 1) // timeSteps if len(dropped) else 0
    starts = rng.shuffle(list(range(0, numSamples * timeSteps, timeSteps)))
    groups = [np.asarray(starts[i:i + minibatchSize], dtype=np.int64) for i in range(0, len(starts), minibatchSize)][:-1]
    assert all(len(g) == minibatchSize for g in groups)
    return TextBatchStream(dropped, groups, timeSteps, device)


# ---- generation (Text.scala:18-135) ------------------------------------------------------------------------------------------------------------
def _prediction_batch(batch, device: int) -> STen:
    return batch if isinstance(batch, STen) else makePredictionBatch(batch, device)


def sequencePrediction(batch, device: int, module, steps: int, returnOutputs: bool = False):
    """Text.sequencePrediction: batch is a sequence of equal-length token sequences (or the [time, batch] int64 STen of makePredictionBatch).
    Returns [steps, B] int64 on the device: FreeRunningRNN(module, steps).forward(prefix, module.initState)[0].argmax(2).  With returnOutputs
    also the [steps, B, V] outputs whose argmax the tokens are."""
    p = _prediction_batch(batch, device)
    tokens, outputs = C.c_void_p(), C.c_void_p()
    lib.lamp_text_sequence_prediction(module.h, p.h, int(steps), C.byref(tokens), C.byref(outputs) if returnOutputs else None)
    return (STen(tokens), STen(outputs)) if returnOutputs else STen(tokens)


def sequencePredictionBeam(prefix: Sequence[int], device: int, module, steps: int, startSequence: int, endOfSequence: int,
                           k: int = 3) -> List[Tuple[np.ndarray, float]]:
    """Text.sequencePredictionBeam for one prefix: up to k (tokens 1-D int64, logProb) pairs, best first.  Every sequence starts with the
    prefix's last token and has at most steps + 1 entries; a beam whose last token is endOfSequence is carried forward unchanged; the
    log-probabilities are added in double on the host.  k is 3 in the reference."""
    p = _prediction_batch([list(prefix)], device)
    tokens = (C.c_int64 * max(1, k * (steps + 1)))()
    offsets = (C.c_int64 * (k + 1))()
    logProbs = (C.c_double * k)()
    n = C.c_int(0)
    lib.lamp_text_sequence_prediction_beam(module.h, p.h, int(steps), int(startSequence), int(endOfSequence), int(k), tokens, offsets, logProbs, C.byref(n))
    return [(np.array(tokens[offsets[i]:offsets[i + 1]], dtype=np.int64), float(logProbs[i])) for i in range(n.value)]


# ---- the kernels, one by one -------------------------------------------------------------------------------------------------------------------
def _h(t: Optional[STen]):
    return t.h if t is not None else None


def recurrentDecodePack(kind: int, tensors: Sequence[STen]) -> Tuple[STen, STen, Optional[STen]]:
    """the module's state tensors -> (w [E + H, nG H] gate-interleaved, bias [nG H], GRU: Whh [H, H]) (lamp_recurrent_decode_pack)"""
    w, b, w2 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    lib.lamp_recurrent_decode_pack(C.byref(w), C.byref(b), C.byref(w2), int(kind), handle_array([t.h for t in tensors]), len(tensors))
    return STen(w), STen(b), (STen(w2) if w2.value else None)


def recurrentDecodeStep(kind: int, table: STen, tokens: STen, packed: Tuple[STen, STen, Optional[STen]], hPrev: STen, cPrev: Optional[STen] = None,
                        parent: Optional[STen] = None, relu: bool = False) -> Tuple[STen, Optional[STen], Optional[STen]]:
    """one time step for tokens' rows: (h, c | None, relu(h) | None), each [R, H] (lamp_recurrent_decode_step)"""
    w, b, w2 = packed
    R, H = tokens.numel, hPrev.shape[1]
    dt, dev = table.scalarTypeByte, table.device
    mk = lambda: STen.zeros([R, H], dt, dev)
    h, c, rl = mk(), (mk() if kind == LSTM else None), (mk() if relu else None)
    lib.lamp_recurrent_decode_step(int(kind), table.h, tokens.h, _h(parent), w.h, b.h, _h(w2), hPrev.h, _h(cPrev), h.h, _h(c), _h(rl))
    return h, c, rl


def logSoftMaxArgmaxRows(logits: STen, logSoftMax: bool = True, out: Optional[STen] = None, tokens: Optional[STen] = None) -> Tuple[STen, STen]:
    """(out [R, V], tokens int64 [R]): the log-softmax of every row (or the row itself) and the index of its largest stored value
    (lamp_log_softmax_argmax_rows); out / tokens: where to write them (any row pitch / any stride)"""
    R, V = logits.shape
    if out is None:
        out = STen.zeros([R, V], logits.scalarTypeByte, logits.device)
    if tokens is None:
        tokens = STen.zeros([R], I64, logits.device)
    lib.lamp_log_softmax_argmax_rows(out.h, tokens.h, logits.h, int(bool(logSoftMax)))
    return out, tokens
