"""lamp.data.languagemodel over the host C ABI: autoregressiveInference and autoregressiveMinibatchesFromCorpus.

Reference: lamp-data/src/main/scala/lamp/data/languagemodel/package.scala.  The reference generates one sequence and runs the whole model
over the whole prefix for every token; here B equal-length prefixes are generated at once, and while the sequence fits the context a new
token is one row per block against a key / value cache (csrc/kernels/decode.hip, csrc/host/generate.cpp).  `languageModelFused` switches
between that path and the reference's chain; `languageModelGeneratePath` says which one the last call took.  The kernels are also exposed
one by one (decodeLinear, decodeAttention, sampleLogits, decodeEmbedding).
"""
from __future__ import annotations

import ctypes as C
from typing import Iterator, Optional, Sequence, Tuple, Union

import numpy as np

from ._capi import lib
from .sten import STen, I64

ACT_NONE, ACT_GELU = 0, 1          # LAMP_DECODE_ACT_*
MAX_DECODE_ROWS = 16               # LAMP_DECODE_MAX_ROWS


def languageModelFused(on: bool) -> bool:
    """process-wide: autoregressiveInference over the decode kernels and a key / value cache (True, the default) or as the reference's
    chain of full forward, / temperature, logSoftMax, exp and multinomial for every token (False); returns the previous setting"""
    prev = C.c_int(0); lib.lamp_language_model_decode_fused(int(bool(on)), C.byref(prev)); return bool(prev.value)


def languageModelGeneratePath() -> Optional[str]:
    """"fused" or "chain": the path the last autoregressiveInference of this process took (None before the first)"""
    p = C.c_int(-1); lib.lamp_language_model_generate_path(C.byref(p))
    return {1: "fused", 0: "chain"}.get(p.value)


def manualSeed(seed: int) -> None:
    """seeds the library's Philox stream (lamp_manual_seed): the same seed gives the same draws"""
    lib.lamp_manual_seed(int(seed))


def _h(t: Optional[STen]):
    return t.h if t is not None else None


def autoregressiveInference(model, modelBlockSize: int, prefix: Union[Sequence[int], np.ndarray, STen], length: int, temperature: float,
                            returnLogits: bool = False):
    """package.scala:35-114.  model: a LanguageModelModule or a LanguageModelLoss.  prefix: a sequence of token ids, or a [B, P] array (or
    int64 STen) of B equal-length prefixes.  Returns the prefix followed by `length` sampled tokens in the form of the input: a list of ints,
    a [B, P + length] int64 array, or an STen on the model's device.  Every step sees the last modelBlockSize tokens at positions
    0 .. len - 1.  With returnLogits the result is (tokens, logits): the untempered logits of every step as an STen [B, length, vocabulary]
    in the model's type.  The draws come from the library's generator (manualSeed)."""
    if isinstance(prefix, STen):
        form, p = "sten", prefix
    else:
        a = np.asarray(prefix, dtype=np.int64)
        form = "list" if a.ndim == 1 else "array"
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2:
            raise ValueError(f"prefix must be a sequence of token ids or a [B, P] array, got shape {a.shape}")
        p = STen.from_numpy(np.ascontiguousarray(a), device=-1)
    tokens, logits = C.c_void_p(), C.c_void_p()
    lib.lamp_language_model_generate(model.h, p.h, int(length), float(temperature), int(modelBlockSize), C.byref(tokens),
                                     C.byref(logits) if returnLogits else None)
    out = STen(tokens)
    if form != "sten":
        out = out.to_numpy()
        if form == "list":
            out = [int(v) for v in out[0]]
    return (out, STen(logits)) if returnLogits else out


def autoregressiveMinibatchesFromCorpus(minibatchSize: int, numBatches: int, corpus: STen, blockLength: int,
                                        createMaxLength: bool = True) -> Iterator[Tuple[STen, STen, Optional[STen]]]:
    """package.scala:130-203: numBatches random minibatches of minibatchSize windows of blockLength tokens from a 1-D corpus of token ids,
    as (tokens, targets, maxLength | None): int64 [minibatchSize, blockLength] on the corpus's device, targets the window shifted by one,
    maxLength arange(1, blockLength + 1) per row (the causal mask).  `SupervisedModel(LanguageModelLoss, IDENTITY).train_step(optimizer,
    tokens, targets)` takes a batch.  The starts are randint(0, corpusLength - blockLength - 1); both windows are one indexSelect each."""
    corpusLength = corpus.shape[0]
    if len(corpus.shape) != 1 or corpusLength - blockLength - 1 <= 0:
        raise ValueError(f"a corpus of shape {corpus.shape} holds no window of {blockLength} + 1 tokens")
    device = corpus.device
    corpusL = corpus.castToLong()
    offsets = STen.arange(0, blockLength, 1, I64, device).unsqueeze(0)
    maxLength = None
    if createMaxLength:
        maxLength = STen.arange(1, blockLength + 1, 1, I64, device).unsqueeze(0).expand([minibatchSize, blockLength]).contiguous()
    for _ in range(numBatches):
        starts = STen.randint(0, corpusLength - blockLength - 1, [minibatchSize], I64, device).unsqueeze(1)
        index = (starts + offsets).view(-1)
        tokens = corpusL.indexSelect(0, index).view(minibatchSize, blockLength)
        targets = corpusL.indexSelect(0, index + 1).view(minibatchSize, blockLength)
        yield tokens, targets, maxLength


# ---- the kernels, one by one ---------------------------------------------------------------------------------------------------------------------
def decodeLinear(x: STen, w: STen, transposed: bool = False, layerNorm: bool = False, eps: float = 1e-5, lnScale: Optional[STen] = None,
                 lnBias: Optional[STen] = None, bias: Optional[STen] = None, act: int = ACT_NONE, scale: Optional[STen] = None,
                 residual: Optional[STen] = None) -> STen:
    """residual + scale * act(LN(x) . w + bias) for x [R <= 16, K]; w [K, N], or [N, K] with transposed (lamp_decode_linear)"""
    o = C.c_void_p()
    lib.lamp_decode_linear(C.byref(o), x.h, w.h, int(transposed), int(layerNorm), float(eps), _h(lnScale), _h(lnBias), _h(bias), int(act), _h(scale),
                           _h(residual))
    return STen(o)


def decodeAttention(qkv: STen, kcache: STen, vcache: STen, t: int, numHeads: int) -> STen:
    """writes the new key / value of qkv [R, 3 H d] into position t of the caches [R, H, Tmax, d], returns the attention of the new query
    over positions 0 .. t as [R, H d] (lamp_decode_attention)"""
    o = C.c_void_p(); lib.lamp_decode_attention(C.byref(o), qkv.h, kcache.h, vcache.h, int(t), int(numHeads)); return STen(o)


def sampleLogits(logits: STen, temperature: float, uniforms: Optional[STen] = None) -> STen:
    """one token per row of logits [R, V] from softmax(logits / temperature); uniforms f64 [R] replace the library's generator
    (lamp_sample_logits)"""
    o = C.c_void_p(); lib.lamp_sample_logits(C.byref(o), logits.h, float(temperature), _h(uniforms)); return STen(o)


def decodeEmbedding(tokenWeight: STen, positionWeight: STen, tokens: STen, t: int) -> STen:
    """tokenWeight[tokens] + positionWeight[t] -> [R, D] (lamp_decode_embedding)"""
    o = C.c_void_p(); lib.lamp_decode_embedding(C.byref(o), tokenWeight.h, positionWeight.h, tokens.h, int(t)); return STen(o)
