"""References for lamp.data.languagemodel (tests/test_generate.py, tests/test_generate_gpu.py): the reference's generation loop over the
oracle's LanguageModel, the sampler in numpy, and f64 torch forms of the decode kernels.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np
import torch


def sample_ref(logits, temperature, u):
    """One token per row: p = exp((logits - max) / temperature) in f64, the running sum of p, and the first index whose running sum exceeds
    u * total, at most V - 1 (the draw of languagemodel/package.scala:95-104 with the uniform number given).  logits [R, V], u [R]."""
    z = np.asarray(logits, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    assert z.ndim == 2 and u.shape[0] == z.shape[0] and temperature > 0
    out = np.zeros(z.shape[0], dtype=np.int64)
    for r in range(z.shape[0]):
        c = np.cumsum(np.exp((z[r] - z[r].max()) / temperature))
        above = np.flatnonzero(c > u[r] * c[-1])
        out[r] = above[0] if above.size else z.shape[1] - 1
    return out


def cumulative_intervals(logits_row, temperature):
    """the running sums of sample_ref for one row, divided by their total: category k owns (c[k - 1], c[k]]"""
    z = np.asarray(logits_row, dtype=np.float64)
    c = np.cumsum(np.exp((z - z.max()) / temperature))
    return c / c[-1]


def window_logits_ref(om, window):
    """the oracle's logits for the next token after `window` (a list of ints): LanguageModelInput as makeInput builds it
    (package.scala:44-65): tokens [1, w], maxLength arange(1, w + 1), positions [[w - 1]]"""
    w = len(window)
    tokens = torch.tensor([list(window)], dtype=torch.int64)
    maxLength = torch.arange(1, w + 1, dtype=torch.int64).unsqueeze(0)
    _, logits = om.forward(tokens, maxLength, torch.tensor([[w - 1]], dtype=torch.int64))
    return logits.value.detach().reshape(-1)


def generate_ref(om, prefix, length, temperature, modelBlockSize, uniforms, windows=None):
    """package.scala:88-112: acc.takeRight(modelBlockSize) -> logits -> a draw -> acc :+ next.  uniforms[i] is step i's uniform number;
    `windows` (a list) receives every window the model saw.  Returns (tokens, [logits of every step])."""
    assert temperature > 0 and len(prefix) > 0
    acc, all_logits = list(prefix), []
    for i in range(length):
        window = acc[-modelBlockSize:]
        if windows is not None:
            windows.append(list(window))
        logits = window_logits_ref(om, window)
        all_logits.append(logits)
        acc.append(int(sample_ref(logits.double().numpy()[None, :], temperature, [uniforms[i]])[0]))
    return acc, all_logits


def decode_linear_ref(x, w, transposed=False, layerNorm=False, eps=1e-5, lnScale=None, lnBias=None, bias=None, gelu=False, scale=None,
                      residual=None):
    """residual + scale * act(LN(x) . W + bias) in f64"""
    d = lambda t: None if t is None else t.double()
    x, w = x.double(), w.double()
    if layerNorm:
        mu = x.mean(1, keepdim=True)
        var = ((x - mu) ** 2).mean(1, keepdim=True)
        x = (x - mu) / torch.sqrt(var + eps)
        if lnScale is not None:
            x = x * d(lnScale).reshape(1, -1)
        if lnBias is not None:
            x = x + d(lnBias).reshape(1, -1)
    y = x @ (w.t() if transposed else w)
    if bias is not None:
        y = y + d(bias).reshape(1, -1)
    if gelu:
        y = 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    if scale is not None:
        y = y * d(scale).reshape(1, -1) + d(residual)
    return y


def decode_attention_ref(qkv, kcache, vcache, t, H):
    """(out [R, H d], new key [R, H, d], new value [R, H, d]) in f64; cache rows beyond t - 1 are not read"""
    R = qkv.shape[0]
    d = qkv.shape[1] // (3 * H)
    q, k, v = (p.double().reshape(R, H, d) for p in qkv.split(H * d, dim=1))
    K = torch.cat([kcache[:, :, :t].double(), k.unsqueeze(2)], 2)          # [R, H, t + 1, d]
    V = torch.cat([vcache[:, :, :t].double(), v.unsqueeze(2)], 2)
    s = torch.einsum("rhd,rhjd->rhj", q, K) / math.sqrt(d)
    p = torch.exp(torch.log_softmax(s, dim=2))
    return torch.einsum("rhj,rhjd->rhd", p, V).reshape(R, H * d), k, v
