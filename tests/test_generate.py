"""lamp.data.languagemodel without a GPU: the references of tests/generate_ref.py against known answers, and the Python surface."""
import numpy as np
import torch

from tests.generate_ref import cumulative_intervals, generate_ref, sample_ref, window_logits_ref
from tests.test_transformer import _oracle_lm


def test_sample_ref_known_answers():
    logits = np.log(np.array([[0.1, 0.2, 0.3, 0.4]]))
    # the running sums are 0.1, 0.3, 0.6, 1.0 of the total
    for u, want in [(0.0, 0), (0.05, 0), (0.15, 1), (0.29, 1), (0.31, 2), (0.59, 2), (0.61, 3), (0.999, 3)]:
        assert sample_ref(logits, 1.0, [u])[0] == want, (u, want)
    # temperature 0.5 squares the weights: 1, 4, 9, 16 of 30 -> running sums 1/30, 5/30, 14/30, 1
    for u, want in [(0.02, 0), (0.1, 1), (0.3, 2), (0.5, 3)]:
        assert sample_ref(logits, 0.5, [u])[0] == want, (u, want)
    # a large temperature flattens: four equal categories in the limit
    assert sample_ref(logits, 1e9, [0.3])[0] == 1 and sample_ref(logits, 1e9, [0.8])[0] == 3
    # a shift of the logits changes nothing; rows are independent; one category is always drawn; u at the very top is clamped
    two = np.array([[5.0, 5.0, 5.0], [-1000.0, 0.0, -1000.0]])
    assert sample_ref(two + 123.0, 1.0, [0.5, 0.5]).tolist() == [1, 1]
    assert sample_ref(np.array([[3.0]]), 2.0, [0.7]).tolist() == [0]
    assert sample_ref(logits, 1.0, [1.0])[0] == 3
    c = cumulative_intervals(logits[0], 1.0)
    assert np.allclose(c, [0.1, 0.3, 0.6, 1.0])


def test_reference_loop_slides_its_window():
    """package.scala:93: every step sees takeRight(modelBlockSize) of the sequence, the prefix included"""
    vocab, ctx = 11, 6
    om = _oracle_lm(vocab, ctx, 8, 2, 1, torch.float64, -1000)
    prefix, length, block = [3, 1, 4], 7, 5
    windows = []
    u = [(0.37 * (i + 1)) % 1.0 for i in range(length)]
    tokens, logits = generate_ref(om, prefix, length, 0.8, block, u, windows)
    assert tokens[:3] == prefix and len(tokens) == 3 + length and all(0 <= t < vocab for t in tokens)
    assert len(logits) == length and all(l.shape == (vocab,) for l in logits)
    assert [len(w) for w in windows] == [3, 4, 5, 5, 5, 5, 5]
    for i, w in enumerate(windows):
        assert w == tokens[:3 + i][-block:]
    # a step depends on its window alone, and the draw is sample_ref of its logits
    for i in (0, 4, 6):
        again = window_logits_ref(om, windows[i])
        assert torch.equal(again, logits[i])
        assert tokens[3 + i] == sample_ref(again.numpy()[None, :], 0.8, [u[i]])[0]
    # a window that slid differs from the same tokens read from the start of the sequence: the positions moved
    assert not torch.allclose(window_logits_ref(om, tokens[0:5]), window_logits_ref(om, tokens[1:6]))


def test_python_surface():
    import lamp_amd.languagemodel as L
    for name in ("autoregressiveInference", "autoregressiveMinibatchesFromCorpus", "languageModelFused", "languageModelGeneratePath", "manualSeed",
                 "decodeLinear", "decodeAttention", "sampleLogits", "decodeEmbedding", "ACT_NONE", "ACT_GELU", "MAX_DECODE_ROWS"):
        assert hasattr(L, name), name
    from lamp_amd._capi import lib
    for name in ("lamp_decode_linear", "lamp_decode_attention", "lamp_sample_logits", "lamp_sample_logits_out", "lamp_decode_embedding",
                 "lamp_language_model_generate", "lamp_language_model_decode_fused", "lamp_language_model_generate_path"):
        assert name in lib.decls, name
