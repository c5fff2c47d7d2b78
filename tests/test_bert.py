"""The f64 restatement of lamp.nn.bert (tests/bert_ref.py), the pretraining batch builder of lamp_amd.bert on a seeded generator, and the
part of lamp_amd.bert's surface that needs no GPU."""
import numpy as np
import pytest
import torch

from lamp_amd import bert as B
from lamp_amd import sten as S
from tests import bert_ref as R
from tests.util import closed_form

F64 = torch.float64
CLS, SEP, PAD, MASK, MAX_ID = 1, 2, 0, 3, 50


# ---- restatement -----------------------------------------------------------------------------------------------------------------------------------
def _tables(v=6, vs=3, l=7, d=4):
    return [closed_form(s, salt, 2.0, F64).requires_grad_(True) for s, salt in (((v, d), 3), ((vs, d), 5), ((1, l, d), 7))]


def test_restatement_row_zero_and_late_positions_get_no_gradient():
    tw, sw, pe = _tables()
    tokens, segments = torch.tensor([[0, 2, 5, 2, 0], [4, 0, 2, 1, 1]]), torch.tensor([[0, 0, 1, 1, 2], [0, 2, 2, 1, 0]])
    out = R.embedding(tokens, segments, tw, sw, pe)
    assert list(out.shape) == [2, 5, 4]
    assert torch.equal(out[1, 2], (tw[2] + sw[2] + pe[0, 2]).detach())
    assert torch.equal(out[0, 0], (tw[0] + sw[0] + pe[0, 0]).detach())      # row 0 is read like any other row
    out.sum().backward()
    assert torch.equal(tw.grad[0], torch.zeros(4, dtype=F64)) and torch.equal(sw.grad[0], torch.zeros(4, dtype=F64))
    assert torch.equal(tw.grad[2], torch.full((4,), 3.0, dtype=F64)) and torch.equal(tw.grad[3], torch.zeros(4, dtype=F64))
    assert torch.equal(sw.grad[1], torch.full((4,), 3.0, dtype=F64))
    assert torch.equal(pe.grad[0, :5], torch.full((5, 4), 2.0, dtype=F64)) and torch.equal(pe.grad[0, 5:], torch.zeros(2, 4, dtype=F64))


def test_restatement_with_any_index_agrees_inside_and_zeroes_outside():
    tw, sw, pe = _tables()
    tokens, segments = torch.tensor([[1, 2, 5, 0]]), torch.tensor([[0, 1, 2, 1]])
    a = R.embedding(tokens, segments, tw, sw, pe)
    b = R.embedding_with_any_index(tokens, segments, tw, sw, pe)
    assert torch.equal(a, b)
    ga = torch.autograd.grad(a.sum(), [tw, sw, pe])
    gb = torch.autograd.grad(b.sum(), [tw, sw, pe])
    assert all(torch.equal(x, y) for x, y in zip(ga, gb))
    wild = torch.tensor([[6, -7, -1, 2]])                                   # >= V, < -V, wraps to 5, plain
    c = R.embedding_with_any_index(wild, segments, tw, sw, pe)
    assert torch.equal(c[0, 0], (sw[0] + pe[0, 0]).detach()) and torch.equal(c[0, 1], (sw[1] + pe[0, 1]).detach())
    assert torch.equal(c[0, 2], (tw[5] + sw[2] + pe[0, 2]).detach())
    gt = torch.autograd.grad(c.sum(), [tw])[0]
    assert torch.equal(gt[2], torch.ones(4, dtype=F64)) and float(gt.abs().sum()) == 4.0   # the wrapped index reads row 5 and adds nothing to it


def test_restatement_written_out_gradients_are_autograd_s():
    """embedding_gradients (every sum in ascending order) against torch's autograd through embedding_with_any_index"""
    tw, sw, pe = _tables(v=6, vs=3, l=7, d=4)
    tokens, segments = torch.tensor([[0, 2, 5, 2, 6], [4, -1, 2, 1, 1], [2, 2, -9, 3, 0]]), torch.tensor([[0, 0, 1, 1, 2], [0, 2, 3, 1, -1], [1, 1, 1, 2, 2]])
    dout = closed_form((3, 5, 4), 301, 1.0, F64)
    want = torch.autograd.grad((R.embedding_with_any_index(tokens, segments, tw, sw, pe) * dout).sum(), [tw, sw, pe])
    got = R.embedding_gradients(dout, tokens, segments, 6, 3, 7)
    for g, w in zip(got, want):
        assert list(g.shape) == list(w.shape) and float((g - w).abs().max()) <= 1e-14
    assert not got[0][0].any() and not got[1][0].any() and not got[2][0, 5:].any()


def test_restatement_flat_index_reads_batch_row_zero_and_per_row_reads_its_own():
    encoded = closed_form((3, 5, 2), 11, 2.0, F64)
    positions = torch.tensor([[1, 4], [0, 3], [2, 2]])
    flat, own = R.mlm_gather(encoded, positions), R.mlm_gather(encoded, positions, perRowPositions=True)
    for b in range(3):
        for p in range(2):
            assert torch.equal(flat[b, p], encoded[0, positions[b, p]])
            assert torch.equal(own[b, p], encoded[b, positions[b, p]])
    assert torch.equal(flat[0], own[0]) and not torch.equal(flat[1], own[1])


# ---- batch builder -----------------------------------------------------------------------------------------------------------------------------------
def _paragraphs(n=9, seed=5):
    rng = np.random.default_rng(seed)
    return [[list(rng.integers(4, MAX_ID, size=int(rng.integers(2, 30)))) for _ in range(int(rng.integers(2, 5)))] for _ in range(n)]


def test_make_mask_rules():
    rng = np.random.default_rng(0)
    tokens = np.array([CLS] + list(range(10, 30)) + [SEP] + list(range(30, 45)) + [SEP])
    seen = set()
    for _ in range(200):
        positions, target, masked = B.makeMaskForMaskedLanguageModel(tokens, MAX_ID, CLS, SEP, MASK, rng)
        assert len(positions) == max(1, int(len(tokens) * 0.15)) == 5 and len(set(positions.tolist())) == 5
        assert all(tokens[p] not in (CLS, SEP) for p in positions)
        assert np.array_equal(target, tokens[positions])
        untouched = np.setdiff1d(np.arange(len(tokens)), positions)
        assert np.array_equal(masked[untouched], tokens[untouched])
        for p in positions:
            seen.add("mask" if masked[p] == MASK else "same" if masked[p] == tokens[p] else "random")
            assert 0 <= masked[p] < MAX_ID or masked[p] == MASK
    assert seen == {"mask", "same", "random"}                               # 1000 draws at 0.8 / 0.1 / 0.1
    positions, target, masked = B.makeMaskForMaskedLanguageModel(np.array([CLS, 9, SEP, SEP]), MAX_ID, CLS, SEP, MASK, rng)
    assert positions.tolist() == [1] and target.tolist() == [9]             # int(4 * 0.15) = 0 -> one position


@pytest.mark.parametrize("maxLength", [7, 16, 33])
def test_prepare_paragraph_shapes_pads_and_segments(maxLength):
    rng = np.random.default_rng(1)
    window, npos = (maxLength - 3) // 2, int(maxLength * 0.15)
    for paragraph in _paragraphs():
        rows = B.prepareParagraph(paragraph, MAX_ID, CLS, SEP, PAD, MASK, maxLength, rng)
        assert len(rows) == len(paragraph) - 1
        for isNext, tokens, segments, positions, targets, length in rows:
            assert isinstance(isNext, bool) and tokens.shape == segments.shape == (maxLength,) and positions.shape == targets.shape == (npos,)
            assert tokens.dtype == segments.dtype == positions.dtype == targets.dtype == np.int64
            assert 5 <= length <= 2 * window + 3 <= maxLength
            assert tokens[0] == CLS and np.all(tokens[length:] == PAD) and np.all(segments[length:] == 0)
            # cls and sep are never masked, so they stand where they stood: the first sep ends segment 0, the last token is the second sep
            seps = np.flatnonzero(tokens[:length] == SEP)
            first = seps[0]
            assert tokens[length - 1] == SEP and first - 1 <= window and length - first - 2 <= window
            assert np.all(segments[:first + 1] == 0) and np.all(segments[first + 1:length] == 1)
            k = max(1, int(length * 0.15))
            assert np.all(positions[k:] == 0) and np.all(targets[k:] == PAD) and k <= npos
            assert all(0 < p < length - 1 and p != first for p in positions[:k]) and len(set(positions[:k].tolist())) == k


def test_prepare_paragraph_targets_are_the_original_tokens():
    """one sentence pair that fits the window, so the unmasked sequence is known"""
    paragraph = [[10, 11, 12, 13], [20, 21, 22]]
    for seed in range(20):
        (isNext, tokens, segments, positions, targets, length), = B.prepareParagraph(paragraph, MAX_ID, CLS, SEP, PAD, MASK, 16, np.random.default_rng(seed))
        second = paragraph[1] if isNext else None
        if second is None:                                                  # a random sentence of the paragraph: told by its length
            second = paragraph[0] if length == 11 else paragraph[1]
        original = np.array([CLS] + paragraph[0] + [SEP] + second + [SEP])
        assert length == len(original)
        k = max(1, int(length * 0.15))
        assert np.array_equal(targets[:k], original[positions[:k]])
        untouched = np.setdiff1d(np.arange(length), positions[:k])
        assert np.array_equal(tokens[untouched], original[untouched])
        assert segments[:length].tolist() == [0] * 6 + [1] * (len(second) + 1)


@pytest.mark.parametrize("dropLast,groups", [(False, 3), (True, 2)])
def test_minibatches_count_shapes_and_types(dropLast, groups):
    """9 paragraphs in groups of 4: 3 groups, the last one dropped with dropLast (the reference's dropRight(1)); host tensors here"""
    paragraphs = _paragraphs(9)
    batches = list(B.minibatchesFromParagraphs(4, dropLast, paragraphs, MAX_ID, CLS, SEP, PAD, MASK, 16, np.random.default_rng(2), device=S.CPU))
    assert len(batches) == groups
    pairs = sum(b["tokens"].shape[0] for b in batches)
    if not dropLast:
        assert pairs == sum(len(p) - 1 for p in paragraphs)
    for b in batches:
        n = b["tokens"].shape[0]
        assert list(b["tokens"].shape) == list(b["segments"].shape) == [n, 16]
        assert list(b["positions"].shape) == list(b["maskedLanguageModelTarget"].shape) == [n, 2]
        assert list(b["maxLength"].shape) == list(b["wholeSentenceTarget"].shape) == [n]
        assert b["wholeSentenceTarget"].scalarTypeByte == S.F32 and set(b["wholeSentenceTarget"].to_numpy().tolist()) <= {0.0, 1.0}
        for key in ("positions", "maskedLanguageModelTarget", "maxLength"):
            assert b[key].scalarTypeByte == S.I64, key
        tokens, lengths = b["tokens"].value.to_numpy(), b["maxLength"].to_numpy()
        for row, length in zip(tokens, lengths):
            assert row[length - 1] == SEP and np.all(row[length:] == PAD)
        assert set(b) == {"tokens", "segments", "positions", "maxLength", "maskedLanguageModelTarget", "wholeSentenceTarget"}


def test_short_max_length_raises():
    with pytest.raises(ValueError, match="maxLength"):
        B.prepareParagraph([[5, 6], [7, 8]], MAX_ID, CLS, SEP, PAD, MASK, 6, np.random.default_rng(0))
    with pytest.raises(ValueError, match="maxLength"):
        list(B.minibatchesFromParagraphs(2, False, [[[5, 6], [7, 8]]], MAX_ID, CLS, SEP, PAD, MASK, 6, np.random.default_rng(0), device=S.CPU))


def test_same_seed_same_batches():
    run = lambda: [b["tokens"].value.to_numpy() for b in B.minibatchesFromParagraphs(4, False, _paragraphs(), MAX_ID, CLS, SEP, PAD, MASK, 16,
                                                                                     np.random.default_rng(3), device=S.CPU)]
    assert all(np.array_equal(x, y) for x, y in zip(run(), run()))


# ---- python surface ----------------------------------------------------------------------------------------------------------------------------------
def test_python_surface_without_a_gpu():
    """the switch returns the previous setting, the split threshold comes from the library, the public names and module methods exist"""
    first = B.bertFused(False)
    assert B.bertFused(True) is False and B.bertFused(first) is True and B.bertFused(first) is first
    assert B.bertLongRow() >= 64
    for name in ("BertEncoder", "MaskedLanguageModelModule", "BertPretrainModule", "BertLoss", "bertEmbedding", "bertFused",
                 "bertLongRow", "bertEmbeddingForward", "bertEmbeddingBackward", "makeMaskForMaskedLanguageModel", "prepareParagraph",
                 "minibatchesFromParagraphs"):
        assert hasattr(B, name), name
    for cls in (B.BertEncoder, B.MaskedLanguageModelModule, B.BertPretrainModule, B.BertLoss):
        for name in ("forward", "state", "parameters", "zeroGrad", "asEval", "asTraining", "load"):
            assert hasattr(cls, name), (cls.__name__, name)
