"""lamp.data.Text without a GPU: the text helpers (lamp_amd/text.py), the restatement of the free-running and beam loops
(tests/text_ref.py) on models small enough to work out by hand, and the exported entry points."""
import math

import numpy as np
import torch

from lamp_amd import text as TX
from lamp_amd.data import JavaRandom
from tests import text_ref as TR


def test_chars_to_integers_both_forms():
    text = "aaaabbbccd"                                    # counts 4, 3, 2, 1: all distinct
    vocab, tokens = TX.charsToIntegers(text)
    assert vocab == {"a": 0, "b": 1, "c": 2, "d": 3}
    assert tokens == [0] * 4 + [1] * 3 + [2] * 2 + [3]
    assert TX.charsToIntegers("dcba", vocab) == [3, 2, 1, 0]


def test_words_to_integers_minimum_frequency_and_unknown():
    text = "the cat  the dog\nthe cat bird"
    tokens, vocab = TX.wordsToIntegers(text, minimumTokenId=5, minimumFrequency=2)
    assert vocab == {"the": 6, "cat": 7}                   # dog and bird occur once: the unknown id
    assert tokens.tolist() == [6, 7, 6, 5, 6, 7, 5]
    tokens, vocab = TX.wordsToIntegers("b a a ", 0, 1)      # trailing whitespace adds no word
    assert vocab == {"a": 1, "b": 2} and tokens.tolist() == [2, 1, 1]


def test_convert_integers_and_logits_to_text():
    vocab = {0: "a", 1: "b", 2: "c"}
    a = np.array([[0, 2], [1, 2], [2, 0]])                 # [time, batch]
    assert TX.convertIntegersToText(a, vocab) == ["abc", "cca"]
    logits = np.full((3, 2, 3), -1.0)
    for t in range(3):
        for b in range(2):
            logits[t, b, a[t, b]] = 0.5
    assert TX.convertLogitsToText(logits, vocab) == ["abc", "cca"]


def test_padding():
    vocab = {"a": 1, "b": 2}
    assert TX.sentenceToPaddedVec("ab", 4, 0, vocab).tolist() == [1, 2, 0, 0]
    assert TX.sentenceToPaddedVec("ababab", 4, 0, vocab).tolist() == [1, 2, 1, 2]
    m = TX.sentencesToPaddedMatrix(["a", "bab"], 3, 9, vocab)
    assert [r.tolist() for r in m] == [[1, 9, 9], [2, 1, 2]]


def test_minibatches_from_text_shapes_shift_and_ragged_group():
    text = list(range(100, 100 + 47))                      # distinct tokens: a window is recognised by its values
    T, B = 5, 2
    stream = TX.minibatchesFromText(text, B, T, JavaRandom(3), device=-1)
    # at most 4 tokens dropped: (47 - d - 1) // 5 = 9 or 8 windows -> 5 or 4 groups of 2, the last one (ragged or not) dropped
    assert stream.numBatches in (3, 4)
    seen = []
    for _ in range(2):                                     # reset() replays the same batches
        stream.reset()
        batches = [(f.to_numpy(), t.to_numpy()) for f, t in stream]
        assert len(batches) == stream.numBatches
        for f, t in batches:
            assert f.shape == (T, B) and t.shape == (T, B) and f.dtype == np.int64
            assert np.array_equal(t[:-1], f[1:]), "target = features shifted by one"
            assert np.array_equal(t, f + 1)                # consecutive tokens of the text
        seen.append(np.concatenate([f[0] for f, _ in batches]))
    assert np.array_equal(seen[0], seen[1])
    starts = seen[0]
    assert len(set(starts.tolist())) == len(starts) and len(set((starts % T).tolist())) == 1, "disjoint windows on one grid"


def _markov(table):
    """a "model" whose output is a row of a [V, V] log-probability table indexed by the last token"""
    def forward(x, state):
        return table[x], state                             # [T, B] -> [T, B, V]
    return forward


P = torch.tensor([[0.05, 0.60, 0.20, 0.15],
                  [0.50, 0.10, 0.10, 0.30],
                  [0.40, 0.30, 0.20, 0.10],
                  [0.25, 0.25, 0.25, 0.25]], dtype=torch.float64)


def test_beam_known_answer_with_an_early_end():
    """prefix [2, 0], end of sequence 3, k = 3.  Step 1 from token 0: 1 (.6), 2 (.2), 3 (.15).  Step 2: [0 1] -> 0 (.6 * .5 = .30), 3 (.6 * .3 =
    .18); [0 2] -> at most .2 * .4 = .08; [0 3] has ended and is carried at .15.  So: [0 1 0] .30, [0 1 3] .18, [0 3] .15, the last one shorter."""
    got = TR.beam(_markov(P.log()), [2, 0], None, 2, start_sequence=0, end_of_sequence=3, k=3)
    assert [t.tolist() for t, _ in got] == [[0, 1, 0], [0, 1, 3], [0, 3]]
    for (_, lp), want in zip(got, (0.30, 0.18, 0.15)):
        assert abs(lp - math.log(want)) < 1e-14
    # one step only: the three best continuations of the prefix's last token
    got = TR.beam(_markov(P.log()), [2, 0], None, 1, 0, 3, 3)
    assert [t.tolist() for t, _ in got] == [[0, 1], [0, 2], [0, 3]]
    # k = 1 is greedy, and a start token that is the end token runs nothing
    assert [t.tolist() for t, _ in TR.beam(_markov(P.log()), [0], None, 3, 0, 3, 1)] == [[0, 1, 0, 1]]
    assert [t.tolist() for t, _ in TR.beam(_markov(P.log()), [0], None, 3, 3, 3, 3)] == [[0]]


def test_free_running_known_answer():
    """greedy over the same table: 0 -> 1 -> 0 -> 1; the first iteration sees the whole prefix, the outputs are the rows that were read"""
    out, _ = TR.free_running(_markov(P.log()), torch.tensor([[2, 1], [0, 1]]), None, 3)      # [time, batch]: prefixes (2, 0) and (1, 1)
    assert out.shape == (3, 2, 4)
    assert out.argmax(2).tolist() == [[1, 0], [0, 1], [1, 0]]
    assert torch.equal(out[0], P.log()[torch.tensor([0, 1])])


def test_text_entry_points_exported():
    from lamp_amd import recurrent as RC
    from lamp_amd._capi import lib
    lib.load()
    names = ["lamp_module_free_running_rnn", "lamp_module_seq2seq", "lamp_module_with_init", "lamp_module_init_state",
             "lamp_module_forward_stateful_pair", "lamp_text_sequence_prediction", "lamp_text_sequence_prediction_beam",
             "lamp_text_generation_fused", "lamp_text_generate_path", "lamp_recurrent_decode_pack", "lamp_recurrent_decode_step",
             "lamp_log_softmax_argmax_rows"]
    for n in names:
        assert n in lib.decls, f"{n} is not declared in include/*.h"
        assert n not in lib.missing, f"{n} is declared but not exported by the library"
    for n in ("FreeRunningRNN", "Seq2Seq", "WithInit"):
        assert hasattr(RC, n)
    for n in ("charsToIntegers", "wordsToIntegers", "convertIntegersToText", "convertLogitsToText", "sentenceToPaddedVec", "sentencesToPaddedMatrix",
              "makePredictionBatch", "minibatchesFromText", "sequencePrediction", "sequencePredictionBeam", "textGenerationFused", "textGeneratePath"):
        assert hasattr(TX, n)
    prev = TX.textGenerationFused(False)                   # run-time only: no GPU is touched
    assert TX.textGenerationFused(prev) is False
