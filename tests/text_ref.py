"""The reference's recurrent text generation restated with torch on the CPU over tests/recurrent_ref.py: the example model's forward, the
free-running loop (lamp-core/src/main/scala/lamp/nn/FreeRunningRNN.scala:26-55), Seq2Seq (Seq2Seq.scala:20-24) and the beam loop
(lamp-data/src/main/scala/lamp/data/Text.scala:38-135).  A `forward` is any callable (x [T, B] int64, state) -> (out [T, B, V], state)."""
import torch

from tests import recurrent_ref as R

NCELL = {"rnn": 3, "gru": 9, "lstm": 12}


def embedding(x, table):
    """Embedding.forward: the reference passes padding index 0 (autograd/ops.scala:2151-2174), so row 0 of the table receives no gradient"""
    return torch.nn.functional.embedding(x, table, padding_idx=0)


def cell_forward(kind, x, w, state):
    """(out, state) of one recurrent module; state: None, (h,) or (h, c)"""
    if kind == "lstm":
        out, h, c = R.lstm(x, w, tuple(state) if state is not None else None)
        return out, (h, c)
    out, h = (R.rnn if kind == "rnn" else R.gru)(x, w, state[0] if state is not None else None)
    return out, (h,)


def model_forward(kind, params, relu=True, log_softmax=True):
    """statefulSequence(Embedding, cell, [relu], SeqLinear, [logSoftMax(2)]) over params = [table] + cell weights + [weight, bias]"""
    table, w, lin = params[0], params[1:1 + NCELL[kind]], params[1 + NCELL[kind]:]

    def forward(x, state):
        out, state = cell_forward(kind, embedding(x, table), w, state)
        y = R.seq_linear(out.relu() if relu else out, lin)
        return (torch.log_softmax(y, 2) if log_softmax else y), state
    return forward


def free_running(forward, x, state, time_steps):
    """FreeRunningRNN.forward: (outputs [timeSteps, B, V], lastState)"""
    batch = x.shape[1]
    last_output, last_state, buffer = x, state, []
    for _ in range(time_steps):                                          # loop, :26-55
        output, last_state = forward(last_output, last_state)
        last_char = output.select(0, output.shape[0] - 1).unsqueeze(0) if output.shape[0] > 1 else output   # :37-43
        last_output = last_char.argmax(2).detach()                       # :45-46
        buffer.append(last_char)
    return torch.stack(buffer, 0).view(time_steps, batch, -1), last_state   # :19-24


def seq2seq(encoder, decoder, source, dest, state0):
    _, encoder_state = encoder(source, state0)                           # Seq2Seq.scala:22
    return decoder(dest, encoder_state)                                  # :23


def beam(forward, prefix, init_state, steps, start_sequence, end_of_sequence, k=3, trace=None):
    """Text.sequencePredictionBeam for one prefix (a list of ints): [(tokens 1-D int64, logProb float)], best first.  trace: a list that
    receives, per step, every candidate's summed log-probability in descending order (for the tests' margin condition)."""
    batch = torch.tensor([list(prefix)], dtype=torch.int64).t()          # makePredictionBatch: [time, 1]
    buffers = [([(batch, init_state, start_sequence)], 0.0)]             # :119
    for _ in range(steps):                                               # loop, :54-115
        candidates = []
        for sequence, log_prob0 in buffers:
            last_output, last_state, last_token = sequence[-1]
            if last_token == end_of_sequence:                            # :64-73
                candidates.append((sequence, None, log_prob0, last_state, last_token))
                continue
            output, state = forward(last_output, last_state)             # :75-76
            last_char = output.select(0, output.shape[0] - 1).unsqueeze(0) if output.shape[0] > 1 else output
            for i in range(last_char.shape[2]):                          # :86-100
                log_prob = float(last_char[0, 0, i].double())
                candidates.append((sequence, torch.full((1, 1), i, dtype=torch.int64), log_prob + log_prob0, state, i))
        candidates = sorted(candidates, key=lambda c: c[2])[::-1]        # sortBy(_._3).reverse, :104
        if trace is not None:
            trace.append([c[2] for c in candidates])
        # a finished beam is carried as it is (Text.scala:105-108 appends its end token once more at every further step; the library and
        # this restatement return it at the length at which it ended)
        buffers = [(sequence + [(selected, state, i)] if selected is not None else sequence, log_prob)
                   for sequence, selected, log_prob, state, i in candidates[:k]]
    out = sorted(buffers, key=lambda b: b[1])[::-1]                      # :117-121
    return [(torch.cat([v.select(0, v.shape[0] - 1) for v, _, _ in seq]).view(len(seq)), lp) for seq, lp in out]   # :122-130
