"""The reference's recurrent modules restated with torch on the CPU, fold by fold (lamp-core/src/main/scala/lamp/nn).

Weights are lists in the order of the modules' `state`; a state of None is the reference's None (zeros).  Everything is computed in
the dtype of the tensors handed in (the tests hand in f64)."""
import torch


def rnn(x, w, h0=None):                                      # RNN.scala:36-50
    wxh, whh, bh = w
    h = h0 if h0 is not None else torch.zeros(x.shape[1], whh.shape[0], dtype=whh.dtype)   # RNN.scala:27-29
    outputs = []
    for t in range(x.shape[0]):                              # RNN.scala:38
        xt = x.select(0, t)                                  # :39
        h = (xt.mm(wxh) + h.mm(whh) + bh).tanh()             # :40
        outputs.append(h)                                    # :42
    return torch.stack(outputs, 0), h                        # :45


def gru(x, w, h0=None):                                      # GRU.scala:45-64
    wxh, whh, wxr, wxz, whr, whz, br, bz, bh = w             # GRU.scala:27-38
    h = h0 if h0 is not None else torch.zeros(x.shape[1], whh.shape[0], dtype=whh.dtype)
    outputs = []
    for t in range(x.shape[0]):                              # :50
        xt = x.select(0, t)                                  # :51
        r = (xt.mm(wxr) + h.mm(whr) + br).sigmoid()          # :52
        z = (xt.mm(wxz) + h.mm(whz) + bz).sigmoid()          # :53
        hcap = (xt.mm(wxh) + (r * h).mm(whh) + bh).tanh()    # :54
        h = z * h + ((z * -1) + 1.0) * hcap                  # :56
        outputs.append(h)
    return torch.stack(outputs, 0), h                        # :62


def lstm(x, w, state=None):                                  # LSTM.scala:56-84
    wxi, wxf, wxo, whi, whf, who, wxc, whc, bi, bf, bo, bc = w   # LSTM.scala:28-42
    if state is None:                                        # LSTM.scala:44-52
        h = torch.zeros(x.shape[1], whf.shape[0], dtype=whf.dtype)
        c = torch.zeros(x.shape[1], whf.shape[0], dtype=whf.dtype)
    else:
        h, c = state
    outputs = []
    for t in range(x.shape[0]):                              # :65
        xt = x.select(0, t)                                  # :66
        it = (xt.mm(wxi) + h.mm(whi) + bi).sigmoid()         # :67
        ft = (xt.mm(wxf) + h.mm(whf) + bf).sigmoid()         # :68
        ot = (xt.mm(wxo) + h.mm(who) + bo).sigmoid()         # :69
        ccap = (xt.mm(wxc) + h.mm(whc) + bc).tanh()          # :71
        c = ft * c + it * ccap                               # :73
        h = ot * c.tanh()                                    # :74
        outputs.append(h)
    return torch.stack(outputs, 0), h, c                     # :79-82


def seq_linear(x, w):                                        # SeqLinear.scala:22-29
    weight, bias = w
    return torch.stack([x.select(0, t).mm(weight) + bias for t in range(x.shape[0])], 0)


def sequence_nll(out, target, class_weights, ignore=-100):   # LossFunctions.scala:84-107
    losses, total = [], 0
    for t in range(out.shape[0]):
        t1 = target.select(0, t)
        total += out.shape[1] - int((t1 == ignore).sum())
        losses.append(torch.nn.functional.nll_loss(out.select(0, t), t1, class_weights, reduction="sum", ignore_index=ignore))
    return sum(losses) * (1.0 / total), total
