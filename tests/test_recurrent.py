"""Recurrent family, the part that needs no GPU: the torch restatement (tests/recurrent_ref.py) pinned to the reference's own
deterministic test and to finite differences, and the new entry points of the C ABI."""
import torch

from tests import recurrent_ref as R
from tests.util import closed_form

F64 = torch.float64


def test_rnn_shape_and_loss_known_answer():
    """nn.test.scala:618-644 ("RNN shape and loss"): all-ones RNN on arange(12).view(2, 3, 2), SequenceNLL against all-ones targets."""
    x = torch.arange(12, dtype=F64).view(2, 3, 2)
    w = [torch.ones(2, 4, dtype=F64), torch.ones(4, 4, dtype=F64), torch.ones(4, dtype=F64)]
    out, _ = R.rnn(x, w)
    assert list(out.shape) == [2, 3, 4]
    loss, n = R.sequence_nll(out, torch.ones(2, 3, dtype=torch.int64), torch.ones(4, dtype=F64))
    assert n == 6
    assert loss.item() == -0.9940025479340507


def _weights(shapes, salt):
    return [closed_form(s, salt + 13 * i, 1.0, F64) for i, s in enumerate(shapes)]


CASES = {
    "rnn": (lambda x, w: R.rnn(x, w)[0], [(2, 4), (4, 4), (4,)]),
    "gru": (lambda x, w: R.gru(x, w)[0], [(2, 4), (4, 4), (2, 4), (2, 4), (4, 4), (4, 4), (4,), (4,), (4,)]),
    "lstm": (lambda x, w: R.lstm(x, w)[0], [(2, 4)] * 3 + [(4, 4)] * 3 + [(2, 4), (4, 4)] + [(4,)] * 4),
    "seq_linear": (lambda x, w: R.seq_linear(x, w), [(2, 4), (4,)]),
}


def _check_fd(name):
    """testGradientAndValueND (nn.test.scala:105-190): central differences with eps 1e-6 agree with autograd to 4 decimals."""
    f, shapes = CASES[name]
    x = closed_form((2, 3, 2), 5, 2.0, F64)
    w = [t.requires_grad_(True) for t in _weights(shapes, 17)]
    f(x, w).sum().backward()
    eps = 1e-6
    for k, p in enumerate(w):
        flat = p.detach().reshape(-1)
        fd = torch.zeros_like(flat)
        for j in range(flat.numel()):
            def at(d):
                q = flat.clone(); q[j] += d
                ws = [t.detach() for t in w]; ws[k] = q.reshape(p.shape)
                return f(x, ws).sum().item()
            fd[j] = (at(eps) - at(-eps)) / (2 * eps)
        assert torch.equal(torch.round(fd.reshape(p.shape) * 1e4), torch.round(p.grad * 1e4)), \
            f"{name}: gradient of state tensor {k} differs from central differences by {(fd.reshape(p.shape) - p.grad).abs().max().item():.3e}"


def test_rnn_gradient_finite_differences(): _check_fd("rnn")
def test_gru_gradient_finite_differences(): _check_fd("gru")
def test_lstm_gradient_finite_differences(): _check_fd("lstm")
def test_seq_linear_gradient_finite_differences(): _check_fd("seq_linear")


def test_sequence_nll_divides_by_the_total_count():
    """LossFunctions.scala:104-106: one division by the count over all time steps, also when a whole step is ignored."""
    out = torch.log_softmax(closed_form((3, 4, 5), 3, 2.0, F64), 2)
    target = torch.tensor([[0, 1, 2, 3], [-100, -100, -100, -100], [4, -100, 1, 0]])
    loss, n = R.sequence_nll(out, target, torch.ones(5, dtype=F64))
    assert n == 7
    keep = target != -100
    want = -out[keep].gather(1, target[keep].unsqueeze(1)).sum() / 7
    assert abs(loss.item() - want.item()) < 1e-14


def test_recurrent_entry_points_exported():
    from lamp_amd._capi import lib
    lib.load()
    names = ["lamp_module_rnn", "lamp_module_gru", "lamp_module_lstm", "lamp_module_seq_linear", "lamp_module_stateful_sequence",
             "lamp_module_lstm_from", "lamp_module_forward_stateful", "lamp_module_num_state_slots", "lamp_recurrent_fused",
             "lamp_lstm_cell_forward", "lamp_lstm_cell_backward", "lamp_gru_gates_forward", "lamp_gru_output_forward",
             "lamp_gru_output_backward", "lamp_gru_gates_backward", "lamp_rnn_cell_forward", "lamp_rnn_cell_backward"]
    for n in names:
        assert n in lib.decls, f"{n} is not declared in include/*.h"
        assert n not in lib.missing, f"{n} is declared but not exported by the library"
