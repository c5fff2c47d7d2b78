"""lamp.nn's recurrent family over the host C ABI: RNN, GRU, LSTM, SeqLinear, statefulSequence, SequenceNLL, FreeRunningRNN, Seq2Seq, WithInit.

Reference: lamp-core/src/main/scala/lamp/nn/{RNN,GRU,LSTM,SeqLinear,StatefulSeq,FreeRunningRNN,Seq2Seq}.scala, LossFunctions.scala:76-108.
Inputs are [time, batch, in]; a stateful module's forward takes (x, state) and returns (output, nextState), `None` for the reference's None.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

from ._capi import lib, handle_array
from .autograd import Variable
from .nn import Module, _mk
from .sten import STen, F32

SEQUENCE_NLL = 3   # loss_kind of SupervisedModel: LossFunctions.SequenceNLL(numClasses, classWeights, ignore)


def recurrentFused(on: bool) -> bool:
    """process-wide: one node per sequence over the fused cell kernels (True, the default unless LAMP_RECURRENT_FUSED=0) or the
    reference's fold over the time steps out of the plain operators; returns the previous setting."""
    prev = C.c_int(0); lib.lamp_recurrent_fused(int(bool(on)), C.byref(prev)); return bool(prev.value)


class StatefulModule(Module):
    def __init__(self, m: Module):
        super().__init__(m.h); m.h = None

    @property
    def initState(self) -> Optional[Tuple[Variable, ...]]:
        """InitState: None for the reference's None, the carried state of a WithInit"""
        cap = max(1, self.stateSlots)
        out = (C.c_void_p * cap)(); n = C.c_int(0)
        lib.lamp_module_init_state(self.h, out, C.byref(n))
        return tuple(Variable(C.c_void_p(out[i])) for i in range(n.value)) if n.value else None

    @property
    def stateSlots(self) -> int:
        n = C.c_int(0); lib.lamp_module_num_state_slots(self.h, C.byref(n)); return n.value

    def forward(self, x: Variable, state: Optional[Sequence[Optional[Variable]]] = None) -> Tuple[Variable, Tuple[Variable, ...]]:
        """StatefulModule.forward((x, state)) -> (output, nextState)."""
        n = self.stateSlots
        st = list(state) if state is not None else []
        assert len(st) in (0, n), f"{n} state slots, got {len(st)} Variables"
        arr = (C.c_void_p * max(1, len(st)))(*[(v.h if v is not None else None) for v in st])
        o = C.c_void_p()
        so = (C.c_void_p * max(1, n))()
        lib.lamp_module_forward_stateful(self.h, x.h, arr, len(st), C.byref(o), so)
        return Variable(o), tuple(Variable(C.c_void_p(so[i])) for i in range(n))


def _from(fn: str, tensors: Sequence[STen]) -> Module:
    m = _mk(fn, handle_array([t.h for t in tensors]), len(tensors))
    m._keep = list(tensors)
    return m


class RNN(StatefulModule):
    """RNN.apply (RNN.scala:65-93) or, with `tensors`, the case class over (weightXh, weightHh, biasH)."""
    def __init__(self, in_=None, hiddenSize=None, dtype=F32, device=0, tensors: Optional[Sequence[STen]] = None):
        super().__init__(_from("lamp_module_rnn_from", tensors) if tensors is not None else _mk("lamp_module_rnn", in_, hiddenSize, dtype, device))


class GRU(StatefulModule):
    """GRU.apply (GRU.scala:93-165) or the case class over its nine tensors in `state` order."""
    def __init__(self, in_=None, hiddenSize=None, dtype=F32, device=0, tensors: Optional[Sequence[STen]] = None):
        super().__init__(_from("lamp_module_gru_from", tensors) if tensors is not None else _mk("lamp_module_gru", in_, hiddenSize, dtype, device))


class LSTM(StatefulModule):
    """LSTM.apply (LSTM.scala:119-213) or the case class over its twelve tensors in `state` order; state = (h, c)."""
    def __init__(self, in_=None, hiddenSize=None, dtype=F32, device=0, tensors: Optional[Sequence[STen]] = None):
        super().__init__(_from("lamp_module_lstm_from", tensors) if tensors is not None else _mk("lamp_module_lstm", in_, hiddenSize, dtype, device))


def SeqLinear(in_=None, out=None, dtype=F32, device=0, tensors: Optional[Sequence[STen]] = None) -> Module:
    """SeqLinear.apply (SeqLinear.scala:44-64): a linear map of every time step."""
    return _from("lamp_module_seq_linear_from", tensors) if tensors is not None else _mk("lamp_module_seq_linear", in_, out, dtype, device)


class statefulSequence(StatefulModule):
    """statefulSequence(m1, ..., mn) (StatefulSeq.scala); stateless members are lifted.  The state is the members' states side by side."""
    def __init__(self, *mods: Module):
        super().__init__(_mk("lamp_module_stateful_sequence", handle_array([m.h for m in mods]), len(mods)))
        self._mods = mods


class FreeRunningRNN(StatefulModule):
    """FreeRunningRNN(module, timeSteps) (FreeRunningRNN.scala): forward(x [T0, B] int64, state) -> (outputs [timeSteps, B, V], lastState), greedy
    generation as a differentiable composition of the wrapped module's forward.  state, load and the training mode are the wrapped module's."""
    def __init__(self, module: StatefulModule, timeSteps: int):
        super().__init__(_mk("lamp_module_free_running_rnn", module.h, int(timeSteps)))
        self.module, self.timeSteps = module, int(timeSteps)


class Seq2Seq(StatefulModule):
    """Seq2Seq(encoder, decoder) (Seq2Seq.scala:6-28): forward((source, dest), state0) = decoder.forward(dest, encoder.forward(source, state0).state);
    state = encoder.state ++ decoder.state."""
    def __init__(self, encoder: StatefulModule, decoder: StatefulModule):
        super().__init__(_mk("lamp_module_seq2seq", encoder.h, decoder.h))
        self.encoder, self.decoder = encoder, decoder

    def forward(self, x: Tuple[Variable, Variable], state: Optional[Sequence[Optional[Variable]]] = None) -> Tuple[Variable, Tuple[Variable, ...]]:
        source, dest = x
        n = self.stateSlots
        st = list(state) if state is not None else []
        assert len(st) in (0, n), f"{n} state slots, got {len(st)} Variables"
        arr = (C.c_void_p * max(1, len(st)))(*[(v.h if v is not None else None) for v in st])
        o = C.c_void_p()
        so = (C.c_void_p * max(1, n))()
        lib.lamp_module_forward_stateful_pair(self.h, source.h, dest.h, arr, len(st), C.byref(o), so)
        return Variable(o), tuple(Variable(C.c_void_p(so[i])) for i in range(n))


class WithInit(StatefulModule):
    """WithInit(module, init) (Seq2Seq.scala:75-114): the module with an initial state of its own (`initState`)"""
    def __init__(self, module: StatefulModule, init: Sequence[Variable]):
        init = list(init)
        super().__init__(_mk("lamp_module_with_init", module.h, handle_array([v.h for v in init]), len(init)))
        self.module, self._init = module, init
