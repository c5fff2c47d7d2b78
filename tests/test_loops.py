"""The training drivers' bookkeeping without a GPU (lamp_amd.loops.epochs / swaEpochs / withSWA over scripted per-epoch passes, on a
module whose state lives in host memory), the SWA learning-rate schedules, and the loop-state files (lamp_amd.data.writeLoopState /
readLoopState) on host tensors.  What is checked against IOLoops.scala:305-605, SWA.scala:24-324 and StateIO.scala:
the smoothing s = last or this, smoothed = this * f + s * (1 - f); the minimum tracked only over returnMinValidationLossModel's epochs;
a snapshot on a strict improvement only; the stop rule epoch >= epochs or factor <= 0; the curves; the files' field names."""
import json
import os

import numpy as np
import pytest

from lamp_amd import data as D, loops, nn, sten as S
from lamp_amd.loops import SimpleLoopState, SimpleThenSWALoopState, SWALearningRateSchedule, SWALoopState, TrainingLoopContext


def _host(a, dtype=None):
    return S.STen.from_numpy(np.asarray(a), device=S.CPU, dtype=dtype)


class _Var:
    needsGrad = True

    def __init__(self, value): self.value = value


class _Module:
    """two host state tensors; the scripted training pass writes the epoch number into them, so a snapshot says when it was taken"""

    def __init__(self):
        self.state = [_Var(_host(np.full((3,), -1.0, np.float32))), _Var(_host(np.full((2, 2), -1.0, np.float64)))]
        self.parameters = self.state

    def asTraining(self): return self

    def load(self, tensors):
        assert len(tensors) == len(self.state)
        for v, t in zip(self.state, tensors):
            v.value.copyFrom(t)

    def stamp(self): return [float(v.value.to_numpy().reshape(-1)[0]) for v in self.state]


class _Model:
    def __init__(self): self.module = _Module()


class _Optimizer:
    def __init__(self, params): self.params, self.state, self.loaded = params, [_host(np.zeros(1, np.float32))], None

    def load(self, tensors): self.loaded = tensors


class _Script:
    """the two per-epoch passes, scripted: training loss 10 - epoch, validation losses from a list; records what they were handed"""

    def __init__(self, validation):
        self.validation, self.factors, self.contexts = list(validation or []), [], []

    def train(self, epochCount, model, optimizer, trainBatches, learningRateScheduleFactor, accumulateGradientOverNBatches, trainingCallback, logger):
        self.factors.append((epochCount, learningRateScheduleFactor))
        self.contexts.append(trainBatches)
        for v in model.module.state:
            v.value.fill_(float(epochCount))
        loss = 10.0 - epochCount
        if trainingCallback is not None:
            trainingCallback(epochCount, loss, model.module)
        return loss

    def validate(self, model, validationBatches, epochCount, validationCallback, logger):
        loss = float(self.validation[epochCount])
        if validationCallback is not None:
            validationCallback(epochCount, loss)
        return loss


def _run_epochs(validation, n, **kw):
    script, model = _Script(validation), _Model()
    log = []
    out = loops.epochs(model, _Optimizer, lambda ctx: ctx, (lambda ctx: ctx) if validation is not None else None, n, logger=log.append,
                       _trainEpoch=script.train, _validationEpoch=script.validate, **kw)
    return out, script, model, [int(line.rsplit(" ", 1)[1]) for line in log if line.startswith("Copying model at epoch")]


# ---- the SWA schedules -----------------------------------------------------------------------------------------------------------------------
def test_swa_constant_schedule():
    s = SWALearningRateSchedule.constant(0.3)
    for epoch in (0, 1, 7, 1000):
        state, f, accumulate = s.swaLearningRateSchedule(s.init, epoch, None)
        assert f == 0.3 and accumulate is True


def test_swa_cyclic_schedule():
    lo, hi, L = 0.01, 1.0, 4
    s = SWALearningRateSchedule.cyclic(lo, hi, L)
    accumulated = []
    for epoch in range(9):
        state, f, accumulate = s.swaLearningRateSchedule(s.init, epoch, 0.5)
        t = (epoch % L + 1) / L
        assert f == (1 - t) * hi + t * lo, (epoch, f)
        if accumulate:
            accumulated.append(epoch)
    assert accumulated == [3, 7]


def test_training_loop_context():
    assert TrainingLoopContext.empty() == TrainingLoopContext(0, None, None)


# ---- epochs ----------------------------------------------------------------------------------------------------------------------------------
LOSSES = [5.0, 3.0, 4.0, 2.0, 6.0]


def test_epochs_minimum_model_and_curve():
    seen = []
    (epochReturned, model, curve, lrState, done), script, m, copies = _run_epochs(
        LOSSES, 5, returnMinValidationLossModel={0, 1, 2, 4}, validationLossExponentialSmoothingFactor=1.0,
        validationCallback=lambda e, loss, module: seen.append((e, loss, module)))
    assert copies == [0, 1]                                   # epoch 3 has the smallest loss but is not in the set; 2 and 4 are no improvement
    assert epochReturned == 1 and done.minValidationLoss == 3.0
    assert curve == [(e, 10.0 - e, (v, v)) for e, v in enumerate(LOSSES)]
    assert m.module.stamp() == [1.0, 1.0]                     # the module holds the snapshot of epoch 1
    assert done.epoch == 5 and done.lastValidationLoss == 6.0 and done.model == [] and done.optimizer == [] and done.minValidationLossModel is None
    assert done.learningCurve == curve[::-1]                  # the loop state keeps it newest first
    assert script.factors == [(e, 1.0) for e in range(5)]
    # the contexts the stream factories were handed: last and minimum loss as of the epoch's start
    assert script.contexts == [TrainingLoopContext(0, None, None), TrainingLoopContext(1, 5.0, 5.0), TrainingLoopContext(2, 3.0, 3.0),
                               TrainingLoopContext(3, 4.0, 3.0), TrainingLoopContext(4, 2.0, 3.0)]
    # the callback: once from the validation pass, once from the driver with the smoothed loss, both with the module
    assert [(e, loss) for e, loss, _ in seen] == [(e, v) for e, v in enumerate(LOSSES) for _ in (0, 1)] and all(mod is m.module for _, _, mod in seen)


def test_epochs_without_minimum_model_returns_the_last_epoch():
    (epochReturned, _, curve, _, done), _, m, copies = _run_epochs(LOSSES, 5)
    assert copies == [] and epochReturned == 4 and done.minValidationLoss is None and m.module.stamp() == [4.0, 4.0]


def test_epochs_smoothing():
    f = 0.5
    (epochReturned, _, curve, _, done), _, _, copies = _run_epochs(LOSSES, 5, returnMinValidationLossModel=range(5),
                                                                   validationLossExponentialSmoothingFactor=f)
    last, want = None, []
    for v in LOSSES:
        s = last if last is not None else v
        last = v * f + s * (1.0 - f)
        want.append(last)
    assert [c[2][0] for c in curve] == want and [c[2][1] for c in curve] == LOSSES
    # smoothed: 5, 4, 4, 3, 4.5 - strict improvements at 0, 1 and 3 (4 at epoch 2 ties the minimum: no snapshot)
    assert want == [5.0, 4.0, 4.0, 3.0, 4.5]
    assert copies == [0, 1, 3] and epochReturned == 3 and done.minValidationLoss == 3.0


def test_epochs_validation_frequency():
    handed = []

    def fn(state, epoch, loss):
        handed.append((epoch, loss))
        return None, 1.0
    (epochReturned, _, curve, _, _), _, _, _ = _run_epochs(LOSSES, 5, validationFrequency=2, learningRateSchedule=nn.LearningRateSchedule(None, fn))
    assert [c[2] for c in curve] == [(5.0, 5.0), None, (4.0, 4.0), None, (6.0, 6.0)]
    # the schedule sees None after an epoch without validation
    assert handed == [(0, None), (1, 5.0), (2, None), (3, 4.0), (4, None), (5, 6.0)]
    assert epochReturned == 4


def test_epochs_stops_when_the_factor_reaches_zero():
    schedule = nn.LearningRateSchedule.fromEpochCount(lambda e: 0.0 if e == 2 else 0.5)
    (epochReturned, _, curve, _, done), script, _, _ = _run_epochs(LOSSES, 5, learningRateSchedule=schedule)
    assert epochReturned == 1 and [c[0] for c in curve] == [0, 1] and done.epoch == 2
    assert script.factors == [(0, 0.5), (1, 0.5)]


def test_epochs_without_validation():
    (epochReturned, _, curve, _, _), _, _, _ = _run_epochs(None, 3, returnMinValidationLossModel=range(3))
    assert epochReturned == 2 and curve == [(0, 10.0, None), (1, 9.0, None), (2, 8.0, None)]


def test_epochs_checkpoints_and_resumes():
    states = []
    (_, _, curve, _, _), _, _, _ = _run_epochs(LOSSES, 5, returnMinValidationLossModel=range(5),
                                               checkpointState=lambda s, lr: states.append((s, lr)))
    assert [s.epoch for s, _ in states] == [1, 2, 3, 4, 5]
    s2 = states[1][0]                                          # after epoch 1
    assert s2.lastValidationLoss == 3.0 and s2.minValidationLoss == 3.0 and s2.minValidationLossModel[0] == 1
    assert [c[0] for c in s2.learningCurve] == [1, 0]
    # resume from it: epochs 2..4 run, the curve and the returned epoch (3: loss 2) are those of the uninterrupted run
    snapshot = SimpleLoopState([_host(v.value.to_numpy()) for v in _Module().state], [], s2.epoch, s2.lastValidationLoss, s2.minValidationLoss,
                               s2.minValidationLossModel, s2.learningCurve)
    (epochReturned, _, resumed, _, _), script, _, copies = _run_epochs(LOSSES, 5, returnMinValidationLossModel=range(5), initState=snapshot)
    assert resumed == curve and epochReturned == 3 and copies == [3] and [e for e, _ in script.factors] == [2, 3, 4]


# ---- swaEpochs / withSWA ---------------------------------------------------------------------------------------------------------------------
def test_swa_epochs_average_on_the_host():
    """state after epoch e is the constant e: constant(1.0) over 3 epochs averages 0, 1, 2 -> 1; cyclic(.., 2) over 4 averages 1 and 3 -> 2"""
    for schedule, n, want in ((SWALearningRateSchedule.constant(1.0), 3, 1.0), (SWALearningRateSchedule.cyclic(0.1, 1.0, 2), 4, 2.0)):
        script, model = _Script(LOSSES), _Model()
        states = []
        _, curve = loops.swaEpochs(model, _Optimizer, lambda ctx: ctx, lambda ctx: ctx, n, learningRateSchedule=schedule, forwardPassAfterTraining=False,
                                   checkpointState=lambda s, lr: states.append((s.epoch, s.numberOfAveragedModels, s.averagedModels is not None)),
                                   _trainEpoch=script.train, _validationEpoch=script.validate)
        assert model.module.stamp() == [want, want]
        assert curve == [(e, 10.0 - e, LOSSES[e]) for e in range(n)]
        if n == 3:
            assert states == [(0, 0, False), (1, 1, True), (2, 2, True)]      # the checkpoint comes before the epoch
        else:
            assert states == [(0, 0, False), (1, 0, False), (2, 1, True), (3, 1, True)]


def test_with_swa_concatenates_the_curves():
    script, model = _Script(LOSSES), _Model()
    states = []
    epochReturned, m, curve, warmed = loops.withSWA(model, _Optimizer, lambda ctx: ctx, 2, 3, validationBatchesOverEpoch=lambda ctx: ctx,
                                                    learningRateSchedule=nn.LearningRateSchedule.noop(), swaLearningRateSchedule=SWALearningRateSchedule.constant(1.0),
                                                    checkpointState=lambda s, lr: states.append(s), swaForwardPassAfterTraining=False,
                                                    _trainEpoch=script.train, _validationEpoch=script.validate)
    assert [c[0] for c in curve] == [0, 1, 2, 3, 4] and epochReturned == 1 and m is model and warmed is model
    assert curve[:2] == [(0, 10.0, (5.0, 5.0)), (1, 9.0, (3.0, 3.0))]
    # the SWA phase counts its epochs from 0 again (the script's losses with it); its validation entries are doubled
    assert curve[2:] == [(2, 10.0, (5.0, 5.0)), (3, 9.0, (3.0, 3.0)), (4, 8.0, (4.0, 4.0))]
    assert all(isinstance(s, SimpleThenSWALoopState) for s in states)
    assert [s.swa is None for s in states] == [True, True, False, False, False]
    assert [s.swa.epoch for s in states[2:]] == [0, 1, 2] and all(s.simple.epoch == 2 for s in states[2:])
    assert model.module.stamp() == [1.0, 1.0]                 # the average of the SWA phase's states 0, 1, 2

    # resumed inside the SWA phase: the warm-up is skipped
    inside = states[3]
    script2, model2 = _Script(LOSSES), _Model()
    resume = SimpleThenSWALoopState(inside.simple, SWALoopState([_host(np.full((3,), 0.0, np.float32)), _host(np.zeros((2, 2)))], [], 1, inside.swa.lastValidationLoss,
                                                                inside.swa.minValidationLoss, 1, [_host(np.full((3,), 0.0, np.float32)), _host(np.zeros((2, 2)))],
                                                                inside.swa.learningCurve))
    _, _, curve2, _ = loops.withSWA(model2, _Optimizer, lambda ctx: ctx, 2, 3, validationBatchesOverEpoch=lambda ctx: ctx,
                                    learningRateSchedule=nn.LearningRateSchedule.noop(), swaLearningRateSchedule=SWALearningRateSchedule.constant(1.0),
                                    initState=resume, swaForwardPassAfterTraining=False, _trainEpoch=script2.train, _validationEpoch=script2.validate)
    assert [e for e, _ in script2.factors] == [1, 2] and curve2 == curve and model2.module.stamp() == [1.0, 1.0]


# ---- loop-state files ------------------------------------------------------------------------------------------------------------------------
def _tensors(salt):
    return [_host(np.arange(6, dtype=np.float32).reshape(2, 3) + salt), _host(np.arange(5, dtype=np.int64) * salt), _host(np.array([salt + 0.25])),
            _host(np.zeros((0, 4), np.float32))]


def _same_tensors(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.to_numpy().tobytes() == y.to_numpy().tobytes()


def _same_simple(a, b):
    _same_tensors(a.model, b.model), _same_tensors(a.optimizer, b.optimizer)
    assert (a.epoch, a.lastValidationLoss, a.minValidationLoss, a.learningCurve) == (b.epoch, b.lastValidationLoss, b.minValidationLoss, b.learningCurve)
    assert (a.minValidationLossModel is None) == (b.minValidationLossModel is None)
    if a.minValidationLossModel is not None:
        assert a.minValidationLossModel[0] == b.minValidationLossModel[0]
        _same_tensors(a.minValidationLossModel[1], b.minValidationLossModel[1])


def _same_swa(a, b):
    _same_tensors(a.model, b.model), _same_tensors(a.optimizer, b.optimizer)
    assert (a.epoch, a.lastValidationLoss, a.minValidationLoss, a.numberOfAveragedModels, a.learningCurve) == \
           (b.epoch, b.lastValidationLoss, b.minValidationLoss, b.numberOfAveragedModels, b.learningCurve)
    assert (a.averagedModels is None) == (b.averagedModels is None)
    if a.averagedModels is not None:
        _same_tensors(a.averagedModels, b.averagedModels)


def _simple(full):
    if full:
        return SimpleLoopState(_tensors(1), _tensors(2)[:2], 3, 0.1 + 0.2, 1e-300, (1, _tensors(3)), [(2, 0.5, (0.25, 1.0 / 3.0)), (1, 0.75, None), (0, 1.5, (2.0, 2.5))])
    return SimpleLoopState(_tensors(1), [], 0, None, None, None, [])


def _swa(full):
    if full:
        return SWALoopState(_tensors(4), _tensors(5)[:1], 7, 0.3, 0.2, 2, _tensors(6), [(1, 0.5, 1.0 / 3.0), (0, 0.75, None)])
    return SWALoopState(_tensors(4), [], 0, None, None, 0, None, [])


@pytest.mark.parametrize("full", [True, False])
def test_loop_state_file_simple(tmp_path, full):
    file, state = str(tmp_path / "state"), _simple(full)
    D.writeLoopState(file, state)
    _same_simple(D.readLoopState(file, S.CPU), state)
    d = json.load(open(file))
    assert d["type"] == "SimpleLoopState" and list(d)[:4] == ["type", "model", "optimizer", "epoch"]
    assert set(d["model"]) == {"tensors", "location", "byteOffset", "byteLength"} and d["model"]["location"] == "state.model"
    assert set(d["model"]["tensors"][0]) == {"dims", "dataType", "byteOffset", "byteLength"} and d["optimizer"]["location"] == "state.optimizer"
    if full:
        assert set(d) == {"type", "model", "optimizer", "epoch", "lastValidationLoss", "minValidationLoss", "minValidationLossModel", "learningCurve"}
        assert d["minValidationLossModel"][0] == 1 and d["minValidationLossModel"][1]["location"] == "state.minvalidmodel"
        assert d["learningCurve"] == [[2, 0.5, 0.25, 1.0 / 3.0], [1, 0.75, None, None], [0, 1.5, 2.0, 2.5]]
        assert sorted(os.listdir(tmp_path)) == ["state", "state.minvalidmodel", "state.model", "state.optimizer"]
    else:
        assert set(d) == {"type", "model", "optimizer", "epoch"}      # absent options and empty lists are left out
        assert sorted(os.listdir(tmp_path)) == ["state", "state.model", "state.optimizer"]


@pytest.mark.parametrize("full", [True, False])
def test_loop_state_file_swa(tmp_path, full):
    file, state = str(tmp_path / "state"), _swa(full)
    D.writeLoopState(file, state)
    _same_swa(D.readLoopState(file, S.CPU), state)
    d = json.load(open(file))
    assert d["type"] == "SWALoopState" and d["numberOfAveragedModels"] == state.numberOfAveragedModels
    if full:
        assert set(d) == {"type", "model", "optimizer", "epoch", "lastValidationLoss", "minValidationLoss", "numberOfAveragedModels", "averagedModels",
                          "learningCurve"}
        assert d["averagedModels"]["location"] == "state.averagemodel" and d["learningCurve"] == [[1, 0.5, 1.0 / 3.0], [0, 0.75, None]]
    else:
        assert set(d) == {"type", "model", "optimizer", "epoch", "numberOfAveragedModels"}


@pytest.mark.parametrize("full", [True, False])
def test_loop_state_file_simple_then_swa(tmp_path, full):
    file = str(tmp_path / "state")
    state = SimpleThenSWALoopState(_simple(full), _swa(True) if full else None)
    D.loopStateToFile(file)(state, None)                      # the ready-made checkpointState
    got = D.readLoopState(file, S.CPU)
    _same_simple(got.simple, state.simple)
    assert (got.swa is None) == (state.swa is None)
    d = json.load(open(file))
    assert d["type"] == "SimpleThenSWALoopState" and "type" not in d["simple"] and d["simple"]["model"]["location"] == "state.simple.model"
    if full:
        _same_swa(got.swa, state.swa)
        assert set(d) == {"type", "simple", "swa"} and "type" not in d["swa"] and d["swa"]["averagedModels"]["location"] == "state.swa.averagemodel"
    else:
        assert set(d) == {"type", "simple"}
    # written again over itself (a checkpoint per epoch): still one consistent set of files
    D.writeLoopState(file, state)
    _same_simple(D.readLoopState(file, S.CPU).simple, state.simple)


def test_loop_state_file_rejects_other_objects(tmp_path):
    with pytest.raises(TypeError):
        D.writeLoopState(str(tmp_path / "x"), {"epoch": 1})
