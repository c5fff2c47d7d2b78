"""The training drivers on the GPU (lamp_amd.loops.epochs / swaEpochs / withSWA / forwardAndDiscardBatchStream) on the model of
tests/test_data.py::test_one_epoch_loops: MLP(20, 4, [16]) with batch norm + logsoftmax, NLL, 96 examples in minibatches of 16, AdamW at
1e-2, lamp_manual_seed(11), the batch order a function of ctx.epoch.  Everything is compared bit for bit: against hand-written oneEpoch
calls, against the states the callbacks recorded, against the chain of the library's own operators for the weight average, and a
resumed run against the uninterrupted one."""
import numpy as np
import pytest

from lamp_amd import autograd as A, data as D, loops, nn, sten as S
from lamp_amd._capi import lib
from lamp_amd.loops import SWALearningRateSchedule, TrainingLoopContext

pytestmark = pytest.mark.gpu
N = 96


@pytest.fixture(scope="module")
def examples(gpu):
    rng = np.random.default_rng(0)
    x = S.STen.from_numpy(rng.standard_normal((N, 20)).astype(np.float32), 0)
    y = S.STen.from_numpy((np.arange(N) % 4).astype(np.int64), 0)
    return x, y


def _make():
    lib.lamp_manual_seed(11)
    net = nn.Sequential(nn.MLP(20, 4, [16], S.F32, 0), nn.Fun("logsoftmax", 1))
    return net, nn.SupervisedModel(net, nn.SupervisedModel.NLL, S.STen.ones([4], S.F32, 0))


class Factory:
    """AdamW at 1e-2; keeps the optimisers it made so that a test can read their state"""

    def __init__(self): self.made = []

    def __call__(self, params):
        self.made.append(nn.AdamW_factory(weightDecay=0.0, learningRate=1e-2)(params))
        return self.made[-1]


def _order(epoch):
    return np.random.default_rng(100 + epoch).permutation(N).tolist()


def _train(examples):
    return lambda ctx: D.BatchStream.minibatchesFromFull(16, False, examples[0], examples[1], order=_order(ctx.epoch))


def _valid(examples):
    return lambda ctx: D.BatchStream.minibatchesFromFull(32, False, examples[0], examples[1], order=list(range(N)))


def _bits(tensors):
    return [t.to_numpy().tobytes() for t in tensors]


def _state(net):
    return _bits([v.value for v in net.state])


def _clones(module):
    return [v.value.cloneTensor() for v in module.state]


def _chain_average(states):
    """snapshot, mean(n = 1), mean(n = 2), ... out of the library's own operators"""
    avg = [t.cloneTensor() for t in states[0]]
    for n, cur in enumerate(states[1:], start=1):
        avg = [(a * float(n)).add(c, 1.0) / float(n + 1) for a, c in zip(avg, cur)]
    return avg


def test_epochs_is_the_hand_written_loop(examples):
    schedule = nn.LearningRateSchedule.decrement(1, 0.5)     # factors 1, 0.5, 0.25
    net, model = _make()
    epochReturned, returned, curve, _, done = loops.epochs(model, Factory(), _train(examples), None, 3, learningRateSchedule=schedule)
    net2, model2 = _make()
    opt2 = Factory()([p.value for p in net2.parameters])
    losses = [loops.oneEpoch(e, model2, opt2, _train(examples)(TrainingLoopContext(e, None, None)), 0.5 ** e) for e in range(3)]
    assert _state(net) == _state(net2)
    assert curve == [(e, losses[e], None) for e in range(3)] and epochReturned == 2 and returned is model and done.epoch == 3


def test_epochs_returns_the_minimum_validation_loss_model(examples):
    # the factor jumps to 50 (a learning rate of 0.5) at epoch 2: the validation loss rises there
    schedule = nn.LearningRateSchedule.fromEpochCount(lambda e: 1.0 if e < 2 else 50.0)
    recorded = {}
    net, model = _make()
    epochReturned, _, curve, _, done = loops.epochs(model, Factory(), _train(examples), _valid(examples), 4, returnMinValidationLossModel=range(4),
                                                    learningRateSchedule=schedule, validationLossExponentialSmoothingFactor=0.5,
                                                    validationCallback=lambda e, loss, module: recorded.__setitem__(e, _bits(_clones(module))))
    smoothed = [c[2][0] for c in curve]
    print(f"smoothed validation losses {smoothed}, unsmoothed {[c[2][1] for c in curve]}")
    best = smoothed.index(min(smoothed))                      # the first strict minimum
    assert best != len(smoothed) - 1, f"the validation loss fell to the last epoch, the test shows nothing: {smoothed}"
    assert epochReturned == best and done.minValidationLoss == smoothed[best]
    assert sorted(recorded) == [0, 1, 2, 3] and _state(net) == recorded[best]
    assert recorded[best] != recorded[3]


def _run(examples, n, factory, **kw):
    net, model = _make()
    out = loops.epochs(model, factory, _train(examples), _valid(examples), n, returnMinValidationLossModel=range(4), **kw)
    return net, out


def test_epochs_resumes_from_a_loop_state_file(examples, tmp_path):
    whole = Factory()
    net, (epochReturned, _, curve, _, _) = _run(examples, 4, whole)
    file = str(tmp_path / "loop")
    _run(examples, 2, Factory(), checkpointState=D.loopStateToFile(file))
    state = D.readLoopState(file, 0)
    assert state.epoch == 2 and [c[0] for c in state.learningCurve] == [1, 0] and state.minValidationLossModel is not None
    resumed = Factory()
    net2, (epochReturned2, _, curve2, _, _) = _run(examples, 4, resumed, initState=state)
    assert _state(net2) == _state(net) and _bits(resumed.made[0].state) == _bits(whole.made[0].state)
    assert curve2 == curve and epochReturned2 == epochReturned


@pytest.mark.parametrize("fused", [True, False])
def test_swa_epochs_average_is_the_chain(examples, fused):
    prev = loops.stateKernelsFused(fused)
    try:
        states = []
        net, model = _make()
        _, curve = loops.swaEpochs(model, Factory(), _train(examples), None, 3, learningRateSchedule=SWALearningRateSchedule.constant(1.0),
                                   forwardPassAfterTraining=False, trainingCallback=lambda e, loss, module: states.append(_clones(module)))
        assert len(states) == 3 and [c[0] for c in curve] == [0, 1, 2]
        assert _state(net) == _bits(_chain_average(states))
        assert _bits(states[0]) != _bits(states[2])
        # cyclic(.., 2) over 4 epochs: only epochs 1 and 3 enter the average
        states = []
        net, model = _make()
        loops.swaEpochs(model, Factory(), _train(examples), None, 4, learningRateSchedule=SWALearningRateSchedule.cyclic(0.1, 1.0, 2),
                        forwardPassAfterTraining=False, trainingCallback=lambda e, loss, module: states.append(_clones(module)))
        assert _state(net) == _bits(_chain_average([states[1], states[3]]))
        assert _state(net) != _bits(_chain_average(states))
    finally:
        loops.stateKernelsFused(prev)


def test_forward_pass_after_training_refreshes_the_running_statistics(examples):
    states = []
    net, model = _make()
    _, curve = loops.swaEpochs(model, Factory(), _train(examples), None, 2, learningRateSchedule=SWALearningRateSchedule.constant(1.0),
                               forwardPassAfterTraining=True, trainingCallback=lambda e, loss, module: states.append(_clones(module)))
    averaged = _chain_average(states)
    trained = [v.needsGrad for v in net.state]
    assert not all(trained) and any(trained)
    got = _state(net)
    assert [b for b, p in zip(got, trained) if p] == [b for b, p in zip(_bits(averaged), trained) if p]      # the parameters are the averaged ones
    # the running statistics: a training-mode forward over the same batches on a module that holds the average
    net2, _ = _make()
    net2.load(averaged)
    net2.asTraining()
    for x, _ in _train(examples)(TrainingLoopContext(len(curve), None, None)):
        net2.forward(A.const(x))
    assert _state(net2) == got
    assert [b for b, p in zip(got, trained) if not p] != [b for b, p in zip(_bits(averaged), trained) if not p]
    # forwardAndDiscardBatchStream alone changes nothing but the running statistics
    before = _state(net)
    loops.forwardAndDiscardBatchStream(_train(examples)(TrainingLoopContext(0, None, None)), net)
    after = _state(net)
    assert [b for b, p in zip(after, trained) if p] == [b for b, p in zip(before, trained) if p]
    assert [b for b, p in zip(after, trained) if not p] != [b for b, p in zip(before, trained) if not p]


def test_with_swa_resumes_inside_the_swa_phase(examples, tmp_path):
    files = []

    def checkpoint(state, lrState):
        files.append(str(tmp_path / f"loop{len(files)}"))
        D.writeLoopState(files[-1], state)

    kw = dict(warmupEpochs=2, swaEpochs=2, validationBatchesOverEpoch=_valid(examples), learningRateSchedule=nn.LearningRateSchedule.noop(),
              swaLearningRateSchedule=SWALearningRateSchedule.constant(0.5), returnMinValidationLossModel=range(2))
    net, model = _make()
    epochReturned, _, curve, _ = loops.withSWA(model, Factory(), _train(examples), checkpointState=checkpoint, **kw)
    assert len(files) == 4 and [c[0] for c in curve] == [0, 1, 2, 3]
    assert all(c[2][0] == c[2][1] for c in curve[2:])
    state = D.readLoopState(files[3], 0)                      # written before the SWA phase's second epoch
    assert state.swa is not None and state.swa.epoch == 1 and state.swa.numberOfAveragedModels == 1 and state.simple.epoch == 2
    trainedEpochs = []
    net2, model2 = _make()
    epochReturned2, _, curve2, _ = loops.withSWA(model2, Factory(), _train(examples), initState=state,
                                                 trainingCallback=lambda e, loss, module: trainedEpochs.append(e), **kw)
    assert trainedEpochs == [1]                               # no warm-up, and only the SWA epoch that was left
    assert _state(net2) == _state(net) and curve2 == curve
