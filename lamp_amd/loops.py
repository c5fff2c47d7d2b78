"""lamp-data's epoch loops and training drivers over the host C ABI.

Mirror of lamp.data.IOLoops.oneEpoch / validationOneEpoch (lamp-data/src/main/scala/lamp/data/IOLoops.scala:607-750, :751-830), of
the per-batch body of distributed.oneEpoch (distributed/package.scala:733-780), and of the drivers above them: IOLoops.epochs
(:305-605), IOLoops.withSWA (:169-303), SWA.epochs (SWA.scala:50-324) and forwardAndDiscardBatchStream (IOLoops.scala:30-62).  The loops are host glue in the reference as well (Scala
on the JVM); every batch is one or two calls into liblamp_hip.so:

  accumulateGradientOverNBatches <= 1   lamp_model_train_step  (gradients + optional RCCL exchange + optimizer.step)
  accumulateGradientOverNBatches  > 1   lamp_model_gradients(zero_grad = 0) per batch, optimizer.step + zeroGrad every N-th batch
  validation                            lamp_model_forward_loss on the module in eval mode

The reference's `prefetch` / `overlapModelWithLoad` switches hide the host gather + PCIe copy of the next minibatch; with the data set
resident in HBM (lamp_amd.data.BatchStream) a minibatch is one gather kernel on the same stream and there is nothing to hide.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Callable, Collection, List, Optional, Sequence, Tuple

from . import sten as S
from .autograd import const
from .data import BatchStream
from .nn import LearningRateSchedule, Optimizer, SupervisedModel, stateKernelsFused, stateSnapshot, swaAverage  # noqa: F401  (the switch is re-exported)


def oneEpoch(epochCount: int, model: SupervisedModel, optimizer: Optimizer, trainBatches: BatchStream, learningRateScheduleFactor: float = 1.0,
             accumulateGradientOverNBatches: int = 1, trainingCallback: Optional[Callable] = None, logger: Optional[Callable[[str], None]] = None,
             comm=None) -> float:
    """One pass over `trainBatches`; returns the average training loss (sum of loss * numInstances over the batches / instances)."""
    first = model.module.state[0].value
    lossAcc = S.STen.zeros([1], S.F64, first.device)        # STen.scalarDouble(0, options): f64 whatever the model type (IOLoops.scala:715)
    numInstances, batchCount = 0, 0
    t1 = time.perf_counter()
    trainBatches.reset()
    if accumulateGradientOverNBatches > 1:
        model.module.zeroGrad()
    for sample, target in trainBatches:
        if accumulateGradientOverNBatches <= 1:
            n = model.train_step(optimizer, sample, target, lossAcc, comm, learningRateScheduleFactor)
        else:
            assert comm is None, "gradient accumulation is a single-process option in the reference (IOLoops.oneEpoch)"
            n, grads = model.addTotalLossAndReturnGradientsAndNumExamples(sample, target, lossAcc, False)
            if batchCount % accumulateGradientOverNBatches == accumulateGradientOverNBatches - 1:
                optimizer.step(grads, learningRateScheduleFactor)
                model.module.zeroGrad()
        numInstances += n
        batchCount += 1
    totalLoss = float(lossAcc.to_numpy().reshape(-1)[0])
    trainingLoss = totalLoss / max(numInstances, 1)
    if logger is not None:
        seconds = time.perf_counter() - t1
        logger(f"Avg training loss in epoch {epochCount} over {numInstances} examples: {trainingLoss} ({numInstances / seconds:.2f} instances/sec)")
    if trainingCallback is not None:
        trainingCallback(epochCount, trainingLoss, model.module)
    return trainingLoss


def validationOneEpoch(model: SupervisedModel, validationBatches: BatchStream, epochCount: int = 0, validationCallback: Optional[Callable] = None,
                       logger: Optional[Callable[[str], None]] = None) -> float:
    """Average validation loss with the module in eval mode (restored to training mode afterwards, as `model.asEval` is a copy there)."""
    first = model.module.state[0].value
    totalLoss = S.STen.zeros([1], S.F64, first.device)      # f64 accumulator (IOLoops.scala:809)
    totalExamples = 0
    model.module.asEval()
    try:
        validationBatches.reset()
        for sample, target in validationBatches:
            totalExamples += model.addTotalLossAndReturnNumExamples(sample, target, totalLoss)
    finally:
        model.module.asTraining()
    validationLoss = float(totalLoss.to_numpy().reshape(-1)[0]) / max(totalExamples, 1)
    if logger is not None:
        logger(f"Avg validation loss in epoch {epochCount} over {totalExamples} examples: {validationLoss}")
    if validationCallback is not None:
        validationCallback(epochCount, validationLoss)
    return validationLoss


# ---- the drivers above the epoch loops ---------------------------------------------------------------------------------------------------
# Bookkeeping only: the learning-rate schedule, the smoothed validation loss, the model of the smallest validation loss, the weight
# average, checkpoints.  The device work is oneEpoch / validationOneEpoch plus three operations on the whole module state - snapshot,
# running mean, load - which are one multi-tensor launch each (nn.stateSnapshot, nn.swaAverage, Module.load; nn.stateKernelsFused).
# Not mirrored: dataParallelModels (the multi-device drivers are DataParallel.oneEpoch / distributed.*), prefetch / overlapModelWithLoad
# (see the header), printOptimizerAllocations.
# `_trainEpoch` / `_validationEpoch` are the two per-epoch passes, oneEpoch / validationOneEpoch unless overridden (a test scripts the
# losses through them and runs the bookkeeping without a GPU); they are called with the keyword arguments of those two functions.
@dataclass(frozen=True)
class TrainingLoopContext:
    """what the batch-stream factories are handed every epoch (IOLoops.scala:21-28)"""
    epoch: int
    lastValidationLoss: Optional[float]
    minValidationLoss: Optional[float]

    @staticmethod
    def empty() -> "TrainingLoopContext":
        return TrainingLoopContext(0, None, None)


# LoopState.scala.  `learningCurve` is kept as the loops build it, newest epoch FIRST (the drivers return it reversed, in epoch order)
@dataclass
class SimpleLoopState:
    model: List[S.STen]
    optimizer: List[S.STen]
    epoch: int
    lastValidationLoss: Optional[float]
    minValidationLoss: Optional[float]
    minValidationLossModel: Optional[Tuple[int, List[S.STen]]]
    learningCurve: List[Tuple[int, float, Optional[Tuple[float, float]]]]      # (epoch, training loss, (smoothed, unsmoothed) validation loss)


@dataclass
class SWALoopState:
    model: List[S.STen]
    optimizer: List[S.STen]
    epoch: int
    lastValidationLoss: Optional[float]
    minValidationLoss: Optional[float]
    numberOfAveragedModels: int
    averagedModels: Optional[List[S.STen]]
    learningCurve: List[Tuple[int, float, Optional[float]]]


@dataclass
class SimpleThenSWALoopState:
    simple: SimpleLoopState
    swa: Optional[SWALoopState]


def forwardAndDiscardBatchStream(batchStream, module) -> None:
    """IOLoops.forwardAndDiscardBatchStream: one forward per batch in the module's current mode, values discarded; in training mode the
    batch-norm running statistics are refreshed as a side effect (what SWA needs after the weights were replaced by their average)."""
    batchStream.reset()
    for sample, _ in batchStream:
        module.forward(const(sample) if isinstance(sample, S.STen) else sample)


def epochs(model: SupervisedModel, optimizerFactory: Callable[[Sequence[S.STen]], Optimizer], trainBatchesOverEpoch: Callable[[TrainingLoopContext], BatchStream],
           validationBatchesOverEpoch: Optional[Callable[[TrainingLoopContext], BatchStream]], epochs: int, trainingCallback: Optional[Callable] = None,
           validationCallback: Optional[Callable] = None, checkpointState: Optional[Callable] = None, validationFrequency: int = 1,
           logger: Optional[Callable[[str], None]] = None, returnMinValidationLossModel: Collection[int] = (),
           learningRateSchedule: Optional[LearningRateSchedule] = None, initState: Optional[SimpleLoopState] = None,
           accumulateGradientOverNBatches: int = 1, learningRateScheduleInitState=None, validationLossExponentialSmoothingFactor: float = 1.0,
           _trainEpoch: Optional[Callable] = None, _validationEpoch: Optional[Callable] = None):
    """IOLoops.epochs (IOLoops.scala:305-605): train until `epochs` or until the schedule's factor is <= 0, validating every
    `validationFrequency` epochs; returns (epochReturned, model, learningCurve, lrState, doneLoopState).  With epochs in
    `returnMinValidationLossModel`, the state at the smallest smoothed validation loss among those epochs is snapshotted on every strict
    improvement and loaded back into the module on return; epochReturned is then that epoch, otherwise the last one trained.
    Callbacks: trainingCallback(epoch, trainingLoss, module); validationCallback(epoch, loss, module), called - as in the reference - by
    the validation pass with the unsmoothed loss and then here with the smoothed one; checkpointState(SimpleLoopState, lrState) after
    every epoch, with epoch + 1 and the schedule state this epoch started from."""
    schedule = learningRateSchedule if learningRateSchedule is not None else LearningRateSchedule.noop()
    trainEpoch = _trainEpoch if _trainEpoch is not None else oneEpoch
    validationEpoch = _validationEpoch if _validationEpoch is not None else validationOneEpoch
    returnMin = set(returnMinValidationLossModel)
    smoothing = float(validationLossExponentialSmoothingFactor)
    module = model.module
    module.asTraining()
    optimizer = optimizerFactory([p.value for p in module.parameters])
    if initState is not None:
        module.load(initState.model)
        optimizer.load(initState.optimizer)
        epoch, lastValidationLoss, minValidationLoss = initState.epoch, initState.lastValidationLoss, initState.minValidationLoss
        minValidationLossModel, learningCurve = initState.minValidationLossModel, list(initState.learningCurve)
        lrState = learningRateScheduleInitState if learningRateScheduleInitState is not None else schedule.init
    else:
        epoch, lastValidationLoss, minValidationLoss, minValidationLossModel, learningCurve, lrState = 0, None, None, None, [], schedule.init
    passValidationCallback = None if validationCallback is None else (lambda e, loss: validationCallback(e, loss, module))

    while True:
        nextLrState, learningRateFactor = schedule.learningRateFactor(lrState, epoch, lastValidationLoss)
        if epoch >= epochs or learningRateFactor <= 0.0:
            doneLoopState = SimpleLoopState([], [], epoch, lastValidationLoss, minValidationLoss, None, learningCurve)
            if minValidationLossModel is None:
                return epoch - 1, model, learningCurve[::-1], nextLrState, doneLoopState
            module.load(minValidationLossModel[1])
            return minValidationLossModel[0], model, learningCurve[::-1], nextLrState, doneLoopState

        ctx = TrainingLoopContext(epoch, lastValidationLoss, minValidationLoss)
        trainingLoss = trainEpoch(epochCount=epoch, model=model, optimizer=optimizer, trainBatches=trainBatchesOverEpoch(ctx),
                                  learningRateScheduleFactor=learningRateFactor, accumulateGradientOverNBatches=accumulateGradientOverNBatches,
                                  trainingCallback=trainingCallback, logger=logger)
        maybeValidationLoss = None
        if epoch % validationFrequency == 0 and validationBatchesOverEpoch is not None:
            unsmoothed = validationEpoch(model=model, validationBatches=validationBatchesOverEpoch(ctx), epochCount=epoch,
                                         validationCallback=passValidationCallback, logger=logger)
            s = lastValidationLoss if lastValidationLoss is not None else unsmoothed
            maybeValidationLoss = (unsmoothed * smoothing + s * (1.0 - smoothing), unsmoothed)
            if validationCallback is not None:
                validationCallback(epoch, maybeValidationLoss[0], module)

        candidate = epoch in returnMin and maybeValidationLoss is not None
        nextMinValidationLoss = minValidationLoss
        nextMinValidationLossModel = minValidationLossModel
        if candidate:
            if minValidationLoss is None or minValidationLoss > maybeValidationLoss[0]:       # a strict improvement
                if logger is not None:
                    logger(f"Copying model at epoch {epoch}")
                nextMinValidationLossModel = (epoch, stateSnapshot([v.value for v in module.state]))
            nextMinValidationLoss = maybeValidationLoss[0] if minValidationLoss is None else min(minValidationLoss, maybeValidationLoss[0])
        nextLearningCurve = [(epoch, trainingLoss, maybeValidationLoss)] + learningCurve
        smoothedOrNone = None if maybeValidationLoss is None else maybeValidationLoss[0]
        if checkpointState is not None:
            checkpointState(SimpleLoopState([v.value for v in module.state], optimizer.state, epoch + 1, smoothedOrNone, nextMinValidationLoss,
                                            nextMinValidationLossModel, nextLearningCurve), lrState)
        epoch, lastValidationLoss, minValidationLoss = epoch + 1, smoothedOrNone, nextMinValidationLoss
        minValidationLossModel, learningCurve, lrState = nextMinValidationLossModel, nextLearningCurve, nextLrState


class SWALearningRateSchedule:
    """SWA.SWALearningRateSchedule (SWA.scala:15-48): swaLearningRateSchedule(state, epoch, lastValidationLoss) returns
    (next state, factor, accumulate) - `accumulate`: this epoch's weights enter the average."""

    def __init__(self, init, fn):
        self.init = init
        self._fn = fn

    def swaLearningRateSchedule(self, state, epoch: int, lastValidationLoss: Optional[float] = None):
        return self._fn(state, epoch, lastValidationLoss)

    @staticmethod
    def constant(f: float) -> "SWALearningRateSchedule":
        return SWALearningRateSchedule(None, lambda state, epoch, loss: (None, float(f), True))

    @staticmethod
    def cyclic(minFactor: float, maxFactor: float, cycleLength: int) -> "SWALearningRateSchedule":
        """falls linearly from near maxFactor to minFactor over every cycle; the last epoch of a cycle is averaged"""
        def f(state, epoch, loss):
            t = 1.0 / cycleLength * ((epoch % cycleLength) + 1)
            return None, (1 - t) * maxFactor + t * minFactor, epoch % cycleLength + 1 == cycleLength
        return SWALearningRateSchedule(None, f)


def swaEpochs(model: SupervisedModel, optimizerFactory: Callable[[Sequence[S.STen]], Optimizer], trainBatchesOverEpoch: Callable[[TrainingLoopContext], BatchStream],
              validationBatchesOverEpoch: Optional[Callable[[TrainingLoopContext], BatchStream]], epochs: int, trainingCallback: Optional[Callable] = None,
              validationCallback: Optional[Callable] = None, checkpointState: Optional[Callable] = None, validationFrequency: int = 1,
              logger: Optional[Callable[[str], None]] = None, learningRateSchedule: Optional[SWALearningRateSchedule] = None,
              initState: Optional[SWALoopState] = None, accumulateGradientOverNBatches: int = 1, learningRateScheduleInitState=None,
              forwardPassAfterTraining: bool = True, _trainEpoch: Optional[Callable] = None, _validationEpoch: Optional[Callable] = None):
    """SWA.epochs (SWA.scala:50-324), stochastic weight averaging (arXiv 1803.05407): after every epoch the schedule marks with
    `accumulate`, the module state enters a running mean - the first time as a snapshot, afterwards ((avg * n) + current) / (n + 1) in
    place on the accumulator.  On return the module holds the average; with forwardPassAfterTraining one more pass over the training
    batches refreshes the batch-norm statistics for the averaged weights.  Returns (model, learningCurve) with entries
    (epoch, training loss, validation loss | None).  checkpointState(SWALoopState, lrState) is called BEFORE every epoch, as there."""
    schedule = learningRateSchedule if learningRateSchedule is not None else SWALearningRateSchedule.constant(1.0)
    trainEpoch = _trainEpoch if _trainEpoch is not None else oneEpoch
    validationEpoch = _validationEpoch if _validationEpoch is not None else validationOneEpoch
    module = model.module
    module.asTraining()
    optimizer = optimizerFactory([p.value for p in module.parameters])
    if initState is not None:
        module.load(initState.model)
        optimizer.load(initState.optimizer)
        epoch, lastValidationLoss, minValidationLoss = initState.epoch, initState.lastValidationLoss, initState.minValidationLoss
        numberOfAveragedModels, averagedModels, learningCurve = initState.numberOfAveragedModels, initState.averagedModels, list(initState.learningCurve)
    else:
        epoch, lastValidationLoss, minValidationLoss, numberOfAveragedModels, averagedModels, learningCurve = 0, None, None, 0, None, []
    lrState = learningRateScheduleInitState if learningRateScheduleInitState is not None else schedule.init
    passValidationCallback = None if validationCallback is None else (lambda e, loss: validationCallback(e, loss, module))

    while True:
        nextLrState, learningRateFactor, accumulate = schedule.swaLearningRateSchedule(lrState, epoch, lastValidationLoss)
        if epoch >= epochs or learningRateFactor <= 0.0:
            if averagedModels is not None:
                module.load(averagedModels)
            break
        if checkpointState is not None:
            checkpointState(SWALoopState([v.value for v in module.state], optimizer.state, epoch, lastValidationLoss, minValidationLoss,
                                         numberOfAveragedModels, averagedModels, learningCurve), lrState)
        ctx = TrainingLoopContext(epoch, lastValidationLoss, minValidationLoss)
        trainingLoss = trainEpoch(epochCount=epoch, model=model, optimizer=optimizer, trainBatches=trainBatchesOverEpoch(ctx),
                                  learningRateScheduleFactor=learningRateFactor, accumulateGradientOverNBatches=accumulateGradientOverNBatches,
                                  trainingCallback=trainingCallback, logger=logger)
        maybeValidationLoss = None
        if epoch % validationFrequency == 0 and validationBatchesOverEpoch is not None:
            maybeValidationLoss = validationEpoch(model=model, validationBatches=validationBatchesOverEpoch(ctx), epochCount=epoch,
                                                  validationCallback=passValidationCallback, logger=logger)
            if validationCallback is not None:
                validationCallback(epoch, maybeValidationLoss, module)
            minValidationLoss = maybeValidationLoss if minValidationLoss is None else min(minValidationLoss, maybeValidationLoss)
        if accumulate:
            current = [v.value for v in module.state]
            averagedModels = stateSnapshot(current) if averagedModels is None else swaAverage(averagedModels, current, numberOfAveragedModels)
            numberOfAveragedModels += 1
        learningCurve = [(epoch, trainingLoss, maybeValidationLoss)] + learningCurve
        epoch, lastValidationLoss, lrState = epoch + 1, maybeValidationLoss, nextLrState

    learningCurve = learningCurve[::-1]
    if forwardPassAfterTraining:
        forwardAndDiscardBatchStream(trainBatchesOverEpoch(TrainingLoopContext(len(learningCurve), None, None)), module)
    return model, learningCurve


_swaEpochs = swaEpochs      # withSWA has a parameter of that name


def withSWA(model: SupervisedModel, optimizerFactory: Callable[[Sequence[S.STen]], Optimizer], trainBatchesOverEpoch: Callable[[TrainingLoopContext], BatchStream],
            warmupEpochs: int, swaEpochs: int, validationBatchesOverEpoch: Optional[Callable[[TrainingLoopContext], BatchStream]] = None,
            trainingCallback: Optional[Callable] = None, validationCallback: Optional[Callable] = None, checkpointState: Optional[Callable] = None,
            logger: Optional[Callable[[str], None]] = None, returnMinValidationLossModel: Collection[int] = (),
            learningRateSchedule: Optional[LearningRateSchedule] = None, swaLearningRateSchedule: Optional[SWALearningRateSchedule] = None,
            initState: Optional[SimpleThenSWALoopState] = None, accumulateGradientOverNBatches: int = 1, learningRateScheduleInitState=None,
            swaLearningRateScheduleInitState=None, swaForwardPassAfterTraining: bool = True, validationLossExponentialSmoothingFactor: float = 1.0,
            _trainEpoch: Optional[Callable] = None, _validationEpoch: Optional[Callable] = None):
    """IOLoops.withSWA (IOLoops.scala:169-303): `warmupEpochs` of `epochs`, then `swaEpochs` of weight averaging on the warmed-up model;
    returns (warmupEpochReturned, model, learningCurve, model).  The curve is the warm-up's followed by the SWA phase's, its epochs offset
    by max(warm-up epoch) + 1 and its validation entries doubled to (x, x).  checkpointState(SimpleThenSWALoopState, lrState) is called
    in both phases (`state.swa is None` says which schedule the lrState belongs to); an initState whose `swa` is set resumes straight
    into the SWA phase.  The SWA schedule starts from the warm-up's final state only when that has the type of its own `init`.
    One departure from the reference: on such a resume the warm-up curve is put back into epoch order (the reference concatenates it
    newest first, as the loop state holds it)."""
    schedule = learningRateSchedule if learningRateSchedule is not None else LearningRateSchedule.decrement(20, 0.5)
    swaSchedule = swaLearningRateSchedule if swaLearningRateSchedule is not None else SWALearningRateSchedule.cyclic(0.01, 1.0, 10)
    if initState is not None and initState.swa is not None:
        simple = initState.simple
        warmupEpochReturned, warmupLearningCurve, warmupLoopState = simple.epoch, list(simple.learningCurve)[::-1], simple
        warmupLRState = learningRateScheduleInitState if learningRateScheduleInitState is not None else schedule.init
    else:
        warmupEpochReturned, _, warmupLearningCurve, warmupLRState, warmupLoopState = epochs(
            model, optimizerFactory, trainBatchesOverEpoch, validationBatchesOverEpoch, warmupEpochs, trainingCallback, validationCallback,
            None if checkpointState is None else (lambda s, lr: checkpointState(SimpleThenSWALoopState(s, None), lr)), 1, logger,
            returnMinValidationLossModel, schedule, None if initState is None else initState.simple, accumulateGradientOverNBatches,
            learningRateScheduleInitState, validationLossExponentialSmoothingFactor, _trainEpoch, _validationEpoch)
    if swaLearningRateScheduleInitState is not None:
        swaLRInit = swaLearningRateScheduleInitState
    elif type(swaSchedule.init) is type(warmupLRState):
        swaLRInit = warmupLRState
    else:
        swaLRInit = None
    _, swaLearningCurve = _swaEpochs(
        model, optimizerFactory, trainBatchesOverEpoch, validationBatchesOverEpoch, swaEpochs, trainingCallback, validationCallback,
        None if checkpointState is None else (lambda s, lr: checkpointState(SimpleThenSWALoopState(warmupLoopState, s), lr)), 1, logger,
        swaSchedule, None if initState is None else initState.swa, accumulateGradientOverNBatches, swaLRInit, swaForwardPassAfterTraining,
        _trainEpoch, _validationEpoch)
    m = max((e for e, _, _ in warmupLearningCurve), default=-1) + 1
    concatLearningCurve = list(warmupLearningCurve) + [(e + m, l1, None if l2 is None else (l2, l2)) for e, l1, l2 in swaLearningCurve]
    return warmupEpochReturned, model, concatLearningCurve, model
