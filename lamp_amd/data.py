"""lamp-data over the host C ABI: tensor-list files, checkpoints, the CIFAR record reader and the minibatch stream.

Mirror of lamp.data.{Writer, Reader, BatchStream} and example-cifar100's Cifar.loadImageFile:
  Writer.writeTensorsIntoFile / writeCheckpoint        lamp-data/src/main/scala/lamp/data/Writer.scala:143-190
  Reader.readTensorsFromFile / loadFromFile            lamp-data/src/main/scala/lamp/data/Reader.scala:62-95
  BatchStream.minibatchesFromFull, everyNth            lamp-data/src/main/scala/lamp/data/BatchStream.scala:528-592, :378-400
  Cifar.loadImageFile                                  example-cifar100/src/main/scala/lamp/example/cifar/cifar100.scala:29-56
  StateIO.writeToFile / readFromFile / stateToFile     lamp-data/src/main/scala/lamp/data/StateIO.scala:16-303 (JSON glue over the tensor-list files)
Every other function is one call into liblamp_hip.so (lamp_amd/csrc/host/data.cpp).
"""
from __future__ import annotations

import ctypes as C
import json
import os
import tempfile
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

from ._capi import lib, handle_array
from .sten import STen, F32


def writeTensorsIntoFile(tensors: Sequence[STen], file: str) -> None:
    lib.lamp_write_tensors_into_file(handle_array([t.h for t in tensors]), len(tensors), str(file).encode())


def readTensorsFromFile(file: str, device: int = -1, pin: bool = False) -> List[STen]:
    n = C.c_int64()
    lib.lamp_tensor_list_length(str(file).encode(), C.byref(n))
    out = (C.c_void_p * max(n.value, 1))()
    got = C.c_int64()
    lib.lamp_read_tensors_from_file(out, n.value, C.byref(got), str(file).encode(), device, int(pin))
    return [STen(out[i]) for i in range(got.value)]


def writeCheckpoint(file: str, model) -> None:
    lib.lamp_module_write_checkpoint(model.h, str(file).encode())


def loadFromFile(module, file: str) -> None:
    lib.lamp_module_load_from_file(module.h, str(file).encode())


# ---- loop-state files (StateIO.scala:16-297, schemas/schemas.scala:58-101) -------------------------------------------------------------------
# `file` holds a JSON descriptor with the reference's field names: a three-way union tagged by "type" (jsoniter-scala's default
# discriminator: the case-class name), tensor lists as the TensorList descriptors of the tensor-list files, tuples as arrays, absent
# options and empty lists left out (None inside a tuple is null).  The tensors of every list go through writeTensorsIntoFile into a file
# of their own beside the descriptor: <name>.model, <name>.optimizer, <name>.minvalidmodel, <name>.averagemodel, with <name> =
# <file>.simple / <file>.swa inside a SimpleThenSWALoopState.  Compatibility with a file the reference wrote is unverified (DESIGN.md
# section 21): its tree holds no loop-state fixture.
def _write_tensor_list(tensors: Sequence[STen], directory: str, location: str) -> dict:
    tmp = os.path.join(directory, location + ".tmp")
    writeTensorsIntoFile(tensors, tmp)                       # the descriptor in `tmp`, the tensor data in `tmp`.data
    with open(tmp) as f:
        descriptor = json.load(f)
    os.replace(tmp + ".data", os.path.join(directory, location))
    os.remove(tmp)
    descriptor["location"] = location
    return descriptor


def _read_tensor_list(descriptor: dict, directory: str, device: int) -> List[STen]:
    location = descriptor["location"]
    absolute = dict(descriptor, location=location if os.path.isabs(location) else os.path.abspath(os.path.join(directory, location)))
    with tempfile.TemporaryDirectory() as scratch:
        path = os.path.join(scratch, "tensors")
        with open(path, "w") as f:
            json.dump(absolute, f)
        return readTensorsFromFile(path, device)


def _without_absent(fields: dict) -> dict:
    return {k: v for k, v in fields.items() if v is not None and v != []}


def _simple_descriptor(s, directory: str, name: str) -> dict:
    minValid = None
    if s.minValidationLossModel is not None:
        minValid = [int(s.minValidationLossModel[0]), _write_tensor_list(s.minValidationLossModel[1], directory, name + ".minvalidmodel")]
    return _without_absent({
        "type": "SimpleLoopState",
        "model": _write_tensor_list(s.model, directory, name + ".model"),
        "optimizer": _write_tensor_list(s.optimizer, directory, name + ".optimizer"),
        "epoch": int(s.epoch), "lastValidationLoss": s.lastValidationLoss, "minValidationLoss": s.minValidationLoss,
        "minValidationLossModel": minValid,
        "learningCurve": [[int(e), float(t), None if v is None else float(v[0]), None if v is None else float(v[1])] for e, t, v in s.learningCurve]})


def _swa_descriptor(s, directory: str, name: str) -> dict:
    return _without_absent({
        "type": "SWALoopState",
        "model": _write_tensor_list(s.model, directory, name + ".model"),
        "optimizer": _write_tensor_list(s.optimizer, directory, name + ".optimizer"),
        "epoch": int(s.epoch), "lastValidationLoss": s.lastValidationLoss, "minValidationLoss": s.minValidationLoss,
        "numberOfAveragedModels": int(s.numberOfAveragedModels),
        "averagedModels": None if s.averagedModels is None else _write_tensor_list(s.averagedModels, directory, name + ".averagemodel"),
        "learningCurve": [[int(e), float(t), None if v is None else float(v)] for e, t, v in s.learningCurve]})


def writeLoopState(file: str, state) -> None:
    """StateIO.writeToFile: a loops.SimpleLoopState / SWALoopState / SimpleThenSWALoopState into `file` and the tensor files beside it"""
    from . import loops
    file = os.path.abspath(str(file))
    directory, name = os.path.dirname(file), os.path.basename(file)
    if isinstance(state, loops.SimpleLoopState):
        descriptor = _simple_descriptor(state, directory, name)
    elif isinstance(state, loops.SWALoopState):
        descriptor = _swa_descriptor(state, directory, name)
    elif isinstance(state, loops.SimpleThenSWALoopState):
        simple = _simple_descriptor(state.simple, directory, name + ".simple")
        swa = None if state.swa is None else _swa_descriptor(state.swa, directory, name + ".swa")
        del simple["type"]                                  # the members' types are fixed: no discriminator inside
        if swa is not None:
            del swa["type"]
        descriptor = _without_absent({"type": "SimpleThenSWALoopState", "simple": simple, "swa": swa})
    else:
        raise TypeError(f"not a loop state: {type(state).__name__}")
    with open(file + ".tmp", "w") as f:
        json.dump(descriptor, f, separators=(",", ":"))
    os.replace(file + ".tmp", file)


def readLoopState(file: str, device: int = 0):
    """StateIO.readFromFile: the loop state in `file` with its tensors on `device` (-1: the host), to be handed to a driver as initState"""
    from . import loops
    file = os.path.abspath(str(file))
    directory = os.path.dirname(file)
    with open(file) as f:
        descriptor = json.load(f)
    tensors = lambda d: _read_tensor_list(d, directory, device)

    def simple(d):
        mv = d.get("minValidationLossModel")
        return loops.SimpleLoopState(tensors(d["model"]), tensors(d["optimizer"]), int(d["epoch"]), d.get("lastValidationLoss"), d.get("minValidationLoss"),
                                     None if mv is None else (int(mv[0]), tensors(mv[1])),
                                     [(int(e), float(t), None if a is None or b is None else (float(a), float(b))) for e, t, a, b in d.get("learningCurve", [])])

    def swa(d):
        avg = d.get("averagedModels")
        return loops.SWALoopState(tensors(d["model"]), tensors(d["optimizer"]), int(d["epoch"]), d.get("lastValidationLoss"), d.get("minValidationLoss"),
                                  int(d["numberOfAveragedModels"]), None if avg is None else tensors(avg),
                                  [(int(e), float(t), None if v is None else float(v)) for e, t, v in d.get("learningCurve", [])])

    kind = descriptor.get("type")
    if kind == "SimpleLoopState":
        return simple(descriptor)
    if kind == "SWALoopState":
        return swa(descriptor)
    if kind == "SimpleThenSWALoopState":
        return loops.SimpleThenSWALoopState(simple(descriptor["simple"]), None if descriptor.get("swa") is None else swa(descriptor["swa"]))
    raise ValueError(f"{file}: unknown loop state type {kind!r}")


def loopStateToFile(file: str):
    """StateIO.stateToFile: the ready-made `checkpointState` of loops.epochs / swaEpochs / withSWA - (state, lrState) -> writeLoopState(file, state).
    The learning-rate schedule's state is not part of the file, as in the reference."""
    return lambda state, lrState=None: writeLoopState(file, state)


def loadImageFile(file: str, numImages: int, dtype: int = F32, device: int = 0) -> Tuple[STen, STen]:
    """Cifar.loadImageFile: (fine labels i64 [n], images [n, 3, 32, 32])."""
    lab, img = C.c_void_p(), C.c_void_p()
    lib.lamp_cifar_load_image_file(C.byref(lab), C.byref(img), str(file).encode(), int(numImages), dtype, device)
    return STen(lab), STen(img)


class JavaRandom:
    """java.util.Random's documented 48-bit LCG (what scala.util.Random wraps), so that a Python driver can draw the shuffles a
    JVM driver would for the same seed.  Not pinned against a JVM here (none in the image)."""

    def __init__(self, seed: int):
        self.seed = (seed ^ 0x5DEECE66D) & ((1 << 48) - 1)

    def _next(self, bits: int) -> int:
        self.seed = (self.seed * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
        v = self.seed >> (48 - bits)
        return v - (1 << bits) if v >= (1 << (bits - 1)) and bits == 32 else v

    def nextInt(self, bound: int) -> int:
        assert bound > 0
        if bound & (bound - 1) == 0:
            return (bound * self._next(31)) >> 31
        while True:
            bits = self._next(31)
            val = bits % bound
            if bits - val + (bound - 1) < (1 << 31):
                return val

    def shuffle(self, xs: Sequence[int]) -> List[int]:
        """scala.util.Random.shuffle (2.13): for n = length down to 2, swap(n - 1, nextInt(n))."""
        buf = list(xs)
        for n in range(len(buf), 1, -1):
            k = self.nextInt(n)
            buf[n - 1], buf[k] = buf[k], buf[n - 1]
        return buf


class BatchStream:
    """BatchStream over a device-resident data set; iterate to get (features, target) STen pairs until EndStream."""

    def __init__(self, handle):
        self.h = handle.value if isinstance(handle, C.c_void_p) else handle

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                lib.lamp_batch_stream_release(h)
            except Exception:
                pass

    @staticmethod
    def minibatchesFromFull(minibatchSize: int, dropLast: bool, features: STen, target: STen, rng=None, device: int = 0,
                            order: Optional[Sequence[int]] = None, hostResident: bool = False, outDtype: int = -1) -> "BatchStream":
        """`rng`: an object with shuffle(list) -> list (JavaRandom, or anything else); `order` overrides it.  hostResident: the features
        stay in (pinned) host memory as in the reference and every minibatch is gathered over PCIe one batch ahead, converted to outDtype."""
        n = features.shape[0]
        if order is None:
            order = rng.shuffle(list(range(n))) if rng is not None else list(range(n))
        arr = np.ascontiguousarray(order, dtype=np.int64)
        o = C.c_void_p()
        if hostResident:
            lib.lamp_batch_stream_from_full_host(C.byref(o), features, target, arr.ctypes.data_as(C.POINTER(C.c_int64)), len(arr), int(minibatchSize),
                                                 int(bool(dropLast)), device, int(outDtype))
        else:
            lib.lamp_batch_stream_from_full(C.byref(o), features, target, arr.ctypes.data_as(C.POINTER(C.c_int64)), len(arr), int(minibatchSize),
                                            int(bool(dropLast)), device)
        return BatchStream(o)

    def everyNth(self, n: int, offset: int) -> "BatchStream":
        lib.lamp_batch_stream_every_nth(self.h, int(n), int(offset))
        return self

    @property
    def numBatches(self) -> int:
        n = C.c_int64(); lib.lamp_batch_stream_num_batches(self.h, C.byref(n)); return n.value

    def nextBatch(self) -> Optional[Tuple[STen, STen]]:
        x, y = C.c_void_p(), C.c_void_p()
        lib.lamp_batch_stream_next(self.h, C.byref(x), C.byref(y))
        return None if not x.value else (STen(x), STen(y))

    def reset(self) -> None:
        lib.lamp_batch_stream_reset(self.h)

    def __iter__(self) -> Iterator[Tuple[STen, STen]]:
        while True:
            b = self.nextBatch()
            if b is None:
                return
            yield b
