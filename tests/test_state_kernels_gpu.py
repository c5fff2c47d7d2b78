"""The two multi-tensor state kernels of the training drivers (kernels/optim.hip: swa_average, state_copy) on the GPU.

swa_average against the chain of the library's own operators on the same inputs on the same GPU - tensor * n, add(.., cur, 1.0),
tensor / (n + 1) - bit for bit: every one of the three results is rounded to the tensor's dtype, the product is not contracted into the
addition, and the division is the true quotient lamp_div_scalar computes.  The shapes are the smallest at which the kernel can go
wrong: 0, 1, 3, 1023, 1024, 1025 and 2 * 1024 + 7 elements (below, at and over the 1024-element chunk, a chunk with no whole 16-byte
packet), bases one element off a 16-byte boundary (the element-wise path), 50 f32 tensors (two groups of 40), four dtypes in one call.
state_copy, the snapshot and Module.load bit for bit against their sources; the launch budget on the ResNet's 74 state tensors.

The per-tensor copies of the unfused forms are hipMemcpyAsync calls, which the kernel timer does not see: for them the budget test can
only assert that no state_copy launch appears; the unfused average shows as 3 element-wise launches per tensor."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from lamp_amd import nn, sten as S
from lamp_amd._capi import LampError, handle_array, lib
from tests.util import closed_form, to_sten, to_torch

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 1023, 1024, 1025, 2 * 1024 + 7]
FLOATS = [torch.float32, torch.float64, torch.bfloat16, torch.float16]
MT_MAX = 40


def _bits(t: S.STen) -> bytes:
    return t.to_numpy().tobytes()


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, i)
        assert torch.equal(to_torch(x), to_torch(y)) and _bits(x) == _bits(y), f"{what}: tensor {i} ({x.shape}, dtype {x.dtype}) differs"


def _off_by_one(t: torch.Tensor) -> S.STen:
    """a contiguous 1-D view that starts one element into its storage: its base is not on a 16-byte boundary"""
    n = t.numel()
    base = to_sten(torch.cat([t.reshape(-1)[:1], t.reshape(-1)]))
    view = base.slice(0, 1, n + 1)
    assert view.is_contiguous() and view.data_ptr % 16 != 0 and view.shape == [n]
    return view


def _values(n, salt, dt):
    # full mantissas in (-2, 2): avg * 7 is not representable in the dtype for most of them
    return closed_form((n,), salt, 4.0, dt)


def _swa_inputs():
    """(avg, cur) as torch tensors plus how to place each: 'a' aligned, 'm' both one element off, 'c' only cur off"""
    pairs = []
    salt = 0
    for dt in FLOATS:
        for n in SIZES:
            salt += 1
            pairs.append((_values(n, salt, dt), _values(n, 500 + salt, dt), "a"))
    for dt in (torch.float32, torch.bfloat16):
        pairs.append((_values(1030, 71, dt), _values(1030, 72, dt), "m"))
        pairs.append((_values(1030, 73, dt), _values(1030, 74, dt), "c"))
    for k in range(41):                                       # with the f32 tensors above: 50 of one class, two groups of MT_MAX
        pairs.append((_values(5, 200 + k, torch.float32), _values(5, 300 + k, torch.float32), "a"))
    return pairs


def _place(pairs):
    avg = [_off_by_one(a) if how == "m" else to_sten(a) for a, _, how in pairs]
    cur = [_off_by_one(c) if how in "mc" else to_sten(c) for _, c, how in pairs]
    return avg, cur


def _chain(avg, cur, n):
    """the library's own operators: what loops.swaEpochs runs per tensor with stateKernelsFused(False)"""
    return [(a * float(n)).add(c, 1.0) / float(n + 1) for a, c in zip(avg, cur)]


def _fused(avg, cur, n):
    lib.lamp_swa_average_(handle_array([t.h for t in avg]), handle_array([t.h for t in cur]), len(avg), n)
    return avg


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_the_inputs_tell_a_contracted_product_apart(dt):
    """on the CPU: for these inputs (avg * 7) + cur with the product rounded to the dtype differs from the sum of the exact product, so a
    kernel that contracts the product into the addition cannot pass the comparison below (n = 1 and 2 scale exactly and tell nothing)"""
    n = 7
    for size in (1025, 2 * 1024 + 7):
        avg, cur = _values(size, 3, dt), _values(size, 503, dt)
        rounded = (avg * n).to(dt) + cur
        contracted = (avg.double() * n + cur.double()).to(dt)
        assert rounded.dtype == dt and not torch.equal(rounded, contracted)
        assert not torch.equal((rounded / (n + 1)).to(dt), (contracted / (n + 1)).to(dt))
        assert not torch.equal((avg * n).to(dt).double(), avg.double() * n)          # avg * n is not representable


@pytest.mark.parametrize("n", [1, 2, 7])
def test_swa_average_is_the_chain_bit_for_bit(gpu, n):
    pairs = _swa_inputs()
    assert sum(1 for a, _, _ in pairs if a.dtype == torch.float32) > MT_MAX
    avg, cur = _place(pairs)
    want = _chain(avg, cur, n)
    before_cur = [_bits(c) for c in cur]
    got = _fused(avg, cur, n)
    _same(got, want, f"n = {n}")
    assert [_bits(c) for c in cur] == before_cur              # the current state is only read
    again_avg, again_cur = _place(pairs)
    _same(_fused(again_avg, again_cur, n), got, f"n = {n}, second run")


def test_swa_average_five_times_on_one_accumulator(gpu):
    sizes = [1025, 7, 2 * 1024 + 7]
    for dt in (torch.float32, torch.bfloat16):
        fused = [to_sten(_values(s, 11 + s, dt)) for s in sizes]
        chain = [to_sten(_values(s, 11 + s, dt)) for s in sizes]
        for n in range(1, 6):
            cur = [to_sten(_values(s, 1000 * n + s, dt)) for s in sizes]
            _fused(fused, cur, n)
            chain = _chain(chain, cur, n)
        _same(fused, chain, f"{dt}: five averages")


def _rejected(avg, cur, index, untouched):
    before = [_bits(t) for t in untouched]
    with pytest.raises(LampError) as e:
        lib.lamp_swa_average_(handle_array([t.h for t in avg]), handle_array([t.h for t in cur]), len(avg), 3)
    assert re.search(r"\b%d\b" % index, str(e.value)), str(e.value)
    lib.lamp_device_synchronize()
    assert [_bits(t) for t in untouched] == before, "a rejected call has written"
    return str(e.value)


def test_swa_average_rejections_name_the_index_and_write_nothing(gpu):
    f = lambda n, salt, dt=torch.float32: to_sten(_values(n, salt, dt))
    good = [f(1030, 1), f(6, 2)]
    # an i64 tensor at index 2
    ints = to_sten(torch.arange(6, dtype=torch.int64))
    _rejected(good + [ints], [f(1030, 3), f(6, 4), to_sten(torch.arange(6, dtype=torch.int64))], 2, good + [ints])
    # a dtype mismatch at index 1
    _rejected(good, [f(1030, 3), f(6, 4, torch.bfloat16)], 1, good)
    # a count mismatch at index 1 (5 against 6 elements)
    _rejected(good, [f(1030, 3), f(5, 4)], 1, good)
    # a non-contiguous tensor at index 2
    strided = to_sten(closed_form((4, 3), 9, 1.0)).transpose(0, 1)
    assert not strided.is_contiguous()
    third = to_sten(closed_form((3, 4), 8, 1.0))
    _rejected(good + [third], [f(1030, 3), f(6, 4), strided], 2, good + [third])
    # and the well-formed call passes
    cur = [f(1030, 3), f(6, 4)]
    lib.lamp_swa_average_(handle_array([t.h for t in good]), handle_array([t.h for t in cur]), 2, 3)


# ---- state_copy, the snapshot, Module.load -----------------------------------------------------------------------------------------------------
def _any_values(n, salt, dt):
    if dt in (torch.int64, torch.uint8):
        v = (torch.arange(n, dtype=torch.int64) + salt) * 7919
        return (v * 1000003 - 5) if dt == torch.int64 else (v % 251).to(torch.uint8)
    return _values(n, salt, dt)


COPY_DTYPES = [torch.float32, torch.bfloat16, torch.int64, torch.uint8]


def _copy_sources():
    src, salt = [], 0
    for dt in COPY_DTYPES:
        for n in SIZES:
            salt += 1
            src.append(to_sten(_any_values(n, salt, dt)))
        src.append(_off_by_one(_any_values(1030, 90 + salt, dt)))
    src += [to_sten(_any_values(5, 400 + k, torch.float32)) for k in range(41)]
    return src


def test_snapshot_is_bit_equal_and_owns_its_storage(gpu):
    src = _copy_sources()
    want = [_bits(t) for t in src]
    snap = nn.stateSnapshot(src)
    assert [_bits(t) for t in snap] == want and [t.shape for t in snap] == [t.shape for t in src] and [t.dtype for t in snap] == [t.dtype for t in src]
    assert all(s.storage_id != t.storage_id for s, t in zip(snap, src) if t.numel)
    for t in src:
        t.fill_(1.0)                                          # overwrite the sources: the snapshot does not follow
    assert [_bits(t) for t in snap] == want
    # the restore, into destinations of which some are off a 16-byte boundary
    lib.lamp_state_copy_(handle_array([t.h for t in src]), handle_array([t.h for t in snap]), len(src))
    assert [_bits(t) for t in src] == want
    # unfused: the same bytes out of one clone per tensor
    prev = nn.stateKernelsFused(False)
    try:
        assert [_bits(t) for t in nn.stateSnapshot(src)] == want
    finally:
        nn.stateKernelsFused(prev)


def test_state_copy_rejections(gpu):
    a, b = to_sten(_values(6, 1, torch.float32)), to_sten(_values(6, 2, torch.float32))
    before = _bits(a)
    for bad in (to_sten(_values(6, 3, torch.bfloat16)), to_sten(_values(5, 3, torch.float32))):
        with pytest.raises(LampError) as e:
            lib.lamp_state_copy_(handle_array([a.h, a.h]), handle_array([b.h, bad.h]), 2)
        assert re.search(r"\b1\b", str(e.value)), str(e.value)
    assert _bits(a) == before


def _mlp():
    lib.lamp_manual_seed(5)
    return nn.Sequential(nn.MLP(20, 4, [16], S.F32, 0), nn.Fun("logsoftmax", 1))


def test_module_load(gpu):
    net = _mlp()
    original = nn.stateSnapshot([v.value for v in net.state])
    want = [_bits(t) for t in original]
    other = [to_sten(_values(int(np.prod(t.shape)), 30 + i, torch.float32).reshape(t.shape)) for i, t in enumerate(original)]
    for fused in (True, False):
        prev = nn.stateKernelsFused(fused)
        try:
            net.load(other)
            assert [_bits(v.value) for v in net.state] == [_bits(t) for t in other]
            net.load(original)                                # a snapshot: device tensors of the state's dtypes
            assert [_bits(v.value) for v in net.state] == want
        finally:
            nn.stateKernelsFused(prev)
    # host tensors, and tensors of another dtype, take the per-tensor copyFrom as before
    net.load([t.cpu() for t in other])
    assert [_bits(v.value) for v in net.state] == [_bits(t) for t in other]
    net.load([t.castToDouble() for t in original])
    assert [_bits(v.value) for v in net.state] == want
    counts = _timer_counts(lambda: net.load([t.castToDouble() for t in original]))
    assert "state_copy" not in counts, counts


# ---- the launch budget ---------------------------------------------------------------------------------------------------------------------------
def _timer_counts(fn):
    lib.lamp_device_synchronize()
    buf = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_report(buf, len(buf))            # clears the log
    lib.lamp_kernel_timer_enable(1)
    try:
        fn()
        lib.lamp_device_synchronize()
    finally:
        lib.lamp_kernel_timer_enable(0)
    lib.lamp_kernel_timer_report(buf, len(buf))
    counts = {}
    for line in buf.value.decode().splitlines():
        f = line.split()
        counts[f[0]] = int(f[1])
    return counts


NEW_KERNELS = {"state_copy", "swa_average"}


@pytest.mark.parametrize("dtype", [S.F32, S.BF16])
def test_launch_budget_on_the_resnet_state(gpu, dtype):
    net = nn.resnet(100, 0.0, dtype, 0)
    state = [v.value for v in net.state]
    assert len(state) == 74
    per_class = {}
    for t in state:
        per_class[t.dtype] = per_class.get(t.dtype, 0) + 1
    launches = sum(-(-c // MT_MAX) for c in per_class.values())          # one per MT_MAX tensors per dtype class
    assert all(-(-c // MT_MAX) <= 2 for c in per_class.values()) and launches <= 2 * len(per_class)
    out = {}
    snap = _timer_counts(lambda: out.update(snapshot=nn.stateSnapshot(state)))
    averaged = out["snapshot"]
    avg = _timer_counts(lambda: nn.swaAverage(averaged, state, 1))
    load = _timer_counts(lambda: net.load(averaged))
    print(f"dtype {dtype}: classes {per_class}; fused: snapshot {snap}, average {avg}, load {load}")
    # nothing but the new kernels: no element-wise multiply / add / divide, no per-tensor copy kernel
    assert set(snap) == {"state_copy"} and 1 <= snap["state_copy"] <= launches, snap
    assert set(avg) == {"swa_average"} and 1 <= avg["swa_average"] <= launches, avg
    assert set(load) == {"state_copy"} and 1 <= load["state_copy"] <= launches, load
    prev = nn.stateKernelsFused(False)
    try:
        snap = _timer_counts(lambda: out.update(snapshot=nn.stateSnapshot(state)))
        chain = out["snapshot"]
        avg = _timer_counts(lambda: out.update(avg=nn.swaAverage(chain, state, 1)))
        load = _timer_counts(lambda: net.load(out["avg"]))
    finally:
        nn.stateKernelsFused(prev)
    print(f"dtype {dtype}: chain: snapshot {snap}, average {avg}, load {load}")
    for counts in (snap, avg, load):
        assert not NEW_KERNELS & set(counts), counts
    assert avg.get("elementwise", 0) == 3 * len(state), avg    # tensor * n, add, tensor / (n + 1) per state tensor
