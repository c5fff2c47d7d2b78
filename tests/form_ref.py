"""What the kernel-form tests of the reductions, the pooling and the index kernels share (tests/test_reduce_kernels_gpu.py,
test_pool_kernels_gpu.py, test_index_kernels_gpu.py): which form a launch took, read from the kernel timers; a mirror of the reduction's
chooser; exact-integer data; the top-k reference.  Everything that needs no GPU is verified by tests/test_form_ref.py."""
import contextlib
import ctypes as C

import torch

from lamp_amd._capi import lib
from tests.util import to_sten

F64, F32, BF16, I64 = torch.float64, torch.float32, torch.bfloat16, torch.int64
ITEM = {F64: 8, F32: 4, BF16: 2, I64: 8}


def dtid(dt):
    return str(dt).replace("torch.", "")


def W(dt):
    """elements per 16-byte packet"""
    return 16 // ITEM[dt]


class Launches(dict):
    """tag -> (launches, declared work per launch) of the tagged launches inside a `with launched()` block.  The report prints the
    work with seven significant digits (%.6e): a count read back from it is exact below 10^7."""

    def count(self, tag):
        return self.get(tag, (0, 0.0))[0]

    def work(self, tag):
        return self[tag][1]


@contextlib.contextmanager
def launched():
    buf = C.create_string_buffer(1 << 16)
    lib.lamp_kernel_timer_filter(None)
    lib.lamp_kernel_timer_report(buf, len(buf))            # drops what earlier tests left in the log
    got = Launches()
    lib.lamp_kernel_timer_enable(1)
    try:
        yield got
    finally:
        lib.lamp_kernel_timer_enable(0)
        lib.lamp_kernel_timer_report(buf, len(buf))
    for line in buf.value.decode().splitlines():
        f = line.split()
        got[f[0]] = (int(f[1]), float(f[3]))


def num_cus():
    n = C.c_int(0)
    lib.lamp_device_num_cus(C.byref(n))
    return n.value


def misaligned(t):
    """t's values as a CONTIGUOUS device view whose data pointer is one element past a 16-byte boundary (tests/test_row_kernels_gpu.py):
    every packet form has to decline it"""
    base = to_sten(torch.cat([t.new_zeros(1), t.reshape(-1)]))
    v = base.narrow(0, 1, t.numel()).view(*t.shape)
    assert base.data_ptr % 16 == 0 and v.data_ptr % 16 == ITEM[t.dtype] and v.is_contiguous()
    return v


def aligned(t):
    a = to_sten(t)
    assert a.data_ptr % 16 == 0
    return a


def small_ints(shape, salt=0, dtype=F64, lim=3):
    """closed-form integers in [-lim, lim]: every partial sum of up to 2^24 / lim^2 of them (or of their squares) is an integer below 2^24
    and therefore exact in f32 and f64 whatever the order of the additions; each of them is exact in bf16"""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64) + salt
    v = ((i * 7919) % 1009) % (2 * lim + 1) - lim
    return v.reshape(shape).to(dtype)


def equal_bits(got, ref):
    """bit-exact up to the payload of a NaN: same NaN positions, same values elsewhere, same sign of every zero"""
    got, ref = got.double(), ref.double()
    if list(got.shape) != list(ref.shape):
        return False
    nan = torch.isnan(ref)
    if not torch.equal(torch.isnan(got), nan):
        return False
    g, r = got[~nan], ref[~nan]
    return torch.equal(g, r) and torch.equal(torch.signbit(g), torch.signbit(r))


# ---- the reduction's chooser (reduce_typed in kernels/reduce.hip) ------------------------------------------------------------------------
def reduce_plan(shape, dims, item, ncu=256, on_packet=True):
    """(launch tag, nsplit, finalize tag) of a reduction of a contiguous tensor of `shape` over `dims` (empty: all) for elements of
    `item` bytes on `ncu` compute units (target_blocks = 4 ncu); on_packet: the data pointer is 16-byte aligned"""
    nd = len(shape)
    red = [not dims] * nd
    for d in dims:
        red[d % nd] = True
    groups = []
    for i in range(nd):
        if shape[i] == 1:
            continue
        if groups and groups[-1][0] == red[i]:
            groups[-1][1] *= shape[i]
        else:
            groups.append([red[i], shape[i]])
    g = [1, 1, 1, 1]                                        # K0, R1, K1, R2
    i = 0
    for slot, want in enumerate((False, True, False, True)):
        if i < len(groups) and groups[i][0] == want:
            g[slot] = groups[i][1]
            i += 1
    if i != len(groups):
        return "reduce_generic", 1, None
    K0, R1, K1, R2 = g
    if K1 == 1 and R2 == 1:
        K0, R1, K1, R2 = 1, 1, K0, R1
    nout = K0 * K1
    w = 16 // item
    target = ncu * 4
    column = R2 == 1 and K1 >= 64
    nsplit = 1
    if column:
        blocks = (nout + 255) // 256
        if K1 % w == 0 and R1 >= 64:
            blocks = ((K1 // w + 31) // 32) * K0
        if blocks < target and R1 >= 256:
            nsplit = min(target // blocks, R1 // 64, 256)
    else:
        total = R1 * R2
        if nout < target and total >= 8192:
            nsplit = min(target // nout, total // 2048, 1024)
    nsplit = max(nsplit, 1)
    vec = column and K1 % w == 0 and on_packet and K0 <= 65535 and R1 >= 64
    tag = "reduce_column_vec" if vec else ("reduce_column" if column else "reduce_block")
    return tag, nsplit, ("reduce_finalize_wide" if nsplit >= 16 and nout < 65536 else "reduce_finalize")


def split_rows(n, nsplit):
    """first and last element of every non-empty chunk of n elements split nsplit ways the way the kernels do, and the number of chunks
    that start past the end"""
    chunk = (n + nsplit - 1) // nsplit
    edges = [(s * chunk, min(s * chunk + chunk, n) - 1) for s in range(nsplit) if s * chunk < n]
    return edges, nsplit - len(edges)


# ---- top-k ---------------------------------------------------------------------------------------------------------------------------
def topk_ref(v, k, dim, largest):
    """the first k of a stable sort along dim: lexicographic (value, index), ascending values or, for `largest`, descending ones.  NaN is
    the greatest value and equal to every other NaN (ATen); -0.0 == 0.0.  Returns (values in v's dtype, int64 indices)."""
    vals, idx = torch.sort(v.double(), dim=dim, descending=bool(largest), stable=True)
    idx = idx.narrow(dim, 0, k).contiguous()
    return torch.gather(v, dim, idx), idx
