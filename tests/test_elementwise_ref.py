"""tests/elementwise_ref.py on a box without a GPU: the tables are what they claim, the written-out float64 references agree with ATen's
float64, the registry names every entry point of kernels/elementwise.hip, and the whole registry and every converting copy run on HOST
tensors - the library's CPU device evaluates the functors (launch_ew's host loop) and the copy template (host_copy_t) that the kernels
instantiate, so a wrong functor or a wrong conversion shows here.  The launch forms themselves: tests/test_elementwise_kernels_gpu.py."""
import pytest
import torch

from lamp_amd._capi import lib
from tests import elementwise_ref as E
from tests.elementwise_ref import BF16, BOOL, F16, F32, F64, I32, I64, U8
from tests.util import assert_close

lib.load()


def test_sizes():
    assert [E.n_for(dt) for dt in (F64, I64, F32, I32, BF16, F16, U8, BOOL)] == [1029, 1029, 2055, 2055, 4107, 4107, 8211, 8211]
    for dt in E.ALL_BOOL:
        w, n = E.W(dt), E.n_for(dt)
        # two blocks of 256 packets, a packet in a third one and three more elements: a scalar tail for every width (2 divides none)
        assert n == (2 * 256 + 1) * w + 3 and n // w > 2 * 256 and n % w != 0


@pytest.mark.parametrize("dt", E.FLOATS, ids=E.dtid)
def test_float_table(dt):
    n, w = E.n_for(dt), E.W(dt)
    sp = E.specials(dt)
    for salt in (0, 1, 12):
        v = E.float_table(-6.0, 6.0, dt, salt)
        assert v.dtype == dt and list(v.shape) == [n]
        rot = sp[salt % len(sp):] + sp[:salt % len(sp)]
        want = torch.tensor(rot, dtype=F64).to(dt)
        # the whole list in the first packets and in the second block, ending mid-packet; its start in the third block's one packet
        for k in (0, 64, 256 * w):
            assert k % 64 == 0 and E.equal_bits(v[k:k + len(sp)], want), k
        assert E.equal_bits(v[2 * 256 * w:2 * 256 * w + w], want[:w])
        assert len(sp) % w != 0
        assert E.equal_bits(v[n - 3:], torch.tensor(E.TAIL, dtype=F64).to(dt))          # the scalar tail: nan, -0.0, inf
        mask = E.special_mask(n, len(sp))
        sweep = v[~mask].double()
        assert bool(torch.isfinite(sweep).all()) and sweep.min() >= -6.0 and sweep.max() <= 6.0 and sweep.min() < -5.9 and sweep.max() > 5.9
        tiny = torch.finfo(dt).tiny
        assert bool(((sweep == 0) | (sweep.abs() >= tiny)).all())                          # zero or normal: no subnormal of the dtype
    assert {88.0, -104.0} <= set(E.specials(F32)) and {11.0, -17.0} <= set(E.specials(F16)) and 88.0 not in E.specials(F16)
    for x in (0.5, 1.5, 2.5, 3.5, 3.0, -3.0, 20.0, 20.5):
        assert x in sp


@pytest.mark.parametrize("dt", E.INTS + (BOOL,), ids=E.dtid)
def test_int_tables(dt):
    n = E.n_for(dt)
    v = E.int_table(dt)
    assert v.dtype == dt and list(v.shape) == [n]
    sp = E.INT_SPECIALS[dt]
    for k in (0, 64, 256 * E.W(dt)):
        assert [int(x) for x in v[k:k + len(sp)].tolist()] == sp                           # exact, also beyond 2^53
    m = min(len(sp), E.W(dt))
    assert [int(x) for x in v[2 * 256 * E.W(dt):][:m].tolist()] == sp[:m]                # the third block's one packet
    assert [int(x) for x in v[n - 3:].tolist()] == (sp * 3)[-3:]                           # the scalar tail
    if dt == I64:
        assert {2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 62, -(2 ** 63 - 1)} <= set(v.tolist()) and -(2 ** 63) not in v.tolist()
    if dt == I32:
        assert {2 ** 31 - 1, -(2 ** 31 - 1)} <= set(v.tolist())
    if dt == U8:
        assert 255 in v.tolist()
    d = E.divisor_table(dt)
    assert d.dtype == dt and bool((d != 0).all())
    if dt in (I64, I32):
        assert bool((d < 0).any()) and bool((d > 0).any())


def test_registry_names_every_entry_point():
    """every lamp_* function kernels/elementwise.hip defines (the element-wise section of include/lamp_hip.h) is in the registry, and
    the registry names nothing else"""
    declared = E.header_entry_points()
    assert len(declared) > 100
    assert sorted(E.REGISTRY) == declared, (sorted(set(declared) - set(E.REGISTRY)), sorted(set(E.REGISTRY) - set(declared)))
    for e in E.REGISTRY.values():
        assert hasattr(lib, "lamp_" + e.name)
        assert e.device_only or e.ref is not None or e.exact is not None, e.name
        assert e.base is None or E.REGISTRY[e.base].kind == "new", e.name


def test_every_copy_pair_is_listed():
    assert len(E.CAST_PAIRS) == 64 and len(set(E.CAST_PAIRS)) == 64


@pytest.mark.parametrize("e", [e for e in E.REGISTRY.values() if e.aten is not None and e.base is None], ids=lambda e: e.name)
def test_written_out_reference_agrees_with_aten(e):
    """the formulas written out here (gelu, hardswish, softplus, relu and leaky relu and the backward forms) against ATen's CPU float64
    on the table: same non-finite pattern, 1e-12 elsewhere"""
    xs = E.operands(e, F64)
    for scalars in e.cases(F64):
        assert_close(e.ref(*xs, *scalars), e.aten(*xs, *scalars), 1e-12, f"{e.name}{scalars}")


@pytest.mark.parametrize("p", E.grid(), ids=E.grid_id)
def test_host_matrix(p):
    e, dt = p
    for scalars in e.cases(dt):
        E.run_and_check(e, dt, scalars, E.on_host, f"{e.name}{scalars} {E.dtid(dt)} host")


@pytest.mark.parametrize("p", E.CAST_PAIRS, ids=E.cast_id)
def test_host_casts(p):
    E.check_cast(p[0], p[1], -1)
