"""Tables, float64 references and one registry for every entry point of kernels/elementwise.hip and for the converting copies of
core/tensor.hip.  Nothing here needs a GPU: tests/test_elementwise_ref.py verifies the tables and the references and runs the registry on
host tensors (the library's CPU device runs the functors and copy templates the kernels instantiate); tests/test_elementwise_kernels_gpu.py
runs it through the three launch forms on the device.

A toleranced functor is compared (util.assert_close) with a plain float64 formula on the inputs AFTER rounding to the dtype under test,
the result cast to that dtype: overflow to inf and underflow are then the dtype's.  An exact functor is compared bit for bit
(form_ref.equal_bits: sign of zero included, NaN payload ignored) with torch in the same dtype on the CPU."""
import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import torch

from lamp_amd import sten as S
from lamp_amd._capi import lib
from tests.form_ref import equal_bits
from tests.util import FWD_TOL, TORCH2LAMP, assert_close, to_sten, to_torch

F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
I64, I32, U8, BOOL = torch.int64, torch.int32, torch.uint8, torch.bool
FLOATS = (F64, F32, BF16, F16)
INTS = (I64, I32, U8)
ALL = FLOATS + INTS
ALL_BOOL = ALL + (BOOL,)
ITEM = {F64: 8, F32: 4, BF16: 2, F16: 2, I64: 8, I32: 4, U8: 1, BOOL: 1}
# f16 is not in FWD_TOL: one rounding is 2^-11 relative, doubled
TOL = dict(FWD_TOL)
TOL[F16] = 2.0 ** -10


def dtid(dt):
    return str(dt).replace("torch.", "")


def W(dt):
    """elements per 16-byte packet"""
    return 16 // ITEM[dt]


def n_for(dt):
    """two full blocks of 256 packets, one packet in a third block and a scalar tail of three: the smallest size at which a wrong packet
    index, block offset or tail start shows"""
    return 2 * 256 * W(dt) + W(dt) + 3


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
SPECIALS = [NAN, INF, -INF, 0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1.5, 2.5, -2.5, 3.0, -3.0, 3.5, -3.5, 20.0, 20.5, -20.5, 88.0, -104.0]
TAIL = [NAN, -0.0, INF]
EVERY = 64


def specials(dt):
    """round's ties, hardswish's +-3, softplus' threshold, exp overflow and underflow in f32 (88, -104) or f16 (11, -17)"""
    return [{88.0: 11.0, -104.0: -17.0}.get(v, v) for v in SPECIALS] if dt == F16 else list(SPECIALS)


def special_mask(n, nsp):
    """True where a table of n elements holds a special: the first nsp of every 64 elements, and the tail of three"""
    i = torch.arange(n)
    return ((i % EVERY) < nsp) | (i >= n - 3)


def float_table(lo, hi, dt, salt=0, n=None):
    """[n_for(dt)] values in dt: a closed-form sweep of [lo, hi] (util.closed_form's), the special list written over it at the start of
    every 64th element (the first packet, later blocks, every lane of a packet; rotated by `salt` so that two operands pair different
    specials), and nan, -0.0, inf as the scalar tail"""
    n = n_for(dt) if n is None else n
    i = torch.arange(n, dtype=torch.int64) + salt
    v = lo + (hi - lo) * ((i * 7919) % 1009).to(F64) / 1008.0
    sp = specials(dt)
    sp = sp[salt % len(sp):] + sp[:salt % len(sp)]
    for k in range(0, n, EVERY):
        m = min(len(sp), n - k)
        v[k:k + m] = torch.tensor(sp[:m], dtype=F64)
    v[n - 3:] = torch.tensor(TAIL, dtype=F64)
    return v.to(dt)


INT_SPECIALS = {I64: [0, 1, -1, 7, -7, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 62, -(2 ** 63 - 1)],      # not the minimum: -a on it is undefined
                I32: [0, 1, -1, 7, -7, 2 ** 31 - 1, -(2 ** 31 - 1)],
                U8: [0, 1, 7, 255],
                BOOL: [0, 1]}


def int_table(dt, salt=0, n=None):
    """[n_for(dt)] integers in dt: a sweep of [-504, 504] ([0, 255] for uint8, {0, 1} for bool), the dtype's special values at the start
    of every 64th element (rotated by salt) and as the scalar tail"""
    n = n_for(dt) if n is None else n
    i = torch.arange(n, dtype=torch.int64) + salt
    v = (i * 7919) % 1009 - 504
    if dt == U8:
        v = (v + 504) % 256
    elif dt == BOOL:
        v = (v + 504) % 2
    sp = INT_SPECIALS[dt]
    sp = sp[salt % len(sp):] + sp[:salt % len(sp)]
    for k in range(0, n, EVERY):
        m = min(len(sp), n - k)
        v[k:k + m] = torch.tensor(sp[:m], dtype=I64)
    v[n - 3:] = torch.tensor((sp + sp + sp)[-3:], dtype=I64)
    return v.to(dt)


def divisor_table(dt, salt=0, n=None):
    """nonzero divisors of both signs (positive ones for uint8): [-9, 9] without 0, and +-7 and 10"""
    n = n_for(dt) if n is None else n
    i = torch.arange(n, dtype=torch.int64) + salt
    v = ((i * 7919) % 1009) % 19 - 9
    v[v == 0] = 10
    if dt in (U8, BOOL):
        v = v.abs()
    if dt == BOOL:
        v = v.clamp(max=1)
    return v.to(dt)


def table(spec, dt, salt, n=None):
    """one operand: spec is (lo, hi) for the float sweep; integer dtypes take int_table, or divisor_table for spec "div" """
    if dt in FLOATS:
        lo, hi = (-6.0, 6.0) if spec == "div" else spec
        return float_table(lo, hi, dt, salt, n)
    return divisor_table(dt, salt, n) if spec == "div" else int_table(dt, salt, n)


# ---- registry -------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Entry:
    name: str                                   # lamp_<name>
    arity: int = 1                              # tensor operands
    ref: Optional[Callable] = None              # float64 formula: ref(*operands in float64, *scalars) -> float64 (bool for predicates)
    exact: Optional[Callable] = None            # torch in the dtype under test: exact(*operands, *scalars); compared bit for bit
    aten: Optional[Callable] = None             # ATen's float64 function the written-out `ref` has to agree with
    dtypes: Sequence = FLOATS
    cases: Callable = lambda dt: [()]           # dt -> list of extra-scalar tuples
    ranges: Sequence = ((-6.0, 6.0),) * 3       # float sweep per operand, or "div"
    tolmul: Callable = lambda scalars: 1
    kind: str = "new"                           # new: fn(&out, *ops, *scalars); inplace: fn(*ops, *scalars) writes ops[0]; out: fn(out, *ops, *scalars)
    base: Optional[str] = None                  # the out-of-place form an in-place or _out twin has to equal bit for bit
    bool_out: bool = False
    device_only: bool = False                   # where, masked_fill, add_scaled_mixed_: kernels of their own, tests of their own


REGISTRY = {}


def _reg(name, **kw):
    assert name not in REGISTRY, name
    REGISTRY[name] = Entry(name, **kw)


def _twin(name, base, kind):
    b = REGISTRY[base]
    _reg(name, arity=b.arity, ref=b.ref, exact=b.exact, aten=b.aten, dtypes=b.dtypes, cases=b.cases, ranges=b.ranges, tolmul=b.tolmul,
         kind=kind, base=base, bool_out=b.bool_out)


X4 = lambda scalars: 4          # exp, expm1, tan, pow: test_unary_functions' rule
SQRT1_2, INV_SQRT_2PI = 0.70710678118654752440, 0.39894228040143267794


def _gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x * SQRT1_2))


def _gelu_bwd(g, x):
    return g * (0.5 * (1.0 + torch.erf(x * SQRT1_2)) + x * (INV_SQRT_2PI * torch.exp(x * x * -0.5)))


def _hardswish(x):
    return x * (x + 3.0).clamp(0.0, 6.0) / 6.0


def _hardswish_bwd(g, x):
    """ATen's pieces: 0 for x <= -3 (also at -3, where the middle piece gives -g / 2), g for x >= 3 (also at 3, where it gives 3 g / 2),
    and the middle piece - NaN - for a NaN x"""
    return torch.where(x <= -3.0, torch.zeros_like(g), torch.where(x >= 3.0, g, g * (x / 3.0 + 0.5)))


def _softplus(x, beta, thr):
    return torch.where(x * beta > thr, x, torch.log1p(torch.exp(x * beta)) / beta)


def _softplus_bwd(g, x, beta, thr):
    z = torch.exp(x * beta)
    return torch.where(x * beta > thr, g, g * z / (z + 1.0))


def _slope(x, slope):
    return torch.where(x < 0, torch.full_like(x, slope), torch.ones_like(x))


def _leaky(x, slope):
    return torch.where(x > 0, x, x * slope)


def _i_relu(a):
    return torch.where(a < 0, torch.zeros_like(a), a)


def _i_abs(a):
    return torch.where(a < 0, -a, a)


def _i_sign(a):
    return (a > 0).to(a.dtype) - (a < 0).to(a.dtype)


def _same(f_float, f_int=None):
    """exact reference in the dtype under test: torch's function for floating tensors, a same-dtype formula for integer ones where given"""
    def run(*args):
        return (f_int or f_float)(*args) if args[0].dtype in INTS + (BOOL,) else f_float(*args)
    return run


def _alpha(f):
    """a (+-) alpha * b in the tensor's dtype: the scalar an integer (wrapping, as the kernel's) for integer tensors"""
    def run(a, b, alpha):
        return f(a, b * (int(alpha) if a.dtype in INTS else alpha))
    return run


def _wrap(f):
    """tensor (op) integral scalar on an integer tensor: in int64, then wrapped into the tensor's dtype as the kernel's store does"""
    def run(a, *scalars):
        return f(a.to(I64), *[int(v) for v in scalars]).to(a.dtype)
    return run


def _cases_alpha(dt):
    return [(1.0,), (3.0,)] if dt in INTS else [(1.0,), (-0.5,)]


def _cases_scalar(dt):
    return [(3.0,), (-2.0,)] if dt in INTS else [(2.5,), (-0.75,)]


# arithmetic: toleranced in the floating dtypes, exact (wrapping as torch does) in the integer ones
def _arith(name, arity, ref, exact_int, cases=lambda dt: [()], ranges=((-6.0, 6.0),) * 3, dtypes=ALL):
    _reg(name, arity=arity, ref=ref, exact=exact_int, cases=cases, ranges=ranges, dtypes=dtypes)


_arith("add", 2, lambda a, b, al: a + al * b, _alpha(torch.add), _cases_alpha)
_arith("sub", 2, lambda a, b, al: a - al * b, _alpha(torch.sub), _cases_alpha)
_arith("mul", 2, lambda a, b: a * b, torch.mul)
_reg("div", arity=2, ref=lambda a, b: a / b)                                              # integer div truncates by design: out of scope
_arith("add_scalar", 1, lambda a, s, al: a + s * al, _wrap(lambda a, s, al: a + s * al), lambda dt: [(3.0, 1.0), (2.0, -2.0)] if dt in INTS else [(2.5, 1.0), (1.5, -0.5)])
_arith("sub_scalar", 1, lambda a, s, al: a - s * al, _wrap(lambda a, s, al: a - s * al), lambda dt: [(3.0, 1.0), (2.0, -2.0)] if dt in INTS else [(2.5, 1.0), (1.5, -0.5)])
_arith("mul_scalar", 1, lambda a, s: a * s, _wrap(lambda a, s: a * s), _cases_scalar)
_reg("div_scalar", ref=lambda a, s: a / s, cases=lambda dt: [(2.5,), (-0.75,)])
_arith("square", 1, lambda a: a * a, lambda a: a * a)
_arith("remainder", 2, torch.remainder, torch.remainder, ranges=((-6.0, 6.0), "div"))
_arith("remainder_scalar", 1, torch.remainder, _wrap(torch.remainder),
       lambda dt: [(10.0,)] if dt == U8 else ([(10.0,), (-7.0,)] if dt in INTS else [(2.5,), (-1.5,)]))
_arith("addcmul_out", 3, lambda a, b, c, v: a + v * b * c, lambda a, b, c, v: a + int(v) * b * c, lambda dt: [(2.0,)] if dt in INTS else [(0.5,)])
REGISTRY["addcmul_out"].kind = "out"
_reg("addcdiv_out", arity=3, ref=lambda a, b, c, v: a + v * b / c, cases=lambda dt: [(0.5,)], kind="out")
_reg("mul_add", arity=3, ref=lambda a, b, c, dt=None: (a * b).to(dt).double() + c)       # the product rounded to the tensor type first
_reg("pow_tensor", arity=2, ref=torch.pow, tolmul=X4, ranges=((-3.0, 3.0), (-3.0, 3.0)))
# 2, 3, 0.5, 1, -1, -2, -0.5: FPowS's special branches; 0 and 1.7: the general one (4 x)
_reg("pow_scalar", ref=lambda a, e: torch.pow(a, e), cases=lambda dt: [(e,) for e in (2.0, 3.0, 0.5, 1.0, -1.0, -2.0, -0.5, 0.0, 1.7)],
     tolmul=lambda s: 4 if s[0] in (0.0, 1.7) else 1, ranges=((-3.0, 3.0),))

# exact: value-preserving or rounding to an integer
_reg("maximum", arity=2, exact=torch.maximum, dtypes=ALL)
_reg("minimum", arity=2, exact=torch.minimum, dtypes=ALL)
_reg("neg", exact=torch.neg, dtypes=ALL)
_reg("abs", exact=_same(torch.abs, _i_abs), dtypes=ALL)
_reg("sign", exact=_same(torch.sign, _i_sign), dtypes=ALL)
_reg("relu", exact=_same(torch.relu, _i_relu), dtypes=ALL)
_reg("ceil", exact=torch.ceil)
_reg("floor", exact=torch.floor)
_reg("round", exact=torch.round)
_reg("nan_to_num", exact=lambda a, nan: torch.nan_to_num(a, nan=nan), cases=lambda dt: [(0.0,), (1.5,)])

# activations and their backward forms
_reg("leaky_relu", ref=_leaky, aten=torch.nn.functional.leaky_relu, cases=lambda dt: [(0.1,)])
_reg("gelu", ref=_gelu, aten=torch.nn.functional.gelu)
_reg("gelu_backward", arity=2, ref=_gelu_bwd, aten=torch.ops.aten.gelu_backward)
_reg("sigmoid", ref=torch.sigmoid)
_reg("sigmoid_backward", arity=2, ref=lambda g, y: g * (1.0 - y) * y, aten=torch.ops.aten.sigmoid_backward, ranges=((-6.0, 6.0), (0.0, 1.0)))
_reg("tanh", ref=torch.tanh)
_reg("tanh_backward", arity=2, ref=lambda g, y: g * (1.0 - y * y), aten=torch.ops.aten.tanh_backward, ranges=((-6.0, 6.0), (-1.0, 1.0)))
_reg("hardswish", ref=_hardswish, aten=torch.nn.functional.hardswish)
_reg("hardswish_backward", arity=2, ref=_hardswish_bwd, aten=torch.ops.aten.hardswish_backward)
_reg("softplus", ref=_softplus, aten=torch.nn.functional.softplus, cases=lambda dt: [(1.0, 20.0), (2.0, 10.0)], ranges=((-30.0, 30.0),))
_reg("softplus_backward", arity=2, ref=_softplus_bwd, aten=torch.ops.aten.softplus_backward, cases=lambda dt: [(1.0, 20.0), (2.0, 10.0)],
     ranges=((-6.0, 6.0), (-30.0, 30.0)))
_reg("relu_backward", arity=2, ref=lambda p, x, slope: p * _slope(x, slope), cases=lambda dt: [(0.0,), (0.1,)])
_reg("relu_backward_accumulate_", arity=3, ref=lambda o, p, x, slope: o + p * _slope(x, slope), cases=lambda dt: [(0.0,), (0.1,)], kind="inplace")

# transcendental
_reg("exp", ref=torch.exp, tolmul=X4)
_reg("expm1", ref=torch.expm1, tolmul=X4)
_reg("log", ref=torch.log, ranges=((-1.0, 6.0),))
_reg("log1p", ref=torch.log1p, ranges=((-2.0, 6.0),))
_reg("log10", ref=torch.log10, ranges=((-1.0, 6.0),))
_reg("sqrt", ref=torch.sqrt, ranges=((-1.0, 6.0),))
_reg("reciprocal", ref=torch.reciprocal)
_reg("sin", ref=torch.sin)
_reg("cos", ref=torch.cos)
_reg("tan", ref=torch.tan, tolmul=X4)
_reg("atan", ref=torch.atan)
_reg("acos", ref=torch.acos, ranges=((-1.25, 1.25),))
_reg("asin", ref=torch.asin, ranges=((-1.25, 1.25),))
_reg("atan2", arity=2, ref=torch.atan2)

# predicates -> bool, from every dtype (bool and uint8 inputs: 16 elements per packet)
for _n, _f in (("lt", torch.lt), ("le", torch.le), ("gt", torch.gt), ("ge", torch.ge), ("eq", torch.eq), ("ne", torch.ne)):
    _reg(_n, arity=2, exact=_f, dtypes=ALL_BOOL, bool_out=True)
    # integer tensors: fractional scalars must not truncate; integral ones hit the table's own values (tensor <op> scalar in torch)
    _reg(_n + "_scalar", exact=_f, dtypes=ALL_BOOL, bool_out=True,
         cases=lambda dt: [(0.5,), (-3.0,)] if dt in FLOATS else [(0.5,), (-0.5,), (2.5,), (1.0,), (-3.0,)])
for _n, _f in (("logical_and", torch.logical_and), ("logical_or", torch.logical_or), ("logical_xor", torch.logical_xor)):
    _reg(_n, arity=2, exact=_f, dtypes=ALL_BOOL, bool_out=True)
_reg("logical_not", exact=torch.logical_not, dtypes=ALL_BOOL, bool_out=True)
_reg("isnan", exact=torch.isnan, dtypes=ALL_BOOL, bool_out=True)
_reg("isfinite", exact=torch.isfinite, dtypes=ALL_BOOL, bool_out=True)

# in-place and _out twins
for _n in ("add", "sub", "mul", "div"):
    _twin(_n + "_out", _n, "out")
    _twin(_n + "_", _n, "inplace")
for _n in ("add_scalar", "mul_scalar", "relu", "exp", "sqrt", "reciprocal", "abs", "acos", "asin", "atan", "ceil", "floor", "cos", "sin", "tan",
           "tanh", "sigmoid", "log", "log1p", "square", "leaky_relu"):
    _twin(_n + "_", _n, "inplace")

# kernels of their own (device only; tests/test_elementwise_kernels_gpu.py)
_reg("where", arity=3, dtypes=ALL_BOOL, device_only=True)
_reg("masked_fill", arity=2, dtypes=ALL_BOOL, device_only=True)
_reg("add_scaled_mixed_", arity=2, dtypes=FLOATS, device_only=True, kind="inplace")


def header_entry_points():
    """the lamp_* names include/lamp_hip.h declares in its element-wise section: the entry points kernels/elementwise.hip defines"""
    import os
    import re
    from lamp_amd._capi import ROOT
    src = open(os.path.join(ROOT, "include", "lamp_hip.h")).read()
    a = src.index(" * element-wise, broadcasting")
    b = src.index(" * reductions", a)
    return sorted(m.group(1) for m in re.finditer(r"^int lamp_(\w+)\(", src[a:b], flags=re.M))


def grid():
    """(entry, dtype) of every registry entry that runs through launch_ew"""
    return [(e, dt) for e in REGISTRY.values() if not e.device_only for dt in e.dtypes]


def grid_id(p):
    return f"{p[0].name}-{dtid(p[1])}"


# ---- running an entry -------------------------------------------------------------------------------------------------------------------
def operands(e, dt, n=None):
    """the CPU operands of an entry in dt (operand k: its range, salt 11 k + 1)"""
    return [table(e.ranges[k], dt, 11 * k + 1, n) for k in range(e.arity)]


def call(e, ops, scalars, out=None):
    """one call of lamp_<name> on STen operands; the result STen (the first operand of an in-place form, `out` of an _out form)"""
    fn = getattr(lib, "lamp_" + e.name)
    sc = [float(s) for s in scalars]
    if e.kind == "new":
        o = C.c_void_p()
        fn(C.byref(o), *ops, *sc)
        return S.STen(o)
    if e.kind == "inplace":
        fn(*ops, *sc)
        return ops[0]
    fn(out, *ops, *sc)
    return out


def reference(e, xs, scalars, dt):
    """the expected result in the dtype of the output: torch in dt for an exact entry, the float64 formula cast to dt otherwise"""
    if e.exact is not None and (e.ref is None or dt not in FLOATS):
        return e.exact(*xs, *scalars)
    kw = {"dt": dt} if e.name == "mul_add" else {}
    return e.ref(*[x.double() for x in xs], *scalars, **kw).to(dt)


def is_exact(e, dt):
    return e.exact is not None and (e.ref is None or dt not in FLOATS)


def bits(t):
    """a tensor's values for a bitwise comparison: the bytes of a bool tensor (a `true` stored as 2 is not 1)"""
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def check(e, dt, got, ref, scalars, what):
    """got (torch, as util.to_torch returns it) against the reference of `reference`"""
    if is_exact(e, dt):
        assert got.dtype == (torch.bool if e.bool_out else (F32 if dt == BF16 else dt)), f"{what}: dtype {got.dtype}"
        assert equal_bits(bits(got), bits(ref)), f"{what}: not bit-exact; first differences at {_diff(bits(got), bits(ref))}"
        return
    tol = TOL[dt] * e.tolmul(scalars)
    assert_close(got, ref.double(), tol, what)
    # a few huge results (exp(88), 20.5^3) carry the mean magnitude assert_close scales its absolute part with: the ordinary ones again
    # on their own
    r = ref.double()
    small = ~(r.abs() > 1e3)
    if not bool(small.all()):
        assert_close(got.double()[small], r[small], tol, what + " (|ref| <= 1e3)")


def _diff(got, ref):
    g, r = got.double().reshape(-1), ref.double().reshape(-1)
    if g.shape != r.shape:
        return f"shapes {list(got.shape)} vs {list(ref.shape)}"
    bad = ~((g == r) & (torch.signbit(g) == torch.signbit(r)) | (torch.isnan(g) & torch.isnan(r)))
    idx = torch.nonzero(bad).reshape(-1)[:5].tolist()
    return [(i, g[i].item(), r[i].item()) for i in idx]


def run(e, xs, scalars, make):
    """lamp_<name> on the CPU operands xs, each handed over as make(x) (an STen on either device, in any layout); the result as torch.
    An in-place or _out form has to write the storage it was given."""
    ops = [make(x) for x in xs]
    out = make(torch.zeros(torch.broadcast_shapes(*[x.shape for x in xs]), dtype=xs[0].dtype)) if e.kind == "out" else None
    target = out if e.kind == "out" else (ops[0] if e.kind == "inplace" else None)
    before = (target.data_ptr, target.storage_id, target.strides) if target is not None else None
    r = call(e, ops, scalars, out)
    if target is not None:
        assert r is target and (r.data_ptr, r.storage_id, r.strides) == before, f"{e.name}: the result is not in the argument's storage"
    return to_torch(r)


def run_and_check(e, dt, scalars, make, what, xs=None):
    """one case of an entry against its reference; a twin also bit for bit against its out-of-place form.  Returns the result."""
    xs = operands(e, dt) if xs is None else xs
    got = run(e, xs, scalars, make)
    check(e, dt, got, reference(e, xs, scalars, dt).expand(got.shape), scalars, what)
    if e.base is not None:
        base = run(REGISTRY[e.base], xs, scalars, make)
        assert equal_bits(bits(got), bits(base)), f"{what}: differs from lamp_{e.base}: {_diff(bits(got), bits(base))}"
    return got


def on_host(x):
    return to_sten(x, device=-1)


# ---- converting copies ----------------------------------------------------------------------------------------------------------------------
CAST_R, CAST_N = 37, 29          # 1073 elements: five blocks of the scalar copy kernels, the last one partial
INT_RANGE = {I64: (-2.0 ** 62, 2.0 ** 62), I32: (-2.0 ** 31 + 1, 2.0 ** 31 - 1), U8: (0.0, 255.0)}
# float -> float: nan, +-inf, +-0.0, the f32 -> bf16 ties 1 + 2^-8 (down to even) and 1 + 3 * 2^-8 (up to even), 3.4e38 (inf in bf16),
# 1e-320 (an f64 subnormal: 0 in the others), 65520 (the tie that is inf in f16) and 70000, 1 + 2^-8 + 2^-30 in f64 (a double rounding
# through f32 gives bf16 1.0, one rounding 1 + 2^-7; ATen goes through f32), and what decides a cast to bool: fractions, 256, 1e-3
CAST_SPECIALS = [NAN, INF, -INF, 0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.4e38, -3.4e38, 1e-320, 65520.0, 70000.0, -70000.0,
                 1.00390625 + 2.0 ** -30, 0.5, -0.25, 256.0, 1e-3, 2.0, 255.0, 1e-8]


def cast_source(src, dst, n=CAST_R * CAST_N):
    """[n] values in src for a copy into dst.  Float -> integer holds only values inside the destination's range and no NaN (anything
    else is undefined in C++ and in ATen); everything else takes the specials above, or the integer table plus 256 and 512"""
    i = torch.arange(n, dtype=torch.int64)
    if src in FLOATS:
        if dst in INTS:
            lo, hi = INT_RANGE[dst]
            lo, hi = max(lo, -60000.0), min(hi, 60000.0)                       # inside f16 as well
            v = lo + (hi - lo) * ((i * 7919) % 1009).to(F64) / 1008.0          # fractions: truncation toward zero
            v[:6] = torch.tensor([0.0, -0.0, 0.5, 1.5, 2.5, 0.999], dtype=F64)
            if dst != U8:
                v[6:9] = torch.tensor([-0.5, -1.5, -2.999], dtype=F64)
            return v.to(src)
        v = -300.0 + 600.0 * ((i * 7919) % 1009).to(F64) / 1008.0
        for k in range(0, n, 97):                                           # 97: the specials move through the lanes and the blocks
            m = min(len(CAST_SPECIALS), n - k)
            v[k:k + m] = torch.tensor(CAST_SPECIALS[:m], dtype=F64)
        return v.to(src)
    v = int_table(src, 3, n)
    if src in (I64, I32):
        v[5:9] = torch.tensor([256, 512, -256, 65536], dtype=src)
    elif src == U8:
        v[5:9] = torch.tensor([2, 128, 254, 16], dtype=src)
    return v


def cast_forms(src, dst, device):
    """every way a converting copy is reached, as (what, result as torch, expected): lamp_cast and lamp_to on a contiguous source
    (copy_contig_kernel<D, S>) and on a transposed 2-D view (copy_strided_kernel<D, S>), lamp_copy_ into a destination of the other
    dtype: contiguous, transposed, and a [1, N] source broadcast into [R, N]"""
    x = cast_source(src, dst)
    x2 = x.reshape(CAST_R, CAST_N)
    X, X2 = to_sten(x, device=device), to_sten(x2, device=device)
    ld = TORCH2LAMP[dst]
    forms = [("cast contiguous", X.castToType(ld), x.to(dst)),
             ("to contiguous", X.to(dtype=ld), x.to(dst)),
             ("cast transposed", X2.t.castToType(ld), x2.t().to(dst)),
             ("to transposed", X2.t.to(dtype=ld), x2.t().to(dst))]
    for what, source, exp in (("copy_ contiguous", X, x.to(dst)), ("copy_ transposed", X2.t, x2.t().to(dst)),
                              ("copy_ broadcast", X2.narrow(0, 3, 1), x2[3:4].to(dst).expand(CAST_R, CAST_N))):
        D = to_sten(torch.zeros(exp.shape, dtype=dst), device=device)
        D.copyFrom(source)
        forms.append((what, D, exp))
    out = []
    for what, got, exp in forms:
        assert got.dtype == ld, what
        out.append((what, to_torch(got), exp.contiguous()))
    return out


def check_cast(src, dst, device):
    for what, got, exp in cast_forms(src, dst, device):
        assert list(got.shape) == list(exp.shape), what
        assert equal_bits(bits(got), bits(exp)), f"{dtid(src)} -> {dtid(dst)} {what}: not bit-exact; first differences at {_diff(bits(got), bits(exp))}"


CAST_PAIRS = [(s, d) for s in ALL_BOOL for d in ALL_BOOL]


def cast_id(p):
    return f"{dtid(p[0])}-to-{dtid(p[1])}"
