"""RAdam, Yogi and the learning-rate schedules without a GPU: the restatement of tests/optim_ref.py reproduces the reference's own
known answers (adamw.test.scala:43-67,128-155), RAdam's branch switches where its formula says, Yogi's sign is that of the ROUNDED
square, the schedules give the reference's values (reducelronplateau.test.scala), and the public names exist.  The restated AdamW and SGDW
reproduce the golden known answers and agree bit for bit with the oracle's classes, and the inputs of tests/test_optimizers_size_gpu.py
are checked for what that file's rules need of them."""
import numpy as np
import pytest
import torch

from tests import optim_ref as R

K = R.KATS


def test_restated_radam_reproduces_the_reference_kat():
    k = K["radam"]
    p = torch.tensor([k["init"]], dtype=torch.float64)
    g = torch.tensor([k["gradients"]], dtype=torch.float64)
    opt = R.RAdam([p], k["weightDecay"], k["learningRate"], k["beta1"], k["beta2"])
    opt.step([g], 1.0)
    assert p[0].tolist() == k["step1"]
    opt.step([g], 1.0)
    assert p[0].tolist() == k["step2"]
    assert g[0].tolist() == k["gradients"], "RAdam only reads its gradients"


def test_restated_yogi_reproduces_the_reference_kat_by_mutating_the_gradient():
    k = K["yogi"]
    p = torch.tensor([k["init"]], dtype=torch.float64)
    g = torch.tensor([k["gradients"]], dtype=torch.float64)
    opt = R.Yogi([p], k["weightDecay"], k["learningRate"], k["beta1"], k["beta2"])
    opt.step([g], 1.0)
    assert np.array_equal(np.round(p[0].numpy(), 4), np.round(k["step1"], 4))
    assert g[0].tolist() == k["gradients_after_step1"]
    opt.step([g], 1.0)                                   # the same tensor, now -g^2, as the reference's test does
    assert np.array_equal(np.round(p[0].numpy(), 4), np.round(k["step2"], 4))
    # a second step on the ORIGINAL gradient gives other values: the write-back is part of the known answer
    p2 = torch.tensor([k["init"]], dtype=torch.float64)
    o2 = R.Yogi([p2], k["weightDecay"], k["learningRate"], k["beta1"], k["beta2"])
    for _ in range(2):
        o2.step([torch.tensor([k["gradients"]], dtype=torch.float64)], 1.0)
    assert not np.array_equal(np.round(p2[0].numpy(), 4), np.round(k["step2"], 4))


@pytest.mark.parametrize("b2", [0.999, 0.9])
def test_radam_is_unrectified_for_four_steps(b2):
    assert [R.radam_is_rectified(b2, t) for t in range(1, 9)] == [False] * 4 + [True] * 4


def test_radam_is_never_rectified_at_beta2_one_half():
    assert R.radam_rho(0.5, 1)[1] <= 4                   # rhoInf = 3: (rhoInf - 4) must not be used
    assert not any(R.radam_is_rectified(0.5, t) for t in range(1, 2000))
    assert R.radam_rho(0.6, 1)[1] <= 4 + 1e-12           # the largest beta2 that is never rectified


def test_the_gpu_descriptor_case_crosses_the_radam_branches():
    """what the eight steps of tests/test_optimizers_gpu.py's descriptor case are meant to exercise"""
    from tests import test_optimizers_gpu as G
    assert len(G.SIZES) == 46 and G.STEPS == 8
    assert [R.radam_is_rectified(0.999, t) for t in range(1, G.STEPS + 1)] == [False] * 4 + [True] * 4
    assert not any(R.radam_is_rectified(0.5, t) for t in range(1, G.STEPS + 1))
    assert sorted(set(G.HYPER["beta2"])) == [0.5, 0.999] and G.HYPER["beta2"].count(0.5) == 2


def test_radam_branch_changes_the_update():
    """steps 1-4 move the parameter by stepParam * m only (no second moment in the update), step 5 divides by sqrt(v) + eps"""
    p = torch.ones(3, dtype=torch.float64)
    g = torch.tensor([0.5, -2.0, 4.0], dtype=torch.float64)
    opt = R.RAdam([p], 0.0, 0.1, 0.9, 0.999)
    for t in range(1, 5):
        before = p.clone()
        opt.step([g.clone()], 1.0)
        np.testing.assert_allclose((p - before).numpy(), (-0.1 * g).numpy(), rtol=1e-12)   # m / (1 - b1^t) == g for a constant gradient
    before = p.clone()
    opt.step([g.clone()], 1.0)
    d = (p - before) / before.new_tensor(-0.1) / torch.sign(g)
    assert float(d.max() - d.min()) < 1e-6 and float(d.max()) < 0.5, "rectified: the step no longer scales with |g|"


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_yogi_leaves_v_where_it_equals_the_rounded_square(dt):
    g0 = torch.tensor([0.3, 0.7, 0.0, 0.3], dtype=dt)
    v0 = g0 * g0                                         # as rounded by torch
    v0[3] = 1.0                                          # a control that does move
    if dt == torch.float32:                              # these squares are inexact: the exact product differs from the rounded one
        assert all(float(x) * float(x) != float(x * x) for x in g0[:2])
    p, g = torch.ones(4, dtype=dt), g0.clone()
    opt = R.Yogi([p], 0.0, 0.01, 0.9, 0.999)
    opt.vt[0].copy_(v0)
    opt.step([g], 1.0)
    assert torch.equal(opt.vt[0][:3], v0[:3])
    assert opt.vt[0][3] != v0[3]
    assert g[:3].tolist() == [0.0, 0.0, 0.0] and g[3] == g0[3] * g0[3]


def test_restated_adamw_reproduces_the_reference_kats():
    """test_oracle_kat.py's test_adamw_kats with the restatement: exact where the reference compares with ==, rounded where it rounds"""
    from tests import kats
    g = kats.GOLDEN["adamw"]
    for key in ("no_weight_decay", "weight_decay"):
        p = torch.tensor([g["init"]], dtype=torch.float64)
        grad = torch.tensor([g["gradients"]], dtype=torch.float64)
        opt = R.AdamW([p], g[key]["weightDecay"], g["learningRate"], g["beta1"], g["beta2"])
        digits = g[key].get("roundTo")
        for step in ("step1", "step2"):
            opt.step([grad], 1.0)
            if digits:
                assert np.array_equal(np.round(p.numpy()[0], digits), np.round(g[key][step], digits))
            else:
                assert p.numpy()[0].tolist() == g[key][step]
    p = torch.tensor([g["init"]], dtype=torch.float64).half()          # fp16 parameters with an f32 working copy
    grad = torch.tensor([g["gradients"]], dtype=torch.float64).half()
    opt = R.AdamW([p], g["half_mixed"]["weightDecay"], g["learningRate"], g["beta1"], g["beta2"], mixedPrecision=True)
    for step in ("step1", "step2"):
        opt.step([grad], 1.0)
        assert p.double().numpy()[0].tolist() == g["half_mixed"][step]
    st = opt.state()
    assert len(st) == 4 and st[0] == 2.0 and all(t.dtype == torch.float32 for t in st[1:]) and st[3] is opt.workingCopy[0]
    assert torch.equal(p, st[3].half()), "the model parameter is the cast of the working copy, which comes last in the state"


def test_restated_sgdw_and_clipping_reproduce_the_reference_kats():
    from tests import kats
    g = kats.GOLDEN["sgd"]
    for key in ("noop", "no_momentum_no_wd", "no_momentum"):
        p = torch.ones(1, 2, dtype=torch.float64)
        R.SGDW([p], g[key]["lr"], g[key]["wd"]).step([torch.tensor([g[key]["grad"]], dtype=torch.float64)], 1.0)
        assert np.allclose(p.numpy()[0], g[key]["expect"], rtol=0, atol=1e-15)
    p = torch.ones(1, 2, dtype=torch.float64)
    opt = R.SGDW([p], g["two_steps"]["lr"], g["two_steps"]["wd"])
    grad = torch.tensor([g["two_steps"]["grad"]], dtype=torch.float64)
    for step in ("step1", "step2"):
        opt.step([grad], 1.0)
        assert np.array_equal(np.round(p.numpy()[0], 4), np.round(g["two_steps"][step], 4))
    c = kats.GOLDEN["gradient_clipping"]
    ts = [torch.ones(s, dtype=torch.float64) for s in c["shapes"]]
    R.gradient_clipping_in_place(ts, c["theta"])
    assert np.array_equal(np.round(ts[0].numpy().reshape(-1), 4), np.round(np.full(6, c["expect"]), 4))


@pytest.mark.parametrize("form", ["f64", "f32", "bf16-mixed"])
def test_restated_adamw_and_sgdw_agree_bit_for_bit_with_the_oracle(form):
    """at scalar hyperparameters, eight steps on the inputs of tests/test_optimizers_size_gpu.py (one gradient None, one step at
    scheduleFactor 0.5): AdamW with and without debias, SGDW with and without momentum and weight decay"""
    from oracle import lamp_oracle as O
    from tests import test_optimizers_size_gpu as Z
    dt = {"f64": torch.float64, "f32": torch.float32, "bf16-mixed": torch.bfloat16}[form]
    mixed = form == "bf16-mixed"
    params0, steps = Z.size_inputs()
    same = lambda xs, ys: len(xs) == len(ys) and all(torch.equal(Z.bits(x), Z.bits(y)) for x, y in zip(xs, ys))

    def run(make_r, make_o, state_o):
        pr, po = [p.to(dt).clone() for p in params0], [p.to(dt).clone() for p in params0]
        r, o = make_r(pr), make_o(po)
        for gs, f in zip(steps, Z.FACTORS):
            r.step([None if g is None else g.to(dt).clone() for g in gs], f)
            o.step([None if g is None else g.to(dt).clone() for g in gs], f)
            assert same(pr, po) and same(r.state()[-len(state_o(o)):] if state_o(o) else [], state_o(o))
    for debias in ((True, False) if not mixed else (True,)):
        hyper = dict(weightDecay=0.05, learningRate=0.01, beta1=0.9, beta2=0.999, debias=debias, mixedPrecision=mixed, clip=5.0 if debias else None)
        run(lambda p: R.AdamW(p, **hyper), lambda p: O.AdamW(p, **hyper), lambda o: o.mt + o.vt + [w for w in o.workingCopy if w is not None])
    if not mixed:
        for momentum, wd in ((None, 0.0), (None, 0.05), (0.9, 0.0), (0.9, 0.05)):
            run(lambda p: R.SGDW(p, 0.01, wd, momentum), lambda p: O.SGDW(p, 0.01, wd, momentum), lambda o: [v for v in o.velocity if v is not None])


def test_the_size_tests_inputs_are_what_they_are_meant_to_be():
    """the seed checks of tests/test_optimizers_size_gpu.py that need no GPU: the f32 yardstick of every f32 rule stays within 2^-20 of
    each tensor's largest magnitude, the exact norm of the bf16 clipping case is far from a rounding midpoint, and the misaligned layout's
    offsets land on every residue of 16 bytes with an aligned parameter next to a misaligned gradient"""
    from tests import test_optimizers_size_gpu as Z
    assert Z.SIZES == [1, 7, 1024, 1025, 2049] + [3] * 41 and Z.FACTORS.count(0.5) == 1 and len(Z.FACTORS) == Z.STEPS == 8
    params0, steps = Z.size_inputs()
    assert steps[0][Z.NONE_AT] is None and all(7.0 <= abs(float(g[j])) <= 9.0 and float(g[j]) * 16 % 1 == 0 for gs in steps for g in gs if g is not None for j in Z.sentinel_at(g.numel()))
    assert Z.sentinel_at(2049) == [0, 1023, 1024, 2048] and Z.sentinel_at(1024) == [0, 1023] and Z.sentinel_at(1) == [0]
    hy = Z.ADAMW_HYPER
    assert hy["beta2"].count(0.998) == 2 and hy["weightDecay"].count(0.0) == 2 and hy["learningRate"].count(0.02) == 1

    def yardstick(ref, chain, kinds):
        worst = 0.0
        for s, r in zip(chain, ref):
            for k in range(kinds):
                for a, b in zip(s[k], r[k]):
                    if b.any():                          # (the moments of the tensor without a gradient stay zero)
                        worst = max(worst, float((a.double() - b).abs().max()) / float(b.abs().max()))
                    else:
                        assert not a.any()
        return worst
    worst = {"adamw f32": yardstick(Z.adamw_restated(torch.float64), Z.adamw_restated(torch.float32), 3)}
    for store in (torch.bfloat16, torch.float16):
        worst[f"adamw mixed {store}"] = yardstick(Z.adamw_restated(torch.float64, store), Z.adamw_restated(torch.float32, store), 3)
    for momentum, wd in ((None, 0.0), (None, 0.05), (0.9, 0.0), (0.9, 0.05)):
        worst[f"sgdw {momentum} {wd}"] = yardstick(Z.sgdw_restated(torch.float64, momentum, wd), Z.sgdw_restated(torch.float32, momentum, wd),
                                                   1 if momentum is None else 2)
    for kind in ("radam", "yogi"):
        worst[kind] = yardstick(Z.moment_restated(kind, torch.float64), Z.moment_restated(kind, torch.float32), 3)
    print({k: f"2^{np.log2(v):.2f}" for k, v in worst.items()})
    assert all(v <= 2.0 ** -20 for v in worst.values()), worst

    # The f32 rule must hold for every contraction the compiler may choose, not for one: AdamW's moments as the chain rounds them (1), with
    # the product of the gradient fused into the addition (2), and with the decay product fused into it (3; what the (f32, 16-bit)
    # instantiation does).  On these inputs all three stay within the factor 2 of the chain.
    ref = Z.adamw_restated(torch.float64, torch.bfloat16)
    f32, fma = np.float32, lambda a, b, c: (a.astype(np.float64) * b + c).astype(np.float32)
    dist = {}
    for form in (1, 2, 3):
        dm = dv = 0.0
        for i, n in enumerate(Z.SIZES):
            if i == Z.NONE_AT:
                continue
            b1, c1, b2, c2 = f32(0.9), f32(1.0 - 0.9), f32(hy["beta2"][i]), f32(1.0 - hy["beta2"][i])
            m, v = np.zeros(n, f32), np.zeros(n, f32)
            for s in range(Z.STEPS):
                g = steps[s][i].to(torch.bfloat16).float().numpy()
                m = [None, m * b1 + c1 * g, fma(g, c1, m * b1), fma(m, b1, c1 * g)][form]
                v = [None, v * b2 + (c2 * g) * g, fma(c2 * g, g, v * b2), fma(v, b2, (c2 * g) * g)][form]
                dm = max(dm, float(np.abs(m - ref[s][1][i].numpy()).max()))
                dv = max(dv, float(np.abs(v - ref[s][2][i].numpy()).max()))
        dist[form] = (dm, dv)
    print("moment distances by contraction form", dist)
    assert all(dist[f][k] <= 2 * dist[1][k] for f in (2, 3) for k in (0, 1)), dist

    gs = Z.clip_inputs(torch.bfloat16)
    d = Z.addition_depth(torch.bfloat16, 1, Z.largest_group([g.numel() for g in gs]))
    norm = Z.exact_norm(gs)
    margin = Z.midpoint_margin(norm, torch.bfloat16)
    print(f"bf16 clipping: d = {d}, exact norm {norm!r}, {margin:.3e} from a rounding midpoint, needed {4 * d * Z.acc_eps(torch.bfloat16):.3e}")
    assert d == 27 and margin >= 4 * d * Z.acc_eps(torch.bfloat16)
    assert Z.addition_depth(torch.float32, 1, 43) == Z.addition_depth(torch.float64, 1, 43) == 23
    assert Z.midpoint_margin(1.0 + 2.0 ** -8, torch.bfloat16) == 0.0 and Z.midpoint_margin(1.0, torch.bfloat16) == 2.0 ** -9

    for k, isz in ((2, 8), (2, 4), (2, 2), (1, 8), (1, 4), (1, 2)):
        offs, total = Z.view_offsets(Z.SIZES if k == 2 else [g.numel() for g in gs], k)
        res = [[o * isz % 16 for o in col] for col in offs]
        assert {r for col in res for r in col} == set(range(0, 16, isz)), (k, isz)
        assert k == 1 or any(a == 0 and b != 0 for a, b in zip(res[0], res[1])), (k, isz)
        flat = sorted((o, n) for col in offs for o, n in zip(col, Z.SIZES if k == 2 else [g.numel() for g in gs]))
        assert flat[0][0] == 1 and all(o + n <= o2 for (o, n), (o2, _) in zip(flat, flat[1:])) and flat[-1][0] + flat[-1][1] + 3 == total


def test_reduce_lr_on_plateau_sequence():
    from lamp_amd.nn import LearningRateSchedule as L
    k = K["reduce_lr_on_plateau"]
    lrs = L.reduceLROnPlateau(stopFactor=k["stopFactor"])
    st = lrs.init
    for epoch, loss, expected in k["sequence"]:
        st, f = lrs.learningRateFactor(st, epoch, loss)
        assert f == expected, (epoch, loss, f, expected)
    with pytest.raises(AssertionError):
        lrs.learningRateFactor(lrs.init, 0, None)


def test_epoch_count_schedules():
    from lamp_amd.nn import LearningRateSchedule as L

    def at(s, e):
        st, f = s.learningRateFactor(s.init, e, None)
        assert st == s.init
        return f
    assert [at(L.noop(), e) for e in (0, 7)] == [1.0, 1.0]
    d = L.decrement(20, 0.5)
    assert [at(d, e) for e in (0, 19, 20, 40)] == [1.0, 1.0, 0.5, 0.25]
    lin = L.linear(1.0, 0.1, 10)
    assert at(lin, 0) == 1.0 and at(lin, 5) == 1.0 + (0.1 - 1.0) * 0.5 and at(lin, 10) == 0.1
    assert at(lin, 11) == 0.1 and at(lin, 1000) == 0.1, "linear clamps at `end`"
    s = L.stepAfter(3, 0.2)
    assert [at(s, e) for e in (0, 3, 4)] == [1.0, 1.0, 0.2]
    c = L.cyclicSchedule(3.0, 10)
    assert at(c, 0) == 1.0 and at(c, 5) == 3.0 and at(c, 10) == 1.0        # start, half a period, a full period
    assert at(c, 2) == 1.0 + 2.0 * (2 / 5.0)
    assert at(c, 7) == 3.0 + (3.0 + (1.0 - 3.0) * (7 / 5.0))               # the falling half as LearningRateSchedule.scala:105-111 writes it
    assert L.interpolate(1.0, 3.0, 4.0, 1.0) == 1.5
    assert at(L.fromEpochCount(lambda e: e * 2), 4) == 8.0


def test_public_names_exist():
    from lamp_amd import nn
    for name in ("RAdam", "RAdam_factory", "Yogi", "Yogi_factory", "LearningRateSchedule"):
        assert callable(getattr(nn, name, None)), name
    for name in ("noop", "decrement", "linear", "stepAfter", "cyclicSchedule", "fromEpochCount", "interpolate", "reduceLROnPlateau"):
        assert callable(getattr(nn.LearningRateSchedule, name, None)), name
    from lamp_amd._capi import parse_header, HEADERS
    decls = {}
    for h in HEADERS:
        decls.update(parse_header(h))
    for fn in ("lamp_radam_step_", "lamp_yogi_step_", "lamp_optimizer_radam", "lamp_optimizer_yogi"):
        assert fn in decls, fn
