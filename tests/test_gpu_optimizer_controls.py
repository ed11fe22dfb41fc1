"""GPU: the controlled optimizer step (csrc/optimizer_ctl.hip, DESIGN K22) through ``native.optimizer_ctl_step`` and the
``FusedAdam`` / ``FusedSGD`` objects - the gradient norm's accuracy and reproducibility, every rule one step at a time against
float64 from the kernel's own fp32 state (tests/optimizer_control_cases.py: definitions and per-element bars, proven on the host in
tests/test_optimizer_controls_host.py), the tick's scalars along three schedules, the padding invariant, the skip on a non-finite
gradient (ordinary data: nothing here provokes a device error), the untouched default path, a captured step that replays a
schedule, and the guards."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import adam_cases as A
from tests import optimizer_control_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = "second_grid_stride_pass"
SCALARS = ("step_size", "bc2_sqrt", "decay", "clip_coef", "lr")


def _native():
    from graphnet_classifier_amd import native
    return native


def _second_norm_pass():
    return _native().GRAD_NORM_PASS + 1027  # the norm's grid-stride loop makes a second pass, then a tail


def _n(size):
    if size != GRID:
        return size
    cus = torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count
    return cus * 8 * 1024 + 1027  # past the element grid's first pass (and the norm's eighth)


def _new(name, n, wd=0.0, max_norm=None, schedule=C.SCHEDULE, t=0, skip=False, lr=C.LR):
    """A rule's device state from the recipe: [p, (m, v) | (buf)], the counter at ``t`` and the control buffers."""
    native = _native()
    rule, mu, nesterov = C.RULES[name]
    sched = dict(schedule)
    ctl = native.opt_ctl(rule, lr, betas=C.BETAS, eps=C.EPS, weight_decay=wd, momentum=mu, nesterov=nesterov, max_grad_norm=max_norm,
                         check_nonfinite=skip, schedule=sched.pop("kind", "constant"), **sched)
    return SimpleNamespace(
        name=name, ctl=ctl, state=[torch.from_numpy(a).to(DEV) for a in C.initial_state(name, n)],
        counter=torch.full((1,), t, dtype=torch.int64, device=DEV),
        scalars=torch.zeros(native.OPT_SCALARS, device=DEV), skipped=torch.zeros(2, dtype=torch.int64, device=DEV),
        partials=torch.zeros(native.GRAD_NORM_BLOCKS, dtype=torch.float64, device=DEV))


def _tensors(o):
    return list(o.state) + [o.counter, o.scalars, o.skipped]


def _step(o, g):
    s = o.state + [None, None]
    _native().optimizer_ctl_step(s[0], g, s[1], s[2], o.counter, o.scalars, o.skipped, o.partials, o.ctl)


def _host(tensors):
    return [t.cpu().numpy().copy() for t in tensors]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(xs, ys) -> bool:
    return all(torch.equal(_bits(a), _bits(b)) for a, b in zip(xs, ys))


def _within_one_ulp(got, want) -> bool:
    return abs(float(got) - float(np.float32(want))) <= float(np.spacing(np.float32(want)))


# --------------------------------------------------------------------------- the norm
@pytest.mark.parametrize("size", A.SIZES + ("second_norm_pass",))
def test_grad_norm_is_the_float64_norm_and_depends_on_the_values_alone(size):
    n = _second_norm_pass() if size == "second_norm_pass" else size
    g_host = A.gradient(n, 3) if n > 1 else np.array([0.75], np.float32)  # the recipe's element 0 is 0
    g = torch.from_numpy(g_host).to(DEV)
    o = _new("sgd", n, max_norm=1.0)
    _step(o, g)
    first, partials = o.scalars.clone(), o.partials.clone()
    want = C.norm64(g_host)
    print(f"n={n}: grad_norm {float(first[5])!r} / {want!r}   clip_coef {float(first[3])!r}")
    assert _within_one_ulp(first[5], want) and _within_one_ulp(first[3], C.clip_coef64(g_host, 1.0))
    _step(o, g)  # p has moved, g has not
    assert torch.equal(_bits(o.scalars[5:6]), _bits(first[5:6])) and torch.equal(o.partials.view(torch.int64), partials.view(torch.int64))
    wide = torch.zeros(n + 8, device=DEV)
    moved = wide[4:4 + n]
    moved.copy_(g)
    assert moved.data_ptr() % 16 == 0 and moved.data_ptr() != g.data_ptr()
    other = torch.full_like(o.partials, -1.0)
    _native().grad_sumsq(moved, other)
    assert torch.equal(other.view(torch.int64), partials.view(torch.int64))  # every partial, bit for bit
    assert abs(float(other.sum().item()) - want * want) <= 1e-12 * want * want


def test_an_all_zero_gradient_has_norm_zero_and_a_coefficient_of_exactly_one():
    for n in (5, 1027, _second_norm_pass()):
        o = _new("adamw", n, wd=0.01, max_norm=1e-3)
        before = o.state[0].clone()
        _step(o, torch.zeros(n, device=DEV))
        assert float(o.scalars[5]) == 0.0 and float(o.scalars[3]) == 1.0 and o.skipped.tolist() == [0, 0] and int(o.counter) == 1
        assert not torch.equal(before, o.state[0]) and bool(torch.isfinite(o.state[0]).all())  # the decay still acts


# --------------------------------------------------------------------------- every rule, one step at a time
def _check_steps(name, n, wd, clip):
    max_norm = C.CLIPS[clip]
    rule = C.RULES[name][0]
    o = _new(name, n, wd, max_norm)
    for s in range(C.STEPS):
        before = _host(o.state)
        t = int(o.counter.item()) + 1
        g = A.gradient(n, s)
        lr_t = C.lr_at(t, C.LR, **C.SCHEDULE)
        ref, bar, _ = C.bars(name, before, g, t, lr_t, wd, max_norm)
        _step(o, torch.from_numpy(g).to(DEV))
        after = _host(o.state)
        scalars = o.scalars.cpu().numpy()
        assert int(o.counter.item()) == t == s + 1 and o.skipped.tolist() == [0, 0]
        coef = C.clip_coef64(g, max_norm)
        for label, got, want in zip(SCALARS, scalars, C.tick64(rule, t, lr_t, wd, coef)):
            assert _within_one_ulp(got, want), (label, s, got, want)
        if max_norm is None:
            assert np.isnan(scalars[5])  # no norm pass ran
        else:
            assert _within_one_ulp(scalars[5], C.norm64(g))
            if n >= 1023:
                assert (scalars[3] < 1.0) == (clip == "bites")
        ratios = [np.abs(got.astype(np.float64) - r) / b for got, r, b in zip(after, ref, bar)]
        print(f"{name} n={n} wd={wd} {clip} step {t}: error / bar  " + "  ".join(f"{r.max():.3f}" for r in ratios))
        for k, (got, r) in enumerate(zip(after, ratios)):
            assert np.isfinite(got).all() and (r <= 1.0).all(), (k, s, int(r.argmax()))  # NaN <= 1 is false
        dead = (g == 0) & ((before[0] == 0) | (wd == 0))
        for a in before[1:]:
            dead = dead & (a == 0)
        if wd == 0:
            assert dead[::7].all()  # every 7th element stays as FlatParameters' padding does
        for a, b in zip(before, after):
            assert np.array_equal(a[dead].view(np.uint32), b[dead].view(np.uint32))


@pytest.mark.parametrize("clip", list(C.CLIPS))
@pytest.mark.parametrize("wd", C.WDS)
@pytest.mark.parametrize("name", list(C.RULES))
def test_each_step_matches_float64_from_the_kernels_own_state(name, wd, clip):
    for n in C.SIZES:
        _check_steps(name, n, wd, clip)


@pytest.mark.parametrize("name", ["adam", "adamw", "sgd_nesterov"])
def test_each_step_matches_float64_in_the_element_grids_second_pass(name):
    _check_steps(name, _n(GRID), 0.01, "bites")


@pytest.mark.parametrize("schedule", C.TICK_SCHEDULES, ids=lambda s: s["kind"])
@pytest.mark.parametrize("name", ["adam", "adamw", "sgd_momentum"])
def test_tick_scalars_along_the_schedules(name, schedule):
    """lr, step size, decay and the clip coefficient as Python derives them in float64; one fp32 ulp for the device's cos and pow."""
    n, wd, max_norm = 5, 0.01, 1e-3
    g = A.gradient(n, 1)
    for t in C.TICK_STEPS:
        o = _new(name, n, wd, max_norm, schedule=schedule, t=t - 1)
        _step(o, torch.from_numpy(g).to(DEV))
        lr_t = C.lr_at(t, C.LR, **schedule)
        want = C.tick64(C.RULES[name][0], t, lr_t, wd, C.clip_coef64(g, max_norm))
        got = o.scalars.cpu().numpy()
        print(f"{name} {schedule['kind']} t={t}: " + "  ".join(f"{label} {a!r} / {b!r}" for label, a, b in zip(SCALARS, got, want)))
        assert int(o.counter.item()) == t and want[3] < 1.0
        for label, a, b in zip(SCALARS, got, want):
            assert _within_one_ulp(a, b), (label, t, a, b)


@pytest.mark.parametrize("wd", C.WDS)
@pytest.mark.parametrize("name", list(C.RULES))
def test_zero_gradient_zero_state_and_zero_value_stay_bit_unchanged(name, wd):
    """FlatParameters' padding under every rule, with a clip that bites: at every position of a float4 group, in the tail, and -0."""
    n = 1027
    o = _new(name, n, wd, 1e-3)
    pad = torch.tensor([0, 5, 513, 770, 1023, 1024, 1026], device=DEV)
    o.state[0][pad] = 0.0
    o.state[0][5] = -0.0
    for s in range(3):
        g = torch.from_numpy(A.gradient(n, s)).to(DEV)
        g[pad] = 0.0
        before = [t.clone() for t in o.state]
        _step(o, g)
        for a, b in zip(before, o.state):
            assert torch.equal(_bits(a[pad]), _bits(b[pad]))
        assert not torch.equal(before[0], o.state[0]) and float(o.scalars[3]) < 1.0


# --------------------------------------------------------------------------- non-finite gradients
NONFINITE = [(1027, 0), (1027, 513), (1027, 1026), ("second_norm_pass", "second_pass")]


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("size,index", NONFINITE, ids=lambda v: str(v))
@pytest.mark.parametrize("name,max_norm", [("adamw", 1e-3), ("sgd_momentum", None)], ids=["adamw-clip", "sgd-check"])
def test_a_non_finite_gradient_skips_the_step_and_is_counted(name, max_norm, size, index, value):
    n = _second_norm_pass() if size == "second_norm_pass" else size
    index = _native().GRAD_NORM_PASS + 5 if index == "second_pass" else index
    o = _new(name, n, 0.01, max_norm, skip=True)
    for s in range(2):
        _step(o, torch.from_numpy(A.gradient(n, s)).to(DEV))
    g = torch.from_numpy(A.gradient(n, 2)).to(DEV)
    g_bad = g.clone()
    g_bad[index] = value
    g_bad_before = g_bad.clone()
    snap = [t.clone() for t in _tensors(o)]
    _step(o, g_bad)
    assert _same_bits(o.state, snap) and int(o.counter.item()) == 2  # p, the state and the counter
    assert o.skipped.tolist() == [1, 1] and not np.isfinite(float(o.scalars[5]))
    assert _same_bits(o.scalars[:5], snap[-2][:5]) and _same_bits([g_bad], [g_bad_before])
    clean = copy.copy(o)
    clean.state, clean.counter, clean.scalars = [t.clone() for t in snap[:-3]], snap[-3].clone(), snap[-2].clone()
    clean.skipped, clean.partials = snap[-1].clone(), torch.zeros_like(o.partials)
    _step(clean, g)  # the step a run without the bad gradient takes from that state
    _step(o, g)
    assert _same_bits(o.state + [o.counter, o.scalars], clean.state + [clean.counter, clean.scalars]) and int(o.counter.item()) == 3
    assert o.skipped.tolist() == [1, 0] and clean.skipped.tolist() == [0, 0] and bool(torch.isfinite(o.state[0]).all())


def test_without_the_check_the_update_rule_runs_as_plain_adam_does():
    """``skip_nonfinite`` off and no clipping: no norm pass, nothing skipped - a NaN gradient reaches its own element only (the
    behaviour tests/test_gpu_adam.py pins for the default path)."""
    n = 1027
    o = _new("adamw", n, 0.01)
    g = torch.from_numpy(A.gradient(n, 0)).to(DEV)
    g[514] = float("nan")
    _step(o, g)
    assert o.skipped.tolist() == [0, 0] and int(o.counter.item()) == 1
    nan = torch.isnan(o.state[0])
    assert bool(nan[514]) and int(nan.sum()) == 1


# --------------------------------------------------------------------------- the optimizer objects
def _linear_pair():
    torch.manual_seed(3)
    a = torch.nn.Linear(37, 5).to(DEV)  # 185 + 5 parameters: two padded segments, with gaps
    return a, copy.deepcopy(a)


def test_fused_adam_without_options_is_the_plain_adam_step_bit_for_bit():
    from graphnet_classifier_amd import native
    from graphnet_classifier_amd.train import FlatParameters, FusedAdam
    lin, _ = _linear_pair()
    fp = FlatParameters(lin)
    opt = FusedAdam(fp)
    assert not opt.controlled and len(opt.state_snapshot()) == 4
    n = fp.numel
    p, m, v = fp.flat.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    counter, scratch = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(2, device=DEV)
    for s in range(3):
        g = torch.from_numpy(A.gradient(n, s)).to(DEV)
        fp.grad.copy_(g)
        opt.step(reduce=False)
        native.adam_step(p, g, m, v, counter, scratch, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert _same_bits([fp.flat, opt.exp_avg, opt.exp_avg_sq, opt.step_count, opt._scratch], [p, m, v, counter, scratch])
    assert float(opt.current_lr) == float(np.float32(1e-3)) and int(opt.skipped_steps) == 0 and np.isnan(float(opt.grad_norm))


def test_fused_sgd_matches_the_native_step_and_restores_every_state_tensor():
    from graphnet_classifier_amd.train import FlatParameters, FusedSGD
    lin, _ = _linear_pair()
    fp = FlatParameters(lin)
    sched = dict(kind="step", warmup_steps=1, gamma=0.5, every=2)
    opt = FusedSGD(fp, 1e-2, momentum=0.9, nesterov=True, weight_decay=0.01, max_grad_norm=0.5, lr_schedule=sched)
    n = fp.numel
    o = _new("sgd_nesterov", n, 0.01, 0.5, schedule=sched, lr=1e-2)
    o.state[0] = fp.flat.clone()
    snap = opt.state_snapshot()
    for s in range(4):
        g = torch.from_numpy(A.gradient(n, s)).to(DEV)
        fp.grad.copy_(g)
        opt.step(reduce=False)
        _step(o, g)
    assert _same_bits([fp.flat, opt.momentum_buffer, opt.step_count, opt._controls.scalars, opt._controls.skipped], _tensors(o))
    assert _within_one_ulp(opt.current_lr, C.lr_at(4, 1e-2, **sched)) and float(opt.current_lr) == float(np.float32(0.5e-2))
    assert _within_one_ulp(opt.grad_norm, C.norm64(A.gradient(n, 3))) and int(opt.skipped_steps) == 0
    opt.state_restore(snap)
    assert int(opt.step_count) == 0 and _same_bits(opt.state_snapshot(), snap) and not bool(opt.momentum_buffer.any())


def test_one_captured_step_replays_a_schedule_and_a_second_capture_continues_it():
    from graphnet_classifier_amd.train import FlatParameters, FusedAdam
    sched = dict(kind="cosine", warmup_steps=2, total_steps=6, min_lr=1e-5)
    kw = dict(weight_decay=0.01, decoupled_weight_decay=True, max_grad_norm=1e-2, lr_schedule=sched)
    a, b = _linear_pair()
    fa, fb = FlatParameters(a), FlatParameters(b)
    cap, eager = FusedAdam(fa, **kw), FusedAdam(fb, **kw)
    n = fa.numel

    def state(opt):
        return [opt.fp.flat, opt.exp_avg, opt.exp_avg_sq, opt.step_count, opt._controls.scalars, opt._controls.skipped]

    def eager_step(s):
        fb.grad.copy_(torch.from_numpy(A.gradient(n, s)).to(DEV))
        eager.step(reduce=False)

    fa.grad.copy_(torch.from_numpy(A.gradient(n, 0)).to(DEV))
    cap.step(reduce=False)  # moments that are not all zero when the capture starts; the kernels are loaded
    eager_step(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.step(reduce=False)
    assert int(cap.step_count.item()) == 1  # capturing ran nothing
    lrs = []
    for s in range(1, 5):
        fa.grad.copy_(torch.from_numpy(A.gradient(n, s)).to(DEV))
        graph.replay()
        eager_step(s)
        lrs.append(float(cap.current_lr.item()))
        assert _within_one_ulp(lrs[-1], C.lr_at(s + 1, 1e-3, **sched)) and float(cap._controls.scalars[3]) < 1.0
        assert _same_bits(state(cap), state(eager)), s  # the counters and the scalars included
    assert len(set(lrs)) == 4 and int(cap.step_count.item()) == int(eager.step_count.item()) == 5
    again = torch.cuda.CUDAGraph()
    with torch.cuda.graph(again):
        cap.step(reduce=False)
    fa.grad.copy_(torch.from_numpy(A.gradient(n, 5)).to(DEV))
    again.replay()
    eager_step(5)
    assert int(cap.step_count.item()) == 6 and _within_one_ulp(cap.current_lr, C.lr_at(6, 1e-3, **sched))
    assert float(cap.current_lr) == float(np.float32(1e-5)) and _same_bits(state(cap), state(eager))


# --------------------------------------------------------------------------- guards
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["param", "grad", "state1", "state2"])
def test_a_misaligned_buffer_raises_and_touches_nothing(which):
    n = 1024
    o = _new("adamw", n, 0.01, 1e-3, t=4)
    g = torch.from_numpy(A.gradient(n, 1)).to(DEV)
    _step(o, g)
    bufs = [o.state[0], g, o.state[1], o.state[2]]
    wide = torch.zeros(n + 4, device=DEV)
    view = wide[1:1 + n]
    view.copy_(bufs[which])
    bufs[which] = view
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    control = [o.counter, o.scalars, o.skipped, o.partials]
    snap = [t.clone() for t in bufs + control]
    with pytest.raises(RuntimeError):
        _native().optimizer_ctl_step(bufs[0], bufs[1], bufs[2], bufs[3], o.counter, o.scalars, o.skipped, o.partials, o.ctl)
    torch.cuda.synchronize()
    assert _same_bits(bufs + control, snap) and int(o.counter.item()) == 5


BAD_CTL = [("adamw", dict(beta1=1.0)), ("adamw", dict(beta2=-0.1)), ("adamw", dict(lr=-1e-3)), ("adamw", dict(lr=float("nan"))),
           ("adamw", dict(eps=-1e-8)), ("adamw", dict(weight_decay=-0.01)), ("adamw", dict(lr=10.0, weight_decay=0.1)),
           ("adamw", dict(max_grad_norm=0.0)), ("adamw", dict(max_grad_norm=float("nan"))), ("adamw", dict(total_steps=2)),
           ("adamw", dict(min_lr=1.0)), ("adamw", dict(warmup_steps=-1)), ("adamw", dict(rule=3)), ("adamw", dict(schedule=7)),
           ("sgd_momentum", dict(momentum=-0.5)), ("sgd", dict(nesterov=1)), ("sgd", dict(schedule=2, every=0)),
           ("sgd", dict(schedule=2, every=3, gamma=0.0))]


@pytest.mark.parametrize("name,bad", BAD_CTL, ids=str)
def test_hyper_parameters_out_of_range_raise_and_touch_nothing(name, bad):
    n = 1027
    o = _new(name, n, 0.01, 1e-3, t=2)
    g = torch.from_numpy(A.gradient(n, 1)).to(DEV)
    _step(o, g)
    snap = [t.clone() for t in _tensors(o) + [g, o.partials]]
    for key, value in bad.items():
        setattr(o.ctl, key, value)
    with pytest.raises(RuntimeError):
        _step(o, g)
    torch.cuda.synchronize()
    assert _same_bits(_tensors(o) + [g, o.partials], snap) and int(o.counter.item()) == 3


def test_the_wrapper_refuses_other_dtypes_strides_and_missing_buffers_and_empty_buffers_are_a_no_op():
    native = _native()
    n = 64
    o = _new("adamw", n, 0.01, 1e-3, t=1)
    g = torch.from_numpy(A.gradient(n, 1)).to(DEV)
    snap = [t.clone() for t in _tensors(o) + [g]]
    p, m, v = o.state

    def call(p=p, g=g, m=m, v=v, c=o.counter, s=o.scalars, k=o.skipped, part=o.partials, ctl=o.ctl):
        native.optimizer_ctl_step(p, g, m, v, c, s, k, part, ctl)

    for kw in (dict(p=p.double()), dict(g=g.half()), dict(p=torch.zeros(2 * n, device=DEV)[::2]), dict(g=g[:-1]), dict(m=None),
               dict(v=None), dict(c=o.counter.int()), dict(s=torch.zeros(2, device=DEV)), dict(k=torch.zeros(1, dtype=torch.int64, device=DEV)),
               dict(part=None), dict(part=torch.zeros(8, dtype=torch.float64, device=DEV)),
               dict(part=torch.zeros(native.GRAD_NORM_BLOCKS, device=DEV))):
        with pytest.raises(ValueError):
            call(**kw)
    sgd = _new("sgd", n)
    with pytest.raises(ValueError):
        native.optimizer_ctl_step(sgd.state[0], g, m, None, sgd.counter, sgd.scalars, sgd.skipped, None, sgd.ctl)  # a buffer, no momentum
    with pytest.raises(ValueError):
        native.grad_sumsq(g.double(), o.partials)
    torch.cuda.synchronize()
    assert _same_bits(_tensors(o) + [g], snap)
    empty = [torch.zeros(0, device=DEV) for _ in range(4)]
    native.optimizer_ctl_step(*empty, o.counter, o.scalars, o.skipped, o.partials, o.ctl)
    torch.cuda.synchronize()
    assert _same_bits(_tensors(o), snap[:-1]) and int(o.counter.item()) == 1  # as the plain Adam entry: not even the counter moves
