"""GPU: the flat Adam update (csrc/optimizer.hip) through ``native.adam_step``, one step at a time against float64 from the
kernel's own fp32 state (tests/adam_cases.py: definition, inputs, per-element bars of 4 x max(error of the fp32 emulation, one
ulp); proven on the host in tests/test_adam_host.py) - the n % 4 tail and n < 4, the grid-stride loop's second pass, weight
decay, the tick kernel's two scalars and its counter up to 2^31 + 5, the padding invariant, NaN containment inside a float4
group, the guards, and a graph replay."""
import numpy as np
import pytest
import torch

from tests import adam_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = "second_grid_stride_pass"


def _n(size):
    if size != GRID:
        return size
    cus = torch.cuda.get_device_properties(torch.device(DEV)).multi_processor_count
    return cus * 8 * 1024 + 1027  # one element past the capped grid's first pass, a full float4 pass more, and a tail


def _state(n, t=0, seed=0):
    """[p, m, v, counter, scratch] on the device: p ~ N(0, 1), m = v = 0, the counter at ``t``."""
    return [torch.from_numpy(A.params(n, seed)).to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV),
            torch.full((1,), t, dtype=torch.int64, device=DEV), torch.zeros(2, device=DEV)]


def _step(state, g, hyper, lr=A.LR, eps=A.EPS):
    from graphnet_classifier_amd import native
    p, m, v, counter, scratch = state
    wd, (b1, b2) = hyper
    native.adam_step(p, g, m, v, counter, scratch, lr, b1, b2, eps, wd)


def _host(state):
    return [t.cpu().numpy().copy() for t in state]


def _within_one_ulp(got, want) -> bool:
    return abs(float(got) - float(want)) <= float(np.spacing(np.float32(want)))


@pytest.mark.parametrize("hyper", A.HYPER, ids=A.hyper_id)
@pytest.mark.parametrize("size", A.SIZES + (GRID,))
def test_each_step_matches_float64_from_the_kernels_own_state(size, hyper):
    n = _n(size)
    wd, (b1, b2) = hyper
    state = _state(n)
    worst = [0.0, 0.0, 0.0]
    for s in range(A.STEPS):
        p, m, v, counter, _ = _host(state)
        t = int(counter[0]) + 1
        g = A.gradient(n, s)
        ref, bar, _ = A.bars(p, g, m, v, t, A.LR, b1, b2, A.EPS, wd)
        _step(state, torch.from_numpy(g).to(DEV), hyper)
        p2, m2, v2, counter2, scratch = _host(state)
        assert int(counter2[0]) == t == s + 1
        want = A.tick_scalars(t, A.LR, b1, b2)
        assert _within_one_ulp(scratch[0], want[0]) and _within_one_ulp(scratch[1], want[1]), (s, scratch, want)
        ratios = [np.abs(got.astype(np.float64) - r) / b for got, r, b in zip((p2, m2, v2), ref, bar)]
        worst = [max(w, float(r.max())) for w, r in zip(worst, ratios)]
        print(f"n={n} step {t}: error / bar  p {ratios[0].max():.3f}  m {ratios[1].max():.3f}  v {ratios[2].max():.3f}")
        for name, got, r in zip("pmv", (p2, m2, v2), ratios):
            assert np.isfinite(got).all() and (r <= 1.0).all(), (name, s, int(r.argmax()))  # NaN <= 1 is false
        dead = (g == 0) & (m == 0) & (v == 0) & ((p == 0) | (wd == 0))
        if wd == 0:
            assert dead[::7].all()  # every 7th element stays as FlatParameters' padding does: 0 gradient, 0 moments
        for before, after in ((p, p2), (m, m2), (v, v2)):
            assert np.array_equal(before[dead].view(np.uint32), after[dead].view(np.uint32))


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)], ids=str)
@pytest.mark.parametrize("t", A.TICK_STEPS)
def test_tick_kernel_scalars_and_counter(t, betas):
    """step_size and bias_correction2_sqrt as Python derives them from the hyper-parameters' doubles; one fp32 ulp for the
    device's pow, which is not bit-specified."""
    n = 5
    state = _state(n, t=t - 1)
    _step(state, torch.from_numpy(A.gradient(n, 1)).to(DEV), (0.0, betas))
    _, _, _, counter, scratch = _host(state)
    want = A.tick_scalars(t, A.LR, *betas)
    print(f"t={t} betas={betas}: step_size {scratch[0]!r} / {want[0]!r}   bc2_sqrt {scratch[1]!r} / {want[1]!r}")
    assert int(counter[0]) == t and counter.dtype == np.int64
    assert _within_one_ulp(scratch[0], want[0]), (scratch[0], want[0])
    assert _within_one_ulp(scratch[1], want[1]), (scratch[1], want[1])


def test_the_float_entry_is_the_double_entry_at_the_fp32_values():
    """``gnc_adam_step_f32`` widens its floats: bit for bit the step ``native.adam_step`` makes with hyper-parameters that are
    fp32 values to begin with."""
    from graphnet_classifier_amd import native
    lib = native.load_library()
    n = 1027
    wd, (b1, b2) = 0.01, (0.9, 0.999)
    as32 = lambda x: float(np.float32(x))  # noqa: E731
    a, b = _state(n), _state(n)
    for s in range(3):
        g = torch.from_numpy(A.gradient(n, s)).to(DEV)
        native.adam_step(a[0], g, a[1], a[2], a[3], a[4], as32(A.LR), as32(b1), as32(b2), A.EPS, wd)
        rc = lib.gnc_adam_step_f32(b[0].data_ptr(), g.data_ptr(), b[1].data_ptr(), b[2].data_ptr(), n, A.LR, b1, b2, A.EPS, wd,
                                   b[3].data_ptr(), b[4].data_ptr(), torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        assert rc == 0
    torch.cuda.synchronize()
    for name, x, y in zip(("p", "m", "v", "counter", "scratch"), a, b):
        assert torch.equal(x, y), name
    assert int(b[3].item()) == 3


def test_zero_gradient_and_zero_moments_leave_the_element_bit_unchanged():
    """The padding invariant of FlatParameters, also with weight decay where p is 0, at every position of a float4 group and in the tail."""
    n = 1027
    for hyper in A.HYPER:
        state = _state(n)
        pad = torch.tensor([0, 513, 770, 1023, 1024, 1026], device=DEV)
        state[0][pad] = 0.0
        state[0][5] = -0.0
        for s in range(3):
            g = torch.from_numpy(A.gradient(n, s)).to(DEV)
            g[pad] = 0.0
            g[5] = 0.0
            before = [t.clone() for t in state[:3]]
            _step(state, g, hyper)
            idx = torch.cat([pad, torch.tensor([5], device=DEV)])
            for a, b in zip(before, state[:3]):
                assert torch.equal(a[idx].view(torch.int32), b[idx].view(torch.int32))
            assert not torch.equal(before[0], state[0])


@pytest.mark.parametrize("index", [512, 513, 514, 515, 1025], ids=lambda i: f"i{i}")
def test_a_nan_gradient_changes_its_own_element_only(index):
    n = 1027
    hyper = (0.01, (0.9, 0.999))
    clean = _state(n)
    for s in range(2):
        _step(clean, torch.from_numpy(A.gradient(n, s)).to(DEV), hyper)
    bad = [t.clone() for t in clean]
    g = torch.from_numpy(A.gradient(n, 2)).to(DEV)
    g_bad = g.clone()
    g_bad[index] = float("nan")
    _step(clean, g, hyper)
    _step(bad, g_bad, hyper)
    others = torch.ones(n, dtype=torch.bool, device=DEV)
    others[index] = False
    for a, b in zip(clean[:3], bad[:3]):
        assert torch.equal(a[others], b[others]) and bool(torch.isnan(b[index])) and not bool(torch.isnan(a).any())
    assert int(bad[3].item()) == int(clean[3].item()) == 3


def _snapshot(state, g):
    return [t.clone() for t in state] + [g.clone()]


def _unchanged(state, g, snap) -> bool:
    return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(list(state) + [g], snap))


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["param", "grad", "exp_avg", "exp_avg_sq"])
def test_a_misaligned_buffer_raises_and_touches_nothing(which):
    from graphnet_classifier_amd import native
    n = 1024
    state = _state(n, t=4)
    g = torch.from_numpy(A.gradient(n, 1)).to(DEV)
    _step(state, g, A.HYPER[0])  # moments that are not all zero
    bufs = [state[0], g, state[1], state[2]]
    wide = torch.zeros(n + 4, device=DEV)
    view = wide[1:1 + n]
    view.copy_(bufs[which])
    bufs[which] = view
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    snap = [t.clone() for t in bufs] + [state[3].clone(), state[4].clone()]
    with pytest.raises(RuntimeError):
        native.adam_step(bufs[0], bufs[1], bufs[2], bufs[3], state[3], state[4], A.LR, 0.9, 0.999, A.EPS, 0.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs + [state[3], state[4]], snap)) and int(state[3].item()) == 5


@pytest.mark.parametrize("bad", [dict(b1=1.0), dict(b2=1.0), dict(b1=-0.1), dict(lr=-1e-3), dict(eps=-1e-8)], ids=str)
def test_hyper_parameters_out_of_range_raise_and_touch_nothing(bad):
    from graphnet_classifier_amd import native
    n = 1027
    state = _state(n, t=2)
    g = torch.from_numpy(A.gradient(n, 1)).to(DEV)
    _step(state, g, A.HYPER[0])
    snap = _snapshot(state, g)
    kw = dict(lr=A.LR, b1=0.9, b2=0.999, eps=A.EPS)
    kw.update(bad)
    with pytest.raises(RuntimeError):
        native.adam_step(state[0], g, state[1], state[2], state[3], state[4], kw["lr"], kw["b1"], kw["b2"], kw["eps"], 0.0)
    torch.cuda.synchronize()
    assert _unchanged(state, g, snap) and int(state[3].item()) == 3


def test_empty_buffers_are_a_no_op_and_the_wrapper_refuses_other_dtypes_and_strides():
    from graphnet_classifier_amd import native
    empty = [torch.zeros(0, device=DEV) for _ in range(4)]
    counter, scratch = torch.full((1,), 7, dtype=torch.int64, device=DEV), torch.full((2,), 0.25, device=DEV)
    native.adam_step(*empty, counter, scratch, A.LR, 0.9, 0.999, A.EPS, 0.0)
    torch.cuda.synchronize()
    assert int(counter.item()) == 7 and scratch.tolist() == [0.25, 0.25]  # current behaviour, pinned: not even the counter moves
    n = 64
    state = _state(n, t=1)
    g = torch.from_numpy(A.gradient(n, 1)).to(DEV)
    snap = _snapshot(state, g)
    call = lambda p, gr, m, v, c=state[3], s=state[4]: native.adam_step(p, gr, m, v, c, s, A.LR, 0.9, 0.999, A.EPS, 0.0)  # noqa: E731
    with pytest.raises(ValueError):
        call(state[0].double(), g, state[1], state[2])
    with pytest.raises(ValueError):
        call(state[0], g.half(), state[1], state[2])
    with pytest.raises(ValueError):
        call(torch.zeros(2 * n, device=DEV)[::2], g, state[1], state[2])
    with pytest.raises(ValueError):
        call(state[0], g, state[1], torch.zeros(n, 2, device=DEV)[:, 0])
    with pytest.raises(ValueError):
        call(state[0], g[:-1], state[1], state[2])
    with pytest.raises(ValueError):
        call(state[0], g, state[1], state[2], c=state[3].int())
    with pytest.raises(ValueError):
        call(state[0], g, state[1], state[2], s=torch.zeros(1, device=DEV))
    torch.cuda.synchronize()
    assert _unchanged(state, g, snap)


def test_one_captured_step_replays_as_three_eager_steps():
    n = 4099
    hyper = (0.01, (0.9, 0.999))
    warm = _state(n, seed=1)
    state = _state(n)
    g = torch.from_numpy(A.gradient(n, 0)).to(DEV)
    _step(state, g, hyper)  # moments that are not all zero when the capture starts
    eager = [t.clone() for t in state]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _step(warm, g, hyper)  # warm-up off the capture, on buffers of its own
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _step(state, g, hyper)
    assert int(state[3].item()) == 1  # capturing ran nothing
    for k in range(1, 4):
        new = torch.from_numpy(A.gradient(n, k)).to(DEV)
        g.copy_(new)
        graph.replay()
        _step(eager, new, hyper)
    torch.cuda.synchronize()
    assert int(state[3].item()) == int(eager[3].item()) == 4
    for name, a, b in zip(("p", "m", "v", "counter", "scratch"), state, eager):
        assert torch.equal(a, b), name
