"""Host side of the fused-Adam tests (no GPU): ``adam64`` of tests/adam_cases.py against float64 torch.optim.Adam, the inputs'
stated properties, the fp32 emulation of ``adam_one`` within the bars the GPU test holds the kernel to, the tick scalars, and
the double-precision entry point's declaration."""
import math
import os
import re

import numpy as np
import pytest
import torch

from graphnet_classifier_amd import native
from tests import adam_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("hyper", A.HYPER, ids=A.hyper_id)
def test_adam64_equals_torch_optim_adam_float64(hyper):
    wd, (b1, b2) = hyper
    n = 1027
    param = torch.nn.Parameter(torch.from_numpy(A.params(n)).double())
    opt = torch.optim.Adam([param], lr=A.LR, betas=(b1, b2), eps=A.EPS, weight_decay=wd, foreach=False)
    p, m, v = A.params(n).astype(np.float64), np.zeros(n), np.zeros(n)
    for s in range(5):
        g = A.gradient(n, s).astype(np.float64)
        param.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = A.adam64(p, g, m, v, s + 1, A.LR, b1, b2, A.EPS, wd)
        state = opt.state[param]
        for got, want in ((p, param.detach()), (m, state["exp_avg"]), (v, state["exp_avg_sq"])):
            want = want.numpy()
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), s
        assert int(state["step"]) == s + 1


def test_gradients_follow_the_recipe():
    n = 4099
    for s in range(A.STEPS):
        g = A.gradient(n, s)
        assert g.dtype == np.float32 and g.shape == (n,)
        assert not g[::7].any() and np.count_nonzero(g) == n - len(g[::7])  # every 7th exactly 0, nothing else
        live = np.abs(g[g != 0]).astype(np.float64)
        assert A.G_MIN <= live.min() and live.max() <= A.G_MAX
        assert 0.9 < live.std() / 10.0 ** (s % 5 - 3) / 0.6 < 1.1  # std of |N(0, 1)| is 0.603
    assert not np.array_equal(A.gradient(n, 0), A.gradient(n, 5))  # same scale, other draws
    p = A.params(n)
    assert p.dtype == np.float32 and abs(float(p.std()) - 1.0) < 0.05


@pytest.mark.parametrize("hyper", A.HYPER, ids=A.hyper_id)
def test_fp32_emulation_meets_the_bars(hyper):
    """The bars contain the emulation by construction (4 x its own error); what is asserted on top is that they are one step's
    fp32 rounding and nothing wider: the figures of the cases module's docstring."""
    wd, (b1, b2) = hyper
    worst = [0.0, 0.0, 0.0]
    for n in A.SIZES:
        for t, (p, g, m, v), out in A.run_fp32(n, hyper):
            ref, bar, err = A.bars(p, g, m, v, t, A.LR, b1, b2, A.EPS, wd)
            for k in range(3):
                assert out[k].dtype == np.float32 and np.isfinite(out[k]).all()
                assert (np.abs(out[k].astype(np.float64) - ref[k]) <= bar[k]).all()
                assert (bar[k] >= A.BAR_FACTOR * A.ulp(ref[k])).all() and (bar[k] >= A.BAR_FACTOR * err[k]).all()
            dead = (g == 0) & (m == 0) & (v == 0)
            if wd == 0:
                assert dead[::7].all() and all(np.array_equal(o[dead], i[dead]) for o, i in zip(out, (p, m, v)))
            worst = [max(a, b) for a, b in zip(worst, A.operand_fractions(p, g, m, v, ref, err, wd))]
    assert worst[0] <= (2e-5 if wd else 1e-6) and worst[1] <= 2e-7 and worst[2] <= 2e-7, worst


def test_tick_scalars_are_torch_optim_adams():
    """torch.optim.Adam (single tensor): step_size = lr / (1 - beta1 ** step), bias_correction2_sqrt = (1 - beta2 ** step) ** 0.5,
    in Python floats; both reach the fp32 kernels rounded once."""
    for b1, b2 in ((0.9, 0.999), (0.5, 0.9)):
        for t in A.TICK_STEPS:
            ss, bc = A.tick_scalars(t, A.LR, b1, b2)
            assert ss == np.float32(A.LR / (1 - b1 ** t)) and bc == np.float32((1 - b2 ** t) ** 0.5)
            assert ss.dtype == np.float32 and bc.dtype == np.float32
    # what rounding the hyper-parameters to fp32 first would cost: more than the one ulp the GPU test allows
    t, b1 = 1, float(np.float32(0.9))
    off = abs(float(np.float32(float(np.float32(A.LR)) / (1 - b1 ** t))) - float(A.tick_scalars(t, A.LR, 0.9, 0.999)[0]))
    assert off > float(np.spacing(A.tick_scalars(t, A.LR, 0.9, 0.999)[0]))
    b2 = float(np.float32(0.999))
    off = abs(math.sqrt(1 - b2 ** 1000) - math.sqrt(1 - 0.999 ** 1000))
    assert off > 10 * float(np.spacing(np.float32(math.sqrt(1 - 0.999 ** 1000))))


def test_double_precision_entry_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "gnc_hip.h")).read()
    lib = native.load_library()
    for name in ("gnc_adam_step_f32", "gnc_adam_step_hp64_f32"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in native._SIGNATURES and hasattr(lib, name), name
    import ctypes
    assert native._SIGNATURES["gnc_adam_step_hp64_f32"][1][5:8] == [ctypes.c_double] * 3
    assert native._SIGNATURES["gnc_adam_step_f32"][1][5:8] == [ctypes.c_float] * 3
    assert lib.gnc_abi_version() == native.ABI_VERSION  # added without an ABI bump
