"""Host side of the controlled-optimizer tests (no GPU): the float64 definitions of tests/optimizer_control_cases.py against
torch.optim in float64 under ``clip_grad_norm_`` and ``LambdaLR``, the fp32 emulations within the fractions the cases module
quotes, ``lr_at``'s end points, the option checks of ``train`` and the declaration of the new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from graphnet_classifier_amd import baseline, native, train as T
from tests import adam_cases as A
from tests import optimizer_control_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM_COSINE = dict(kind="cosine", warmup_steps=4, total_steps=20, min_lr=1e-5)  # 25 steps: warm-up, decay, five held steps


def _torch_optimizer(name, param, wd):
    rule, mu, nesterov = C.RULES[name]
    if rule == "adamw":
        return torch.optim.AdamW([param], lr=C.LR, betas=C.BETAS, eps=C.EPS, weight_decay=wd, foreach=False)
    if rule == "adam":
        return torch.optim.Adam([param], lr=C.LR, betas=C.BETAS, eps=C.EPS, weight_decay=wd, foreach=False)
    return torch.optim.SGD([param], lr=C.LR, momentum=mu, nesterov=nesterov, weight_decay=wd, foreach=False)


@pytest.mark.parametrize("max_norm", [None, 0.5], ids=["noclip", "clip"])
@pytest.mark.parametrize("name", ["adamw", "adam", "sgd_momentum", "sgd_nesterov"])
def test_float64_definitions_equal_torch_optim_under_clipping_and_a_schedule(name, max_norm):
    n, steps, wd = 4099, 25, 0.01
    param = torch.nn.Parameter(torch.from_numpy(A.params(n)).double())
    opt = _torch_optimizer(name, param, wd)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: C.lr_at(e + 1, C.LR, **WARM_COSINE) / C.LR)
    state = tuple(a.astype(np.float64) for a in C.initial_state(name, n))
    bitten = 0
    for s in range(steps):
        g = A.gradient(n, s).astype(np.float64)
        param.grad = torch.from_numpy(g.copy())
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_([param], max_norm)
            bitten += float(total) > max_norm
        opt.step()
        sched.step()
        state = C.step64(name, state, g, s + 1, C.lr_at(s + 1, C.LR, **WARM_COSINE), wd, max_norm)
    want = param.detach().numpy()
    worst = np.abs(state[0] - want).max() / np.abs(want).max()
    print(f"{name} max_norm={max_norm}: max|p - p_torch| / max|p| = {worst:.1e}")
    assert worst <= 1e-13
    assert max_norm is None or bitten >= steps - 5  # the clip is not idle


@pytest.mark.parametrize("name", list(C.RULES))
def test_fp32_emulations_stay_within_the_quoted_fractions_and_their_bars(name):
    worst = C.worst_fractions(name)
    assert worst[0] <= 1e-6 and all(w <= 3e-7 for w in worst[1:]), worst
    for wd in C.WDS:
        for clip, max_norm in C.CLIPS.items():
            for n in C.SIZES:
                for t, lr_t, g, state, out in C.run_fp32(name, n, wd, max_norm):
                    ref, bar, err = C.bars(name, state, g, t, lr_t, wd, max_norm)
                    for k in range(len(state)):
                        assert out[k].dtype == np.float32 and np.isfinite(out[k]).all()
                        assert (np.abs(out[k].astype(np.float64) - ref[k]) <= bar[k]).all()
                        assert (bar[k] >= A.BAR_FACTOR * A.ulp(ref[k])).all()
                    if n >= 1023 and clip != "noclip":
                        assert (C.clip_coef64(g, max_norm) < 1.0) == (clip == "bites")
                    dead = (g == 0) & (state[0] == 0) if wd else (g == 0)
                    for a in state[1:]:
                        dead = dead & (a == 0)
                    if wd == 0:
                        assert dead[::7].all()  # FlatParameters' padding: zero gradient and state stay as they are, bit for bit
                    assert all(np.array_equal(o[dead].view(np.uint32), i[dead].view(np.uint32)) for o, i in zip(out, state))


def test_lr_at_end_points_and_the_library_form():
    lr, w, total = 1e-3, 10, 50
    cos = dict(kind="cosine", warmup_steps=w, total_steps=total, min_lr=1e-6)
    assert C.lr_at(1, lr, **cos) == lr * (1.0 / 10.0) and C.lr_at(w, lr, **cos) == lr  # the warm-up's first step and its end
    assert C.lr_at(w + 1, lr, **cos) < lr and C.lr_at(w + 1, lr, **cos) > 0.99 * lr
    assert abs(C.lr_at((w + total) // 2, lr, **cos) - (1e-6 + 0.5 * (lr - 1e-6))) < 1e-18  # half way down
    assert C.lr_at(total - 1, lr, **cos) > 1e-6
    assert C.lr_at(total, lr, **cos) == C.lr_at(total + 5, lr, **cos) == C.lr_at(10 ** 6, lr, **cos) == 1e-6  # reached, and held
    step = dict(kind="step", warmup_steps=w, gamma=0.5, every=7)
    assert C.lr_at(w + 6, lr, **step) == lr and C.lr_at(w + 7, lr, **step) == lr * 0.5  # the boundary is the 7th step past the warm-up
    assert C.lr_at(w + 13, lr, **step) == lr * 0.5 and C.lr_at(w + 14, lr, **step) == lr * 0.25
    assert C.lr_at(5, lr, **step) == lr * (5.0 / 10.0)
    assert C.lr_at(1, lr) == C.lr_at(10 ** 6, lr) == lr and C.lr_at(3, lr, warmup_steps=4) == lr * (3.0 / 4.0)
    for sched in C.TICK_SCHEDULES + (C.SCHEDULE, WARM_COSINE, {}):
        for t in C.TICK_STEPS + tuple(range(1, 70)):
            assert T.lr_at(t, lr, **sched) == C.lr_at(t, lr, **sched), (sched, t)  # the same doubles, not merely close
    with pytest.raises(ValueError):
        T.lr_at(3, lr, kind="linear")


BAD_OPTIONS = [
    dict(optimizer="adagrad"), dict(optimizer="adam", momentum=0.9), dict(optimizer="adamw", nesterov=True),
    dict(optimizer="sgd", nesterov=True), dict(optimizer="sgd", momentum=-0.1), dict(weight_decay=-1e-2), dict(lr=-1e-3),
    dict(lr=float("nan")), dict(optimizer="adamw", lr=1.0, weight_decay=1.0), dict(max_grad_norm=0.0),
    dict(max_grad_norm=float("inf")), dict(lr_schedule="cosine"), dict(lr_schedule=dict(kind="linear")),
    dict(lr_schedule=dict(kind="cosine", warmup_steps=10, total_steps=10)), dict(lr_schedule=dict(kind="cosine", total_steps=9, min_lr=1.0)),
    dict(lr_schedule=dict(kind="step", every=0)), dict(lr_schedule=dict(kind="step", gamma=0.0)),
    dict(lr_schedule=dict(warmup_steps=-1)), dict(lr_schedule=dict(warmup_steps=2.5)), dict(lr_schedule=dict(kind="constant", warmup=3)),
]


@pytest.mark.parametrize("bad", BAD_OPTIONS, ids=str)
def test_unknown_names_and_inconsistent_values_raise_before_anything_is_allocated(bad, tmp_path):
    with pytest.raises(ValueError):
        T.check_optimizer_options(**bad)
    with pytest.raises(ValueError):
        T.train(None, None, 1, output_path=str(tmp_path / "w"), **bad)  # no model, no data: the check comes first
    assert not (tmp_path / "w").exists()
    with pytest.raises(ValueError):
        baseline.train_MLP(epochs=1, output_path=str(tmp_path / "w"), dataset_path=str(tmp_path / "no_such_folder"), **bad)


def test_good_options_pass_and_the_schedule_comes_back_as_lr_at_keywords():
    assert T.check_optimizer_options() == dict(kind="constant", warmup_steps=0, total_steps=0, min_lr=0.0, gamma=0.1, every=1)
    sched = T.check_optimizer_options("sgd", 0.1, 1e-4, 0.9, True, 1.0, dict(kind="cosine", warmup_steps=3, total_steps=30))
    assert sched["kind"] == "cosine" and T.lr_at(3, 0.1, **sched) == 0.1 and T.lr_at(30, 0.1, **sched) == 0.0
    T.check_optimizer_options("adamw", 1e-3, 0.05, max_grad_norm=1.0, lr_schedule=dict(kind="step", gamma=0.5, every=100))
    with pytest.raises(ValueError):
        baseline.train_MLP(epochs=1, batch=8)  # not a training control
    with pytest.raises(ValueError):
        native.opt_ctl("adagrad", 1e-3)
    c = native.opt_ctl("adamw", 1e-3, weight_decay=0.01, max_grad_norm=2.0, schedule="cosine", warmup_steps=3, total_steps=9)
    assert (c.rule, c.schedule, c.clip, c.check_nonfinite, c.max_grad_norm) == (1, 1, 1, 1, 2.0)  # clipping implies the check
    assert native.opt_ctl("sgd", 1e-2, check_nonfinite=True).clip == 0


def test_new_entry_points_are_declared_exported_and_listed_without_an_abi_bump():
    header = open(os.path.join(ROOT, "include", "gnc_hip.h")).read()
    lib = native.load_library()
    for name in ("gnc_grad_sumsq_f32", "gnc_optimizer_ctl_step_f32", "gnc_sizeof_opt_ctl", "gnc_grad_norm_pass", "gnc_grad_norm_blocks"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in native._SIGNATURES and name in native.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.gnc_abi_version() == native.ABI_VERSION == 20 and re.search(r"#define GNC_ABI_VERSION 20\b", header)
    assert lib.gnc_sizeof_opt_ctl() == ctypes.sizeof(native.OptCtl)
    assert lib.gnc_grad_norm_pass() == native.GRAD_NORM_PASS == native.GRAD_NORM_BLOCKS * 256 * 4
    assert lib.gnc_grad_norm_blocks() == native.GRAD_NORM_BLOCKS
    fields = [f[0] for f in native.OptCtl._fields_]
    struct = re.search(r"typedef struct gnc_opt_ctl_t \{(.*?)\} gnc_opt_ctl_t;", header, re.S).group(1)
    declared = re.findall(r"\b([a-z_0-9]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    assert declared == fields  # the ctypes mirror has the header's fields in the header's order
    makefile = open(os.path.join(ROOT, "graphnet_classifier_amd", "csrc", "Makefile")).read()
    assert "optimizer_ctl.hip" in re.search(r"^SRCS\s*=\s*(.+)$", makefile, re.M).group(1).split()
    assert native.OPT_SCALARS == 8
