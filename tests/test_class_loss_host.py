"""Host side of the loss-head tests (no GPU): the float64 definitions of tests/class_loss_cases.py against ``torch.nn.functional``,
a plain fp32 evaluation inside the bars (the seed condition), the hand-written example, the option checks of ``ClassificationLoss``
and ``train`` and the declaration of the new entry points."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from graphnet_classifier_amd import baseline, native, train as T
from graphnet_classifier_amd.loss import ClassificationLoss, accuracy_of, check_loss_options
from tests import class_loss_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("s", L.SMOOTHINGS)
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_float64_cross_entropy_equals_torch_functional(weighted, s, reduction):
    worst = 0.0
    for G, C in ((1, 2), (3, 3), (65, 33), (17, 1000)):
        logits, labels, weights = L.ce_case(G, C, 3, weighted)
        z = logits.double().requires_grad_(True)
        w64 = weights.double() if weighted else None
        want = F.cross_entropy(z, labels, weight=w64, label_smoothing=s, reduction=reduction)
        (0.125 * want).backward()
        r = L.ref_ce(logits, labels, weights, s, reduction, scale=0.125)
        worst = max(worst, abs(float(r["loss"]) - 0.125 * float(want.detach())) / abs(0.125 * float(want.detach())), float((r["dz"] - z.grad).abs().max()))
    print(f"weighted={weighted} s={s} {reduction}: worst difference {worst:.1e}")
    assert worst <= 1e-12


def test_float64_cross_entropy_takes_the_single_graph_form():
    logits, labels, weights = L.ce_case(1, 2, 3, True)
    want = F.cross_entropy(logits[0].double(), labels[0], weight=weights.double(), label_smoothing=0.1)  # [C] with a 0-dim label
    assert labels[0].dim() == 0 and abs(float(L.ref_ce(logits, labels, weights, 0.1)["loss"]) - float(want)) <= 1e-12


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("pos_weight", [1.0, 2.0])
def test_float64_binary_cross_entropy_equals_torch_functional(pos_weight, reduction):
    for G in (1, 3, 65):
        for s in L.SMOOTHINGS:
            logits, labels = L.bce_case(G, 8)
            z = logits.double().requires_grad_(True)
            target = (labels.double() * (1 - s) + s / 2).reshape(-1, 1)
            want = F.binary_cross_entropy_with_logits(z, target, pos_weight=torch.tensor([pos_weight], dtype=torch.float64),
                                                      reduction=reduction)
            want.backward()
            r = L.ref_bce(logits, labels, pos_weight, s, reduction)
            assert abs(float(r["loss"]) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
            assert float((r["dz"] - z.grad).abs().max()) <= 1e-12


def test_a_plain_fp32_evaluation_stays_inside_the_bars():
    loss_share, grad_share = L.worst_fractions()
    print(f"fp32 torch evaluation: {loss_share:.2f} of the loss bar, {grad_share:.2f} of the gradient bar")
    assert loss_share <= 0.5 and grad_share <= 0.5


def test_the_binary_bars_are_positive_and_scale_with_the_terms():
    logits, labels = L.bce_case(65, 8)
    r, loss_bar, dz_bar = L.bars_bce(logits, labels, 2.0, 0.1)
    assert float(loss_bar) > 0 and bool((dz_bar > 0).all()) and float(loss_bar) <= 1e-4 * float(r["loss"])
    fp32 = L.ref_bce(logits.float(), labels, 2.0, 0.1)  # float64 of the fp32 inputs: the reference itself
    assert float((fp32["loss"] - r["loss"]).abs()) == 0.0


def test_the_hand_written_example():
    r = L.ref_ce(L.HAND_LOGITS, L.HAND_LABELS)
    assert abs(L.HAND_LOSS - math.log(8.0 / 3.0) / 2.0) <= 1e-15
    assert abs(float(r["loss"]) - L.HAND_LOSS) <= 1e-7  # ln 3 is rounded to fp32 in the logits
    assert float((r["dz"] - L.HAND_DZ).abs().max()) <= 1e-7
    assert abs(float(r["rows"][0]) - math.log(2.0)) <= 1e-15  # equal logits
    assert torch.equal(L.confusion_of(L.HAND_LOGITS, L.HAND_LABELS, 2), L.HAND_CONFUSION)  # the tie goes to class 0
    assert accuracy_of(L.HAND_CONFUSION) == 0.5 and accuracy_of(torch.zeros(2, 2, dtype=torch.int64)) == 0.0


BAD_LOSS_OPTIONS = [
    dict(kind="focal"), dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=float("nan")),
    dict(kind="bce", class_weight=[1.0, 2.0]), dict(kind="ce", pos_weight=2.0), dict(class_weight=[1.0, -2.0]),
    dict(kind="bce", pos_weight=-1.0), dict(class_weight=[1.0, float("inf")]), dict(reduction="none"), dict(class_weight=[]),
]


@pytest.mark.parametrize("bad", BAD_LOSS_OPTIONS, ids=str)
def test_bad_loss_options_raise_in_the_constructor(bad):
    with pytest.raises(ValueError):
        check_loss_options(**bad)
    with pytest.raises(ValueError):
        ClassificationLoss(**bad)


def test_a_good_criterion_allocates_nothing_before_its_first_call():
    crit = ClassificationLoss("ce", [1.0, 2.3], 0.05, track_metrics=True)
    assert crit.status is None and crit.confusion is None and crit.class_weight is None and crit.num_classes is None
    assert crit.state_snapshot() == [] and not crit.accumulates_into(torch.zeros((), dtype=torch.float64))
    crit.check()
    crit.reset_metrics()
    with pytest.raises(ValueError):
        crit(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64))  # three classes, two weights: at the first call
    with pytest.raises(ValueError):
        ClassificationLoss("bce")(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64))  # the binary loss takes ONE logit
    with pytest.raises(ValueError):
        crit.bind_loss_sum(torch.zeros(1))
    assert crit.status is None
    ClassificationLoss("bce", pos_weight=2.0, label_smoothing=0.1)
    ClassificationLoss("ce", torch.tensor([1.0, 2.0]), reduction="sum")


BAD_TRAIN_OPTIONS = [
    dict(loss="focal"), dict(loss=3), dict(class_weight=[1.0, 2.0]), dict(label_smoothing=0.1), dict(pos_weight=2.0), dict(metrics=True),
    dict(loss="ce", pos_weight=2.0), dict(loss="bce", class_weight=[1.0, 2.0]), dict(loss="ce", label_smoothing=1.0),
    dict(loss="ce", class_weight=[-1.0, 1.0]), dict(loss=ClassificationLoss("ce"), label_smoothing=0.1),
]


@pytest.mark.parametrize("bad", BAD_TRAIN_OPTIONS, ids=str)
def test_bad_loss_keywords_of_train_raise_before_anything_is_allocated(bad, tmp_path):
    with pytest.raises(ValueError):
        T.train(None, None, 1, output_path=str(tmp_path / "w"), **bad)  # no model, no data: the check comes first
    assert not (tmp_path / "w").exists()
    with pytest.raises(ValueError):
        baseline.train_MLP(epochs=1, output_path=str(tmp_path / "w"), dataset_path=str(tmp_path / "no_such_folder"), **bad)


def test_make_criterion_names_the_reference_loss_by_default():
    assert isinstance(T.make_criterion(), torch.nn.CrossEntropyLoss)
    crit = T.make_criterion("ce", [1.0, 2.3], 0.05, None, True)
    assert isinstance(crit, ClassificationLoss) and crit.track_metrics and crit.label_smoothing == 0.05 and crit.status is None
    mine = ClassificationLoss("bce", pos_weight=2.0)
    assert T.make_criterion(mine, metrics=True) is mine and mine.track_metrics


def test_new_entry_points_are_declared_exported_and_listed_without_an_abi_bump():
    header = open(os.path.join(ROOT, "include", "gnc_hip.h")).read()
    lib = native.load_library()
    for name in ("gnc_class_loss_f32", "gnc_class_loss_launches", "gnc_class_loss_workspace_doubles"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in native._SIGNATURES and name in native.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.gnc_abi_version() == native.ABI_VERSION == 20 and re.search(r"#define GNC_ABI_VERSION 20\b", header)
    assert lib.gnc_class_loss_workspace_doubles() == native.CLASS_LOSS_WORKSPACE_DOUBLES
    assert native.CLASS_LOSS_ONE_LAUNCH_ROWS == native.PAD_BATCH_MAX_GRAPHS == 64  # every captured mini-batch is one launch
    assert re.search(r"#define GNC_CLASS_LOSS_ONE_LAUNCH_ROWS 64\b", header)
    assert [lib.gnc_class_loss_launches(g, 1) for g in (0, 1, 64, 65, 10 ** 6)] == [1, 1, 1, 3, 3]
    assert [lib.gnc_class_loss_launches(g, 0) for g in (64, 65)] == [1, 2]  # scoring: no gradient pass
    makefile = open(os.path.join(ROOT, "graphnet_classifier_amd", "csrc", "Makefile")).read()
    assert "class_loss.hip" in re.search(r"^SRCS\s*=\s*(.+)$", makefile, re.M).group(1).split()
    assert native.LOSS_KINDS == {"ce": 0, "bce": 1} and native.LOSS_REDUCTIONS == {"mean": 0, "sum": 1}
    for enum in (r"GNC_LOSS_CE = 0, GNC_LOSS_BCE = 1", r"GNC_LOSS_MEAN = 0, GNC_LOSS_SUM = 1"):
        assert enum in header


def test_the_library_rejects_bad_arguments_without_a_device():
    lib = native.load_library()
    one = 8  # a non-null, aligned stand-in: the argument checks come before any launch

    def call(**kw):
        a = dict(logits=one, ld=2, labels=one, weight=None, G=4, C=2, kind=0, s=0.0, pw=1.0, reduction=0, scale=1.0, loss=one, dz=None,
                 ld_dz=2, loss_sum=None, confusion=None, status=one, workspace=None)
        a.update(kw)
        return lib.gnc_class_loss_f32(a["logits"], a["ld"], a["labels"], a["weight"], a["G"], a["C"], a["kind"], a["s"], a["pw"],
                                      a["reduction"], a["scale"], a["loss"], a["dz"], a["ld_dz"], a["loss_sum"], a["confusion"],
                                      a["status"], a["workspace"], None)

    for bad in (dict(C=0), dict(kind=2), dict(reduction=2), dict(s=1.0), dict(s=float("nan")), dict(scale=float("inf")),
                dict(kind=1, C=2), dict(kind=1, C=1, weight=one), dict(kind=1, C=1, pw=-1.0), dict(status=None), dict(loss=None),
                dict(ld=1), dict(dz=one, ld_dz=1), dict(G=65), dict(G=-1), dict(logits=6)):
        assert call(**bad) != 0, bad
        assert lib.gnc_last_error_string()
