"""GPU: the loss-head kernel (csrc/class_loss.hip, DESIGN K23) against the float64 reference of tests/class_loss_cases.py within its
error bars - both lane mappings, the one-launch form and the three-launch form - and the properties the trainer relies on: scoring
mode, the counts, the accumulator, the same bits alone and in a batch, one launch in the captured regime, labels outside the classes."""
import pytest
import torch

from tests import class_loss_cases as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_SCALES = (1.0, 0.125)
REDUCTIONS = ("mean", "sum")


def _head(logits, labels, weights=None, **kw):
    """(loss float32 [1], dz float32 [G, C] | None, status int32 [1]) on the CPU; tensors among ``kw`` go to the device."""
    from graphnet_classifier_amd import native
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    z = logits if logits.is_cuda else logits.to(DEV)
    loss, dz = native.class_loss(z, labels.to(DEV), status=status, class_weight=weights.to(DEV) if weights is not None else None, **kw)
    return loss.cpu(), dz.cpu() if dz is not None else None, status.cpu()


def _check(got_loss, got_dz, ref, loss_bar, dz_bar, what):
    loss_err = float((got_loss.double().reshape(()) - ref["loss"]).abs())
    dz_err = (got_dz.double() - ref["dz"]).abs()
    share = (loss_err / float(loss_bar), float((dz_err / dz_bar).max()))
    assert loss_err <= float(loss_bar), (what, "loss", loss_err, float(loss_bar))
    assert bool((dz_err <= dz_bar).all()), (what, "dz", float((dz_err / dz_bar).max()))
    return share


@pytest.mark.parametrize("C", L.CS)
@pytest.mark.parametrize("G", L.GS)
def test_cross_entropy_against_float64_within_the_bars(G, C):
    worst = [0.0, 0.0]
    for logit_scale in L.SCALES:
        for weighted in (False, True):
            logits, labels, weights = L.ce_case(G, C, logit_scale, weighted)
            for s in L.SMOOTHINGS:
                for reduction in REDUCTIONS:
                    for scale in LOSS_SCALES:
                        ref, loss_bar, dz_bar = L.bars_ce(logits, labels, weights, s, reduction, scale)
                        loss, dz, status = _head(logits, labels, weights, label_smoothing=s, reduction=reduction, scale=scale)
                        share = _check(loss, dz, ref, loss_bar, dz_bar, (logit_scale, weighted, s, reduction, scale))
                        worst = [max(a, b) for a, b in zip(worst, share)]
                        assert int(status) == 0
    print(f"G={G} C={C}: {worst[0]:.2f} of the loss bar, {worst[1]:.2f} of the gradient bar")


@pytest.mark.parametrize("G", L.GS)
def test_binary_cross_entropy_against_float64_within_the_bars(G):
    worst = [0.0, 0.0]
    for logit_scale in L.SCALES:
        logits, labels = L.bce_case(G, logit_scale)
        for pw in (1.0, 2.0):
            for s in L.SMOOTHINGS:
                for reduction in REDUCTIONS:
                    for scale in LOSS_SCALES:
                        ref, loss_bar, dz_bar = L.bars_bce(logits, labels, pw, s, reduction, scale)
                        loss, dz, status = _head(logits, labels, kind="bce", pos_weight=pw, label_smoothing=s, reduction=reduction,
                                                 scale=scale)
                        share = _check(loss, dz, ref, loss_bar, dz_bar, (logit_scale, pw, s, reduction, scale))
                        worst = [max(a, b) for a, b in zip(worst, share)]
                        assert int(status) == 0
    print(f"binary G={G}: {worst[0]:.2f} of the loss bar, {worst[1]:.2f} of the gradient bar")


def test_the_hand_written_example():
    confusion = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    loss, dz, _ = _head(L.HAND_LOGITS, L.HAND_LABELS, confusion=confusion)
    assert abs(float(loss) - L.HAND_LOSS) <= 3e-7 and float((dz.double() - L.HAND_DZ).abs().max()) <= 1e-7
    assert torch.equal(confusion.cpu(), L.HAND_CONFUSION)  # the tie goes to class 0
    equal = torch.tensor([[0.7, 0.7]])
    assert abs(float(_head(equal, torch.tensor([0]))[0]) - 0.6931471805599453) <= 3e-7  # ln 2, a few fp32 roundings


@pytest.mark.parametrize("G, C", [(3, 3), (64, 33), (65, 2), (1025, 65)])
def test_a_row_stride_above_the_width_gives_the_bits_of_the_contiguous_rows(G, C):
    logits, labels, weights = L.ce_case(G, C, 3, True)
    wide = torch.full((G, C + 3), float("nan"), device=DEV)
    wide[:, :C] = logits.to(DEV)
    view = wide[:, :C]
    assert not view.is_contiguous()
    a = _head(logits, labels, weights, label_smoothing=0.1)
    b = _head(view, labels, weights, label_smoothing=0.1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("G, C", [(3, 2), (65, 65)])
def test_autograd_through_the_public_wrapper_with_an_upstream_gradient(G, C):
    from graphnet_classifier_amd import functional as Fn
    logits, labels, weights = L.ce_case(G, C, 3, True)
    ref, loss_bar, dz_bar = L.bars_ce(logits, labels, weights, 0.1)
    z = logits.to(DEV).requires_grad_(True)
    loss = Fn.class_loss(z, labels, class_weight=weights.to(DEV), label_smoothing=0.1)
    assert loss.dim() == 0 and loss.requires_grad
    (loss * 2.5).backward()  # the upstream gradient stays on the device
    got = z.grad.cpu().double() / 2.5  # 2.5 x an fp32 value: one more rounding, inside the (G + 4) u |ref| term
    assert float((loss.detach().cpu().double() - ref["loss"]).abs()) <= float(loss_bar)
    assert bool(((got - ref["dz"]).abs() <= dz_bar + L.U * ref["dz"].abs()).all())
    with torch.no_grad():
        scored = Fn.class_loss(z, labels, class_weight=weights.to(DEV), label_smoothing=0.1)
    assert not scored.requires_grad and torch.equal(scored, loss.detach())


def test_the_single_graph_form_of_the_reference():
    from graphnet_classifier_amd import functional as Fn
    logits, labels, weights = L.ce_case(1, 2, 3, True)
    ref, loss_bar, dz_bar = L.bars_ce(logits, labels, weights, 0.1)
    z = logits[0].to(DEV).requires_grad_(True)  # [C] with a 0-dim label (models/GNN.py:338-341)
    loss = Fn.class_loss(z, labels[0].to(DEV), class_weight=weights.to(DEV), label_smoothing=0.1)
    loss.backward()
    assert z.grad.shape == (2,) and float((loss.detach().cpu().double() - ref["loss"]).abs()) <= float(loss_bar)
    assert bool(((z.grad.cpu().double() - ref["dz"][0]).abs() <= dz_bar[0]).all())
    with pytest.raises(ValueError):
        Fn.class_loss(torch.zeros(2, 2, 2, device=DEV), labels)


@pytest.mark.parametrize("G, C", [(64, 2), (65, 2), (64, 65), (1025, 33)])
def test_scoring_mode_returns_the_loss_bits_of_training_mode(G, C):
    logits, labels, weights = L.ce_case(G, C, 3, True)
    trained = _head(logits, labels, weights, label_smoothing=0.1)
    scored = _head(logits, labels, weights, label_smoothing=0.1, with_gradient=False)
    assert scored[1] is None and torch.equal(scored[0], trained[0])
    zb, yb = L.bce_case(G, 3)
    assert torch.equal(_head(zb, yb, kind="bce", pos_weight=2.0)[0], _head(zb, yb, kind="bce", pos_weight=2.0, with_gradient=False)[0])


@pytest.mark.parametrize("G, C", [(64, 3), (65, 3), (64, 65), (65, 130), (1025, 2)])
def test_the_confusion_counts_equal_argmax_and_bincount_and_accumulate(G, C):
    logits, labels, _ = L.ce_case(G, C, 1, False)
    logits[0] = 0.25                      # every class ties: class 0
    if G > 2 and C > 2:
        logits[1] = -1.0
        logits[1, C - 1] = logits[1, 1] = 5.0   # a tie between two classes: the lower one
    if C > 70:
        logits[2] = -1.0
        logits[2, 70] = logits[2, 6] = logits[2, 69] = 4.0  # the same lane's second class, and a neighbour's
    want = L.confusion_of(logits, labels, C)
    confusion = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    _head(logits, labels, confusion=confusion)
    assert torch.equal(confusion.cpu(), want) and int(want.sum()) == G
    _head(logits, labels, confusion=confusion, with_gradient=False)  # scoring counts too
    assert torch.equal(confusion.cpu(), 2 * want)


def test_the_binary_counts_and_a_row_of_nans_stay_inside_the_matrix():
    zb, yb = L.bce_case(65, 3)
    zb[0] = 0.0  # not above zero: class 0
    confusion = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    _head(zb, yb, kind="bce", confusion=confusion)
    assert torch.equal(confusion.cpu(), L.confusion_of(zb, yb, 2))
    for C in (3, 65):
        logits, labels, _ = L.ce_case(5, C, 1, False)
        logits[2] = float("nan")
        confusion = torch.zeros(C, C, dtype=torch.int64, device=DEV)
        _head(logits, labels, confusion=confusion)
        keep = torch.tensor([0, 1, 3, 4])
        rest = confusion.cpu() - L.confusion_of(logits[keep], labels[keep], C)
        assert int(rest.sum()) == 1 and int(rest[labels[2]].sum()) == 1 and int(rest.min()) == 0  # counted once, in its label's row


@pytest.mark.parametrize("G", [3, 65])
def test_the_accumulator_receives_the_returned_loss_exactly(G):
    logits, labels, weights = L.ce_case(G, 3, 3, True)
    acc = torch.zeros((), dtype=torch.float64, device=DEV)
    first = _head(logits, labels, weights, loss_sum=acc)[0]
    assert float(acc) == float(first.double())
    second = _head(logits * 2, labels, weights, loss_sum=acc, scale=0.125, with_gradient=False)[0]
    assert float(acc) == float(first.double() + second.double()) and float(second) != float(first)


@pytest.mark.parametrize("kind, C", [("ce", 3), ("ce", 65), ("ce", 1000), ("bce", 1)])
def test_with_sum_a_row_alone_has_the_bits_of_the_row_in_a_batch(kind, C):
    """A batch of 65 (three launches), of 64 (one launch) and every row alone: the same dlogits bits, and the loss of a row alone is
    the row's own term."""
    if kind == "ce":
        logits, labels, weights = L.ce_case(65, C, 3, True)
        kw = dict(label_smoothing=0.1, reduction="sum", scale=0.125)
    else:
        (logits, labels), weights = L.bce_case(65, 3), None
        kw = dict(kind="bce", pos_weight=2.0, label_smoothing=0.1, reduction="sum", scale=0.125)
    big = _head(logits, labels, weights, **kw)[1]
    small = _head(logits[:64], labels[:64], weights, **kw)[1]
    assert torch.equal(big[:64], small)
    total = 0.0
    for i in (0, 1, 17, 63, 64):
        loss, alone, _ = _head(logits[i:i + 1], labels[i:i + 1], weights, **kw)
        assert torch.equal(alone[0], big[i]), i
        total += float(loss.double())
    pick = torch.tensor([0, 1, 17, 63, 64])
    five = _head(logits[pick], labels[pick], weights, **kw)[0]
    assert abs(float(five.double()) - total) <= 8 * L.U * abs(total)  # five fp32 roundings against one


def test_the_captured_regime_is_one_launch():
    from graphnet_classifier_amd import native
    assert native.class_loss_launches(native.PAD_BATCH_MAX_GRAPHS) == 1 and native.class_loss_launches(65) == 3
    assert native.class_loss_launches(65, with_gradient=False) == 2
    timers = native.KernelTimers()
    native.set_kernel_timers(timers)
    try:
        for G, C in ((1, 2), (64, 2), (64, 1000)):
            logits, labels, weights = L.ce_case(G, C, 1, True)
            confusion = torch.zeros(C, C, dtype=torch.int64, device=DEV)
            acc = torch.zeros((), dtype=torch.float64, device=DEV)
            before = timers.num_launches()
            _head(logits, labels, weights, label_smoothing=0.1, confusion=confusion, loss_sum=acc)  # everything at once
            assert timers.num_launches() - before == 1 and list(timers.events) == ["class_loss"]
    finally:
        native.set_kernel_timers(None)


@pytest.mark.parametrize("kind, G, C", [("ce", 8, 3), ("ce", 70, 3), ("ce", 8, 65), ("ce", 70, 65), ("bce", 8, 1), ("bce", 70, 1)])
def test_labels_outside_the_classes_are_left_out_and_flagged(kind, G, C):
    """The kernel reads a label once, compares it with [0, K) and from then on carries -1 for a bad one: neither the weights nor the
    counts are indexed with it (csrc/class_loss.hip, row_stats / tally)."""
    from graphnet_classifier_amd.loss import ClassificationLoss
    if kind == "ce":
        logits, labels, weights = L.ce_case(G, C, 3, True)
        kw = dict(label_smoothing=0.1)
    else:
        (logits, labels), weights = L.bce_case(G, 3), None
        kw = dict(kind="bce", pos_weight=2.0)
    K = 2 if kind == "bce" else C
    bad = labels.clone()
    bad[1], bad[G - 2] = -1, K
    keep = torch.tensor([i for i in range(G) if i not in (1, G - 2)])
    confusion = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    loss, dz, status = _head(logits, bad, weights, confusion=confusion, **kw)
    want_conf = torch.zeros(K, K, dtype=torch.int64, device=DEV)
    want_loss, want_dz, clean = _head(logits[keep], labels[keep], weights, confusion=want_conf, **kw)
    assert int(status) == 1 and int(clean) == 0
    assert not bool(dz[1].any()) and not bool(dz[G - 2].any())
    ref, loss_bar, dz_bar = (L.bars_ce(logits[keep], labels[keep], weights, 0.1) if kind == "ce"
                             else L.bars_bce(logits[keep], labels[keep], 2.0))
    assert float((loss.double().reshape(()) - ref["loss"]).abs()) <= float(loss_bar)
    assert bool(((dz[keep].double() - ref["dz"]).abs() <= dz_bar).all())
    assert float((loss - want_loss).abs()) <= 4 * L.U * abs(float(want_loss))  # the same terms, summed in double in another order
    assert float((dz[keep] - want_dz).abs().max()) <= 4 * L.U * float(want_dz.abs().max())
    assert torch.equal(confusion, want_conf) and int(confusion.sum()) == G - 2  # the bad rows are not counted
    # every label bad: den == 0, loss and gradient 0
    loss, dz, status = _head(logits, torch.full_like(labels, K), weights, **kw)
    assert float(loss) == 0.0 and not bool(dz.any()) and int(status) == 1
    crit = ClassificationLoss(kind, weights, track_metrics=True, **({"label_smoothing": 0.1} if kind == "ce" else {"pos_weight": 2.0}))
    crit(logits.to(DEV), bad.to(DEV))
    with pytest.raises(IndexError, match=str(K)):
        crit.check()
    crit.check()  # cleared
    assert int(crit.confusion.sum()) == G - 2
