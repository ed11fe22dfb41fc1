"""Case builders, the float64 CPU reference and the error bars of the classification loss head (K23), shared by
tests/test_class_loss_host.py, tests/test_gpu_class_loss.py and tests/test_gpu_class_loss_train.py.  No GPU.

The reference is the definition in plain float64 torch on the CPU:
  CE   lp = log_softmax(z_i), p = exp(lp), W = sum_c w_c (w = 1 without weights), A_i = (1 - s) w[y_i], B = s / C
       row_i = -A_i lp[y_i] - B sum_c w_c lp[c];  den = sum_i w[y_i] (mean) or 1 (sum);  loss = scale sum_i row_i / den
       dz[i, c] = scale [A_i (p_c - [c == y_i]) + B (W p_c - w_c)] / den
  BCE  one logit per sample, t_i = y_i (1 - s) + s / 2, softplus(x) = max(x, 0) + log1p(exp(-|x|))
       row_i = pw t_i softplus(-z_i) + (1 - t_i) softplus(z_i);  den = G (mean) or 1 (sum)
       dz[i] = scale [(1 - t_i) sigmoid(z_i) - pw t_i sigmoid(-z_i)] / den

Error bars, from each case's own float64 quantities: u = 2^-24, a_i = max_c |z_ic|, c_i = C + 6 a_i + 12 - recursive summation over
the classes (C), the rounding of z - m and of z - lse carried through expf and into lp (a few a_i u), and expf / logf / the division /
the products (the constant).  An error of c_i u in every lp enters the row with the weights it is multiplied by; the sums over rows
are taken in double and rounded once, and den, scale / den and the final products are a few roundings more (the G + 8 and G + 4
terms are generous for them):
  CE   |loss - ref| <= scale [sum_i c_i u (A_i + B W) + (G + 8) u sum_i |row_i|] / den
       |dz - ref|   <= scale (c_i + 8) u [A_i (p_c + [c == y_i]) + B (W p_c + w_c)] / den + (G + 4) u |ref|
  BCE  the same with C = 2 in c_i (two softplus terms), the weights of the two terms in place of A_i + B W, and the two sigmoid
       terms' magnitudes in place of the bracket:
       |loss - ref| <= scale [sum_i c_i u (pw t_i + 1 - t_i) + (G + 8) u sum_i |row_i|] / den
       |dz - ref|   <= scale (c_i + 8) u [pw t_i sigmoid(-z_i) + (1 - t_i) sigmoid(z_i)] / den + (G + 4) u |ref|
``worst_fractions`` evaluates the CE formulas in plain fp32 torch and reports the largest share of the bars it uses (the host test
prints them: 0.13 of the loss bar and 0.23 of the gradient bar were seen when the bars were set).
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
GS = (1, 3, 64, 65, 1025)          # the one-launch bound, one past it, past one workgroup's rows
CS = (2, 3, 33, 64, 65, 1000)      # a lane per row; a wave per row: below, at and past a wavefront's width, many passes
SEED_CS = (2, 3, 33, 1000)
SCALES = (1, 3, 8)
SMOOTHINGS = (0.0, 0.1)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(5000 + seed)


def ce_case(G: int, C: int, logit_scale: float, weighted: bool):
    """(logits float32 [G, C] = randn * logit_scale, labels int64 [G], weights float32 [C] in [0.2, 1.2) or None), seeded by the shape."""
    g = _gen(G * 7919 + C * 31 + int(logit_scale))
    logits = torch.randn(G, C, generator=g, dtype=torch.float32) * float(logit_scale)
    labels = torch.randint(0, C, (G,), generator=g, dtype=torch.int64)
    weights = (torch.rand(C, generator=g, dtype=torch.float32) + 0.2) if weighted else None
    return logits, labels, weights


def bce_case(G: int, logit_scale: float):
    """(logits float32 [G, 1], labels int64 [G] of 0 / 1)."""
    g = _gen(G * 104729 + int(logit_scale))
    return torch.randn(G, 1, generator=g, dtype=torch.float32) * float(logit_scale), torch.randint(0, 2, (G,), generator=g, dtype=torch.int64)


# ---------------------------------------------------------------------------------------------------------------- reference
def ref_ce(logits, labels, weights=None, s: float = 0.0, reduction: str = "mean", scale: float = 1.0, dtype=torch.float64):
    """dict(loss 0-dim, dz [G, C], rows [G], den, p [G, C], w [C], A [G], B, W) of the definition, evaluated in ``dtype``."""
    z = logits.to(dtype)
    G, C = z.shape
    w = weights.to(dtype) if weights is not None else torch.ones(C, dtype=dtype)
    lp = torch.log_softmax(z, dim=1)
    p = torch.exp(lp)
    W = w.sum()
    A = (1.0 - s) * w[labels]
    B = s / C
    rows = -A * lp[torch.arange(G), labels] - B * (lp * w).sum(1)
    den = w[labels].double().sum() if reduction == "mean" else torch.tensor(1.0, dtype=torch.float64)
    onehot = F.one_hot(labels, C).to(dtype)
    loss = scale * rows.double().sum() / den  # the sums over rows in double, whatever the rows' type
    dz = (scale / den).to(dtype) * (A[:, None] * (p - onehot) + B * (W * p - w))
    return dict(loss=loss, dz=dz, rows=rows, den=den, p=p, w=w, A=A, B=B, W=W, onehot=onehot)


def bars_ce(logits, labels, weights=None, s: float = 0.0, reduction: str = "mean", scale: float = 1.0):
    """(ref, loss_bar 0-dim, dz_bar [G, C]) in float64."""
    r = ref_ce(logits, labels, weights, s, reduction, scale)
    G, C = logits.shape
    c = C + 6.0 * logits.double().abs().max(dim=1).values + 12.0
    k = abs(scale) / r["den"]
    loss_bar = k * ((c * U * (r["A"] + r["B"] * r["W"])).sum() + (G + 8) * U * r["rows"].abs().sum())
    dz_bar = (k * ((c + 8.0) * U)[:, None] * (r["A"][:, None] * (r["p"] + r["onehot"]) + r["B"] * (r["W"] * r["p"] + r["w"]))
              + (G + 4) * U * r["dz"].abs())
    return r, loss_bar, dz_bar


def _softplus(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def ref_bce(logits, labels, pos_weight: float = 1.0, s: float = 0.0, reduction: str = "mean", scale: float = 1.0):
    """dict(loss 0-dim, dz [G, 1], rows [G], den, t [G], z [G]) of the definition in float64."""
    z = logits.double().reshape(-1)
    t = labels.double() * (1.0 - s) + s / 2.0
    rows = pos_weight * t * _softplus(-z) + (1.0 - t) * _softplus(z)
    den = torch.tensor(float(z.numel()) if reduction == "mean" else 1.0, dtype=torch.float64)
    loss = scale * rows.sum() / den
    dz = scale * ((1.0 - t) * torch.sigmoid(z) - pos_weight * t * torch.sigmoid(-z)) / den
    return dict(loss=loss, dz=dz.reshape(-1, 1), rows=rows, den=den, t=t, z=z)


def bars_bce(logits, labels, pos_weight: float = 1.0, s: float = 0.0, reduction: str = "mean", scale: float = 1.0):
    r = ref_bce(logits, labels, pos_weight, s, reduction, scale)
    z, t, G = r["z"], r["t"], logits.size(0)
    c = 2.0 + 6.0 * z.abs() + 12.0
    k = abs(scale) / r["den"]
    loss_bar = k * ((c * U * (pos_weight * t + 1.0 - t)).sum() + (G + 8) * U * r["rows"].abs().sum())
    dz_bar = (k * (c + 8.0) * U * (pos_weight * t * torch.sigmoid(-z) + (1.0 - t) * torch.sigmoid(z))).reshape(-1, 1) \
        + (G + 4) * U * r["dz"].abs()
    return r, loss_bar, dz_bar


# ------------------------------------------------------------------------------------------------------- the seed condition
def worst_fractions():
    """(loss, gradient): the largest |fp32 evaluation - float64 reference| / bar over G x SEED_CS x SCALES x SMOOTHINGS, weighted."""
    worst = [0.0, 0.0]
    for G in GS:
        for C in SEED_CS:
            for logit_scale in SCALES:
                for s in SMOOTHINGS:
                    logits, labels, weights = ce_case(G, C, logit_scale, weighted=True)
                    r, loss_bar, dz_bar = bars_ce(logits, labels, weights, s)
                    got = ref_ce(logits, labels, weights, s, dtype=torch.float32)
                    worst[0] = max(worst[0], float((got["loss"].float().double() - r["loss"]).abs() / loss_bar))
                    worst[1] = max(worst[1], float(((got["dz"].double() - r["dz"]).abs() / dz_bar).max()))
    return tuple(worst)


# ------------------------------------------------------------------------------------------------- one example, by hand
# C = 2.  Row 0: equal logits -> lp = (-ln 2, -ln 2), row = ln 2 whatever the label, and a tie, so the predicted class is 0 while the
# label is 1.  Row 1: z = (0, ln 3) -> p = (1/4, 3/4), label 1 -> row = ln(4/3), predicted class 1.
# mean loss = (ln 2 + ln(4/3)) / 2 = ln(8/3) / 2;  dz = (p - onehot) / 2 = [[1/4, -1/4], [1/8, -1/8]];  counts[1, 0] = counts[1, 1] = 1.
HAND_LOGITS = torch.tensor([[0.7, 0.7], [0.0, 1.0986122886681098]], dtype=torch.float32)
HAND_LABELS = torch.tensor([1, 1], dtype=torch.int64)
HAND_LOSS = 0.4904146265058631  # ln(8/3) / 2
HAND_DZ = torch.tensor([[0.25, -0.25], [0.125, -0.125]], dtype=torch.float64)
HAND_CONFUSION = torch.tensor([[0, 0], [1, 1]], dtype=torch.int64)


def confusion_of(logits, labels, K: int):
    """int64 [K, K], rows = label: ``torch.argmax`` (lowest index on ties) and ``bincount`` on the CPU."""
    if logits.size(1) == 1 and K == 2:
        pred = (logits.reshape(-1) > 0).long()
    else:
        pred = torch.argmax(logits, dim=1)
    return torch.bincount(labels * K + pred, minlength=K * K).view(K, K)
