"""Times of the image-MLP baseline with its first Linear on the split-K kernels K16 (csrc/wide_linear.hip) and with
``GNC_NO_WIDE_LINEAR=1`` (the row-tiled fused-MLP kernels, the path of the parent commit), same process, the two legs interleaved call by
call: median of 40 calls after 10 warm-up calls, HIP events around the call.

  (a) the first Linear alone, forward and forward + backward (route off: a single-Linear K4 launch, gnc_xty_f32 for dW0 / db0);
  (b) the whole ``MLP(3 R R, 2, hidden_layers=L)``, forward and forward + backward;
  (c) one optimizer step (forward, cross-entropy, backward, pack, fused Adam), eager and replayed from a hipGraph;
  (d) ``train()`` for 3 epochs on the 19 photos of tests/golden/g12_image_mlp.npz at R = 128, batch_size = 8: seconds per image of
      the last epoch (decode, resize, ToTensor and the steps), next to the reference's logged 0.30-0.40 min/epoch (unknown CPU and
      dataset size: context, not a comparison).

Prints one JSON line per shape and writes them to the file given as the first argument.  ``--rows 8,64,512`` changes the batch sizes.

    python tools/bench_image_mlp.py profiles/image_mlp.json
"""
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graphnet_classifier_amd import native  # noqa: E402
from graphnet_classifier_amd.MLP import MLP  # noqa: E402
from graphnet_classifier_amd.train import CapturedTensorStep, FlatParameters, FusedAdam, train  # noqa: E402

DEV = "cuda:0"
SWITCH = "GNC_NO_WIDE_LINEAR"


def leg(on: bool):
    if on:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = "1"


def timed_pair(fn_on, fn_off, warmup=10, reps=40):
    """(median microseconds with the route, without it): the two legs alternate call by call"""
    ms = {True: [], False: []}
    for i in range(warmup + reps):
        for on, fn in ((True, fn_on), (False, fn_off)):
            leg(on)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms[on].append(a.elapsed_time(b))
    leg(True)
    return round(statistics.median(ms[True]) * 1e3, 1), round(statistics.median(ms[False]) * 1e3, 1)


def first_linear(rows, K, H=128):
    x = torch.rand(rows, K, device=DEV)
    lin = torch.nn.Linear(K, H).to(DEV)
    w, b = lin.weight.detach(), lin.bias.detach()
    g = torch.randn(rows, H, device=DEV)

    def on_fwd():
        return native.wide_linear_forward(x, w, b, "ReLU")[0]

    def off_fwd():
        return native.mlp_forward([(x, None)], [w], [b], activation="Identity")

    def on_both():
        native.wide_linear_backward(g, on_fwd(), x, "ReLU")

    def off_both():
        off_fwd()
        native.xty(g, x)
    return timed_pair(on_fwd, off_fwd), timed_pair(on_both, off_both)


def whole_mlp(rows, K, layers):
    torch.manual_seed(0)
    model = MLP(K, 2, hidden_layers=layers)
    x = torch.rand(rows, K, device=DEV)
    g = torch.randn(rows, 2, device=DEV)

    def fwd():
        with torch.no_grad():
            model(x)

    def both():
        for p in model.parameters():
            p.grad = None
        model(x).backward(g)
    return timed_pair(fwd, fwd), timed_pair(both, both)


def optimizer_step(rows, K, layers):
    out = {}
    x = torch.rand(rows, K, device=DEV)
    y = torch.randint(0, 2, (rows,), device=DEV)
    steps = {}
    for on in (True, False):
        leg(on)
        torch.manual_seed(0)
        model = MLP(K, 2, hidden_layers=layers)
        opt = FusedAdam(FlatParameters(model), lr=1e-3)
        crit = torch.nn.CrossEntropyLoss()
        loss_sum = torch.zeros((), dtype=torch.float64, device=DEV)

        def eager(model=model, opt=opt, crit=crit):
            loss = crit(model(x), y)
            opt.zero_grad()
            loss.backward()
            opt.step()
        captured = CapturedTensorStep(model, opt, crit, x, y, loss_sum)  # records under this leg's setting
        steps[on] = (eager, lambda captured=captured: captured(x, y))
    leg(True)
    out["eager"] = timed_pair(steps[True][0], steps[False][0])
    out["captured"] = timed_pair(steps[True][1], steps[False][1])
    return out


def epoch_time(side=128):
    import numpy as np
    from PIL import Image
    from graphnet_classifier_amd.dataset import ImageTensorFolder
    g = np.load(os.path.join(ROOT, "tests", "golden", "g12_image_mlp.npz"))
    with tempfile.TemporaryDirectory() as tmp:
        for i, label in enumerate(g["labels"]):
            d = os.path.join(tmp, "data", f"class{int(label)}")
            os.makedirs(d, exist_ok=True)
            Image.fromarray(g[f"photo_{i:02d}"]).save(os.path.join(d, f"img{i:02d}.png"))
        ds = ImageTensorFolder(os.path.join(tmp, "data"), side)
        torch.manual_seed(0)
        model = MLP(3 * side * side, 2)
        stamps = []

        class Stamped:
            def __iter__(self):
                stamps.append(time.time())
                yield from ds.loader(batch_size=8)
        train(model, Stamped(), 3, output_path=os.path.join(tmp, "weights"))
        torch.cuda.synchronize()
        stamps.append(time.time())
    return {"images": len(ds), "epoch_s": [round(b - a, 4) for a, b in zip(stamps, stamps[1:])],
            "last_epoch_ms_per_image": round((stamps[-1] - stamps[-2]) / len(ds) * 1e3, 3)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows_list = [8, 64]
    for a in sys.argv[1:]:
        if a.startswith("--rows"):
            rows_list = [int(v) for v in a.split("=", 1)[1].split(",")]
    rows = []
    for side in (64, 128):
        K = 3 * side * side
        for B in rows_list:
            (f_on, f_off), (fb_on, fb_off) = first_linear(B, K)
            row = {"B": B, "R": side, "K": K, "linear_fwd_us": [f_on, f_off], "linear_fwd_bwd_us": [fb_on, fb_off]}
            for layers in (2, 5):
                (m_on, m_off), (mb_on, mb_off) = whole_mlp(B, K, layers)
                row[f"mlp_L{layers}_fwd_us"], row[f"mlp_L{layers}_fwd_bwd_us"] = [m_on, m_off], [mb_on, mb_off]
                st = optimizer_step(B, K, layers)
                row[f"step_L{layers}_eager_us"], row[f"step_L{layers}_captured_us"] = list(st["eager"]), list(st["captured"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    ep = {"epoch_R128_B8": epoch_time()}
    rows.append(ep)
    print(json.dumps(ep), flush=True)
    if args:
        with open(args[0], "w") as fh:
            json.dump({"columns": "[route on, GNC_NO_WIDE_LINEAR=1] median microseconds", "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
