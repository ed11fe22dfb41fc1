"""Shared by the GPU tests of a capture's buffer lifetimes.  A hipGraph holds the ADDRESSES of the buffers it read while it was
recorded: one that the capture object does not keep alive goes back to the allocator, the next small allocation lands on it, and
from then on a replay reads those bytes.  The first replay straight after construction cannot show that; replays with unrelated
allocations between them can."""
import torch

from tests._util import max_abs

DEV = "cuda:0"


def allocate_between_replays(held, k, other_model, other_sample):
    """Unrelated small device allocations, all kept alive in ``held``: eight small int64 tensors (the size of an offsets buffer)
    and an eager forward of another model."""
    held.extend(torch.full((2,), 7 + k + j, dtype=torch.int64, device=DEV) for j in range(8))
    with torch.no_grad():
        held.append(other_model(other_sample))


def replay_between_allocations(capture, sample, want, other_model, other_sample, what):
    """Four replays of a fixed-topology ``CapturedForward`` with ``allocate_between_replays`` (and a clone of the logits) between
    them, each within the bar of ``want``, and the same bits among themselves."""
    held = []
    for k in range(4):
        got = capture(sample[0], sample[1])
        print(f"{what}, fixed topology, replay {k}: |captured - eager sized| = {max_abs(got, want):.3e}")
        assert max_abs(got, want) <= 1e-5, k
        held.append(got.clone())
        allocate_between_replays(held, k, other_model, other_sample)
    assert all(torch.equal(held[0], h) for h in held[10::10])  # the replays among themselves: the same bits
