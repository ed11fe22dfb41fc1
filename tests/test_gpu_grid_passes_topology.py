"""GPU, kernel level: the general path of gnc_topology_build (fb_sort_all of csrc/topology_build.hip) with MORE than 4096 edges
per block.  fb_geom gives one block per 4096 edges up to min(2 x CUs, 512) co-resident blocks; beyond E = 4096 x that many the
chunk of a block grows past 4096 and each of its 64 threads sorts more than 64 keys per radix pass.  The case of
tests/test_gpu_kernels.py::test_topology_build_matches_stable_sort that comes closest (E = 1,000,003) stays at 245 blocks of
4,082 edges.  N = 70,001 needs 17 key bits: three 8-bit radix passes.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_topology_general_path_with_more_than_4096_edges_per_block():
    from graphnet_classifier_amd import native
    native.load_library()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = min(2 * cus, 512)
    e, n = 4096 * blocks + 4097, 70001
    chunk = -(-e // blocks)  # fb_geom: edges per block, and consecutive keys per thread of its one wave
    assert -(-e // 4096) > blocks and chunk > 4096 and -(-chunk // 64) > 64
    assert 2 ** 16 < n <= 2 ** 24  # three radix passes of 8 bits
    rng = np.random.default_rng(4097)
    src, dst = rng.integers(0, n, size=e).astype(np.int64), rng.integers(0, n, size=e).astype(np.int64)  # not graph-ordered
    order = np.argsort(dst, kind="stable")
    ref_rowptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=n))]).astype(np.int32)
    want = [torch.from_numpy(a).to(DEV) for a in (ref_rowptr, order.astype(np.int32), src[order].astype(np.int32),
                                                  dst[order].astype(np.int32))]
    src_dev, dst_dev = torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV)
    first = None
    for _ in range(2):  # int64 ids with endpoints, twice: the same bits
        rowptr, perm, ss, ds, status = native.topology_build(src_dev, dst_dev, n, gated_fallback=True)
        assert status.tolist() == [0, 0, 1]
        for got, ref, name in zip((rowptr, perm, ss, ds), want, ("rowptr", "perm", "src_sorted", "dst_sorted")):
            assert torch.equal(got, ref), f"{name}: {int((got != ref).sum())} of {ref.numel()} entries differ"
        first = first or (rowptr, perm)
    dst32 = torch.from_numpy(dst.astype(np.int32)).to(DEV)
    for _ in range(2):  # int32 ids, no endpoints (the source-sorted CSR of the backward)
        rp2, pm2, s2, d2, st2 = native.topology_build(None, dst32, n, gated_fallback=True)
        assert s2 is None and d2 is None and st2.tolist() == [0, 0, 1]
        assert torch.equal(rp2, first[0]) and torch.equal(pm2, first[1])
