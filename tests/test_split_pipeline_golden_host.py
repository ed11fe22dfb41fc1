"""Host-side checks of the fixtures of tests/test_gpu_split_pipeline_bits.py (tests/golden/split_pipeline/): they load, their
shapes and digests agree with split_pipeline.json, and they were not recorded from the commit under test."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import test_gpu_split_pipeline_bits as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(m.GOLDEN, "split_pipeline.json")) as f:
        return json.load(f)


def test_every_case_has_its_fixture(meta):
    assert sorted(meta["cases"]) == sorted(f"{name}/{rows}" for name, rows in m.KEYS)
    assert meta["row_step"] == m.ROW_STEP and meta["whole_below"] == m.WHOLE_BELOW
    for name, rows in m.KEYS:
        path = m.fixture_path(name, rows)
        assert os.path.getsize(path) < 1 << 20, path
        want = meta["cases"][f"{name}/{rows}"]
        with np.load(path) as z:
            assert sorted(z.files) == sorted(k for k in want if k not in m.TWINS)
            for twin, of in m.TWINS.items():  # recorded from the parent: its twins agreed bit for bit
                assert twin not in want or (want[twin]["sha256"] == want[of]["sha256"] and want[twin]["shape"] == want[of]["shape"])
            for k in z.files:
                a, shape = z[k], want[k]["shape"]
                assert a.dtype == np.float32 and np.isfinite(a).all()
                assert re.fullmatch(r"[0-9a-f]{64}", want[k]["sha256"])
                if shape[0] < m.WHOLE_BELOW:  # stored whole: the digest can be checked here
                    assert list(a.shape) == shape
                    assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == want[k]["sha256"]
                else:
                    assert list(a.shape) == [(shape[0] + m.ROW_STEP - 1) // m.ROW_STEP] + shape[1:]
        # both row counts of a case hold the same tensors' first dimension = the case's rows (aggregates: its nodes)
        assert want["out" if "out" in want else "out_a"]["shape"][0] == rows


def test_recorded_commit_is_not_head(meta):
    assert re.fullmatch(r"[0-9a-f]{7,40}", meta["commit"])
    assert "GNC_LIB_PATH=" in meta["command"] and meta["library"] != os.path.join("graphnet_classifier_amd", "libgnc_hip.so")
    r = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    if r.returncode != 0 or not r.stdout.strip():
        return  # an exported tree without history has no HEAD to compare with
    dirty = subprocess.run(["git", "status", "--porcelain", "--", "graphnet_classifier_amd/csrc"], cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.DEVNULL, text=True).stdout.strip()
    if not dirty:  # (with uncommitted kernel sources HEAD is still the parent the work in progress is compared against)
        head = r.stdout.strip()
        assert not head.startswith(meta["commit"]) and not meta["commit"].startswith(head)
