"""bench.py's plain run and --dump-outputs: the steps it times are the steps asked for, and what the last step computed
is written as float64 arrays from a fixed sample, the same from run to run.  The sample and the byte budget are checked
on the CPU with a stand-in batch; the GPU test runs the benchmark itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Stats:
    pairs = 4321


class _FakeBatch:
    """result(i) as cpecan_batch_result hands it over: int32 (score, x, y) rows, `rows(i)` of them."""

    def __init__(self, rows):
        self.rows = rows

    def result(self, i):
        n = self.rows(i)
        return np.stack([np.full(n, 1000 + i), np.arange(n), np.arange(n) + i % 3], axis=1).astype(np.int32)

    def stats(self):
        return _Stats()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_sample_is_fixed_float64_and_matches_the_lists(tmp_path):
    mine = np.arange(10000) + 7
    batch = _FakeBatch(lambda i: 50 + i % 11)
    names = bench.dump_outputs(str(tmp_path / "a"), batch, mine, None)
    bench.dump_outputs(str(tmp_path / "b"), batch, mine, None)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == names
    for k in a:
        assert a[k].dtype == np.float64
        assert np.array_equal(a[k], b[k])
    idx = a["sample_problems"].astype(np.int64) - 7
    assert len(idx) == bench.DUMP_MAX_PROBLEMS and np.all(np.diff(idx) > 0)
    lens = a["sample_list_lengths"].astype(np.int64)
    assert lens.tolist() == [50 + i % 11 for i in idx]
    assert a["aligned_pairs"].shape == (lens.sum(), 3)
    first = batch.result(int(idx[0]))
    assert np.array_equal(a["aligned_pairs"][:lens[0]], first.astype(np.float64))
    assert a["batch_pairs_emitted"].tolist() == [4321.0]


def test_dump_stays_inside_the_byte_budget(tmp_path):
    bench.dump_outputs(str(tmp_path), _FakeBatch(lambda i: 40000), np.arange(5000), None)
    total = sum(os.path.getsize(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path)))
    assert 0 < total <= 64 << 20
    got = _load(str(tmp_path))
    assert got["aligned_pairs"].shape[0] == got["sample_list_lengths"].sum() > 0


def test_dump_of_the_expectation_step(tmp_path):
    from cpecan_amd import api
    acc = api.hmm_constructEmpty(0.5, api.threeState)
    acc.likelihood = -12.25
    bench.dump_outputs(str(tmp_path), None, None, acc)
    got = _load(str(tmp_path))
    assert got["expectation_transitions"].shape == (9,) and got["expectation_emissions"].shape == (48,)
    assert got["expectation_likelihood"].tolist() == [-12.25]
    assert np.array_equal(got["expectation_transitions"], np.array(acc.transitions[:9]))


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 2 and "--steps" in out.stderr


def _plain_run(dump_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "A", "--steps", "3",
                          "--warmup", "1", "--dump-outputs", dump_dir], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_same_outputs_twice(tmp_path):
    one, two = _plain_run(str(tmp_path / "one")), _plain_run(str(tmp_path / "two"))
    for line in (one, two):
        assert line["steps"] == 3 and line["warmup"] == 1
        assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "cells/s"
        # the plain run measures the headline only; the rest is --full's
        assert line["value_e2e"] is None
        assert not any(k in line for k in ("cpu_baseline", "parity_spot_check", "other_configs"))
    a, b = _load(str(tmp_path / "one")), _load(str(tmp_path / "two"))
    assert sorted(a) == ["aligned_pairs", "batch_pairs_emitted", "sample_list_lengths", "sample_problems"]
    for k in a:
        assert a[k].dtype == np.float64
        assert np.array_equal(a[k], b[k]), k
    assert a["aligned_pairs"].shape[0] == a["sample_list_lengths"].sum() > 0
    assert a["batch_pairs_emitted"][0] == one["e2e"]["pairs_emitted"]
