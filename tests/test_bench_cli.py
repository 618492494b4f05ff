"""bench.py command line: a plain run prints the headline result line only,
``--full`` adds the finalReward golden check, ``--dump-outputs`` writes the
last timed step's outputs reproducibly (tiny model on CPU)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
         "--model", "tiny-debug", "--seq-len", "256", "--device", "cpu", *extra],
        cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_identical_outputs(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "a"))
    full = _bench("--full", "--dump-outputs", str(tmp_path / "b"))

    for d in (plain, full):
        assert d["metric"].startswith("APO iterations/sec")
        assert d["unit"] == "iterations/s" and d["higher_is_better"] is True
        assert d["dtype"] == "bf16" and d["steps"] == 3 and d["warmup"] == 1
        assert d["ms_per_step"] > 0
        # value and ms_per_step describe the same timed steps
        assert d["value"] * d["ms_per_step"] == pytest.approx(1000.0, rel=1e-9)
    # the golden reward check runs (and is reported) only behind --full
    assert "final_reward_100spans" not in plain["config"]
    assert full["config"]["final_reward_100spans"] == 0.49500000000000005

    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["beam_topk.npy", "scores.npy", "sequence_logprobs.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == names
    for n in names:
        a = np.load(tmp_path / "a" / n)
        b = np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64
        assert np.isfinite(a).all()
        assert np.array_equal(a, b), n  # seeded inputs: run-to-run identical
    assert np.load(tmp_path / "a" / "scores.npy").shape == (16,)
    assert np.load(tmp_path / "a" / "sequence_logprobs.npy").shape == (64,)
    assert np.load(tmp_path / "a" / "beam_topk.npy").tolist() == plain["config"]["beam_topk"]

