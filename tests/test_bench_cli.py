"""bench.py's command line: a plain run prints the headline line only (every side leg is behind
--full), --steps sets the timed steps, and --dump-outputs writes the last timed step's outputs,
which a second run with the same arguments reproduces bit for bit."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import bench

FULL_ONLY = ("graph_replay", "side_configs", "obs_reward_fuse", "path_a", "cpu_baseline")


def test_full_and_dump_outputs_are_off_by_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


class _CountingEnv:
    fused = True

    def __init__(self):
        self.k = 0

    def step(self, actions, out=None):
        self.k += 1
        n = len(actions)
        return ({"obs": torch.full((n, 3), float(self.k))}, torch.full((n,), self.k + 0.5),
                torch.full((n,), self.k % 2, dtype=torch.int64), {})


def test_loop_keeps_what_the_last_step_returned(tmp_path):
    env = _CountingEnv()
    loop = bench.ShardLoop(env, [torch.zeros(5, 2)] * 4)
    win = loop.window(0, 7)
    assert env.k == 7 and win["gathers"] == 0
    got = bench.last_outputs(loop)
    assert {k: (v.dtype, v.shape) for k, v in got.items()} == {
        "obs": (np.float32, (5, 3)), "rew": (np.float32, (5,)), "resets": (np.float32, (5,))}
    assert (got["obs"] == 7).all() and (got["rew"] == 7.5).all() and (got["resets"] == 1).all()
    bench.dump_outputs(str(tmp_path), got, seed=42)
    assert sorted(os.listdir(tmp_path)) == ["obs.npy", "resets.npy", "rew.npy"]
    for k, v in got.items():
        np.testing.assert_array_equal(np.load(tmp_path / f"{k}.npy"), v)


def test_dump_outputs_samples_rows_past_the_size_bound(tmp_path, monkeypatch):
    n = 1000
    arrays = {"obs": np.arange(n * 4, dtype=np.float32).reshape(n, 4), "rew": np.arange(n, dtype=np.float32)}
    monkeypatch.setattr(bench, "DUMP_BYTES", 2000)      # 20 B per row: 100 rows fit
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, seed=3)
    obs, rew = np.load(tmp_path / "a" / "obs.npy"), np.load(tmp_path / "a" / "rew.npy")
    assert obs.shape == (100, 4) and rew.shape == (100,) and obs.nbytes + rew.nbytes <= 2000
    assert (np.diff(rew) > 0).all()                      # distinct rows, ascending
    np.testing.assert_array_equal(obs, arrays["obs"][rew.astype(int)])   # the same rows of every array
    np.testing.assert_array_equal(obs, np.load(tmp_path / "b" / "obs.npy"))
    # two ranks share the bound; rank 1 writes under its own names
    bench.dump_outputs(str(tmp_path / "c"), arrays, seed=3, rank=1, world=2)
    assert np.load(tmp_path / "c" / "rew_rank1.npy").shape == (50,)


def _run_main(monkeypatch, capsys, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TORCHELASTIC_RUN_ID", raising=False)
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_reproducible_dump(gpu, tmp_path, monkeypatch, capsys):
    argv = ["--gpus", "1", "--steps", "6", "--warmup", "3", "--task", "Ant", "--num-envs", "192"]
    outs = []
    for d in ("a", "b"):
        line = _run_main(monkeypatch, capsys, [*argv, "--dump-outputs", str(tmp_path / d)])
        assert not [k for k in FULL_ONLY if k in line]
        assert line["steps"] == 6 and line["warmup"] == 3 and line["unit"] == "env-steps/s"
        assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["nan_resets"] == 0
        # value is env-steps per second of the timed window, ms_per_step that window over its steps
        # (both rounded in the line: ms_per_step to 1e-4 ms, value to 0.1)
        ms = line["ms_per_step"]
        assert ms > 0
        assert line["value"] == pytest.approx(192 / (ms * 1e-3), rel=6e-5 / ms + 1e-6)
        assert line["roofline"]["kernel_ms"] > 0
        outs.append({k: np.load(tmp_path / d / f"{k}.npy") for k in ("obs", "rew", "resets")})
    a, b = outs
    assert a["obs"].shape == (192, 60) and a["rew"].shape == (192,) and a["resets"].shape == (192,)
    assert all(v.dtype == np.float32 for v in a.values())
    assert np.isfinite(a["obs"]).all() and a["obs"].std() > 0 and a["rew"].std() > 0
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
