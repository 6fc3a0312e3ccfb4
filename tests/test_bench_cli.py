"""bench.py's command line (no GPU): a plain run keeps the headline alone, --full restores every
leg at its default, --dump-outputs writes the timed loop's latents as float32."""
import sys

import numpy as np
import torch

import bench

LEGS = ("config4_steps", "config5_steps", "legs_steps", "train_steps", "sharded_T", "png_steps", "cpu_steps")


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_times_the_headline_alone(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2", "--train-steps", "10", "--cpu-steps", "5")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert all(getattr(a, k) == 0 for k in LEGS)
    assert a.e2e is False and a.no_profile is True


def test_full_keeps_every_leg(monkeypatch):
    a = _parse(monkeypatch, "--full", "--steps", "7", "--cpu-steps", "2")
    assert a.full and a.steps == 7 and a.cpu_steps == 2
    assert all(getattr(a, k) > 0 for k in LEGS)
    assert a.e2e is True and a.no_profile is False


def test_dump_outputs_writes_float32(tmp_path):
    x = torch.arange(2 * 4 * 3 * 3, dtype=torch.float32).reshape(2, 4, 3, 3)
    bench.dump_outputs(str(tmp_path / "d"), x, 1, 0)
    bench.dump_outputs(str(tmp_path / "d"), x, 2, 1)
    got = np.load(tmp_path / "d" / "latents.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.numpy())
    assert (tmp_path / "d" / "latents_rank1.npy").exists()
