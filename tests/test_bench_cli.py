"""CPU: bench.py's command line. A plain run measures the headline only (every side measurement
is behind --full, where each keeps its own --no-... switch), and --dump-outputs writes the last
timed step's loss and parameters as float32 .npy files within a fixed size."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402

SIDE = ("no_cpu_baseline", "no_roofline", "no_traffic", "no_site_trace", "no_gpu_step")


def test_plain_run_is_the_headline_only():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup, a.full, a.dump_outputs) == (1, 7, 2, False, "")
    assert all(getattr(a, k) for k in SIDE)


def test_full_keeps_every_side_measurement_and_its_switch():
    a = bench.parse(["--full"])
    assert a.full and not any(getattr(a, k) for k in SIDE)
    a = bench.parse(["--full", "--no-traffic", "--dump-outputs", "out"])
    assert a.no_traffic and a.dump_outputs == "out"
    assert not any(getattr(a, k) for k in SIDE if k != "no_traffic")


def test_step_outputs_are_float32_copies():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    model[1].bias.requires_grad_(False)
    out = bench.step_outputs(torch.tensor(1.5, dtype=torch.float64), model)
    assert list(out) == ["loss", "param_00_0_weight", "param_01_0_bias", "param_02_1_weight"]
    assert all(v.dtype == np.float32 for v in out.values())
    assert out["loss"].tolist() == [1.5] and out["param_00_0_weight"].shape == (4, 3)
    before = out["param_00_0_weight"].copy()
    with torch.no_grad():
        model[0].weight.add_(1.0)  # a later pass trains on: the arrays taken earlier stay
    assert np.array_equal(out["param_00_0_weight"], before)


def test_dump_outputs_whole_and_sampled(tmp_path):
    rng = np.random.default_rng(1)
    arrays = {"small": rng.standard_normal((5, 3)), "big": rng.standard_normal(5000).astype(np.float32)}
    bench.dump_outputs(arrays, str(tmp_path / "a"))
    for k, v in arrays.items():
        got = np.load(tmp_path / "a" / (k + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, v.astype(np.float32))
    # over the size limit: the large array becomes a fixed sample, the small one stays whole
    cap = 12000
    for d in ("b", "c"):
        bench.dump_outputs(arrays, str(tmp_path / d), max_bytes=cap)
    files = sorted(os.listdir(tmp_path / "b"))
    assert files == ["big.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in files) <= cap
    big = np.load(tmp_path / "b" / "big.npy")
    assert big.dtype == np.float32 and 0 < big.size < 5000
    assert np.isin(big, arrays["big"]).all()
    assert np.array_equal(big, np.load(tmp_path / "c" / "big.npy"))
    assert np.array_equal(np.load(tmp_path / "b" / "small.npy"), arrays["small"].astype(np.float32))
