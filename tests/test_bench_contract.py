"""CPU checks of the benchmark contract: `python bench.py --gpus N` starts its N ranks itself (one child, torch.distributed.run on
127.0.0.1, nothing touches the GPU in the parent), and the committed JSON line of the round carries every field the driver reads.
On the GPU: what `--dump-outputs DIR` writes is the last timed step's result on the seeded inputs."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_gpus_n_spawns_the_ranks_as_a_child(monkeypatch):
    import subprocess

    import bench
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert exc.value.code == 7                                    # the child's exit code is passed on
    cmd = seen["cmd"]
    assert cmd[0] == sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert os.path.basename(cmd[cmd.index("--master-port") + 2]) == "bench.py"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def test_committed_bench_line_has_the_contract_fields():
    path = os.path.join(ROOT, "profiles", "r02_bench.json")
    if not os.path.exists(path):
        pytest.skip("no committed round-2 bench line yet")
    d = json.loads(open(path).read().strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert r["solve"]["bound"] == "hbm" and 0 < r["solve"]["frac"] < 1
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["unit"] == d["unit"]
    assert d["parity"]["inertia_equal"] and d["parity"]["sign_D_equal"] and d["parity"]["rel_err_x"] <= d["parity"]["tolerance_x"]
    assert abs(d["value"] - d["n_gpus"] * d["steps"] / (d["ms_per_step"] * d["steps"] / 1e3)) < 1e-6 * d["value"]


def test_steps_below_one_are_refused_before_any_work(monkeypatch):
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert exc.value.code == 2                                    # argparse's usage error: ms_per_step needs a timed step


def test_dump_outputs_writes_float64_npy_files_within_the_limit(tmp_path):
    import numpy as np

    import bench
    bench.dump_outputs(str(tmp_path / "out"), {"x": np.arange(4, dtype=np.float32), "flag": [1]}, suffix="_rank2")
    assert sorted(os.listdir(tmp_path / "out")) == ["flag_rank2.npy", "x_rank2.npy"]
    x = np.load(tmp_path / "out" / "x_rank2.npy")
    assert x.dtype == np.float64 and x.tolist() == [0.0, 1.0, 2.0, 3.0]
    assert np.load(tmp_path / "out" / "flag_rank2.npy").tolist() == [1.0]
    assert bench.DUMP_LIMIT_BYTES == 64 << 20
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(9)}, limit=64)
    assert not (tmp_path / "big").exists()


@pytest.mark.gpu
def test_dump_outputs_hold_the_last_timed_step(tmp_path):
    import subprocess

    import numpy as np

    from onephase_jl_amd import synth
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "S-small", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
           "--no-kkt-level", "--no-live-pmc", "--no-sharded-model", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path)) == ["d.npy", "flag.npy", "inertia.npy", "x.npy"]
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(a.dtype == np.float64 for a in got.values())
    # rank 0's seeded inputs, rebuilt here: the dumped x solves that system
    prob = synth.make_config("S-small", seed=0)
    n, m = prob["n"], prob["m"]
    M = synth.symmetrize_lower(synth.augmented_matrix(prob, delta=1e-8))
    rhs = np.random.default_rng(1234).normal(size=n + m)
    assert got["x"].shape == got["d"].shape == (n + m,)
    assert np.max(np.abs(M @ got["x"] - rhs)) <= 1e-8 * np.max(np.abs(rhs))
    assert got["inertia"].tolist() == [n, m, 0, 0] and got["flag"].tolist() == [1]
    assert np.sum(got["d"] > 0) == n and np.sum(got["d"] < 0) == m


def test_a_plain_run_is_the_default_and_the_other_legs_need_full():
    import bench
    plain = bench.arg_parser().parse_args([])
    assert plain.full is False
    assert not (plain.no_cpu_baseline or plain.no_kkt_level or plain.no_live_pmc or plain.no_sharded_model)
    assert bench.arg_parser().parse_args(["--full"]).full is True


# what only --full adds to the line: measurements and checks beside the headline figure
FULL_ONLY_KEYS = ("cpu_baseline", "parity", "vs_cpu_port", "sharded")
FULL_ONLY_CONFIG_KEYS = ("kkt_level", "sharded_model", "sharded")


@pytest.mark.gpu
def test_plain_run_spends_little_outside_its_steps():
    import subprocess
    import time
    steps, warmup = 2, 1
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "config", "roofline"):
        assert k in d, k
    assert d["steps"] == steps and d["warmup"] == warmup and d["config"]["inertia_ok"]
    assert abs(d["value"] - d["steps"] / (d["ms_per_step"] * d["steps"] / 1e3)) < 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY_KEYS if k in d] and not [k for k in FULL_ONLY_CONFIG_KEYS if k in d["config"]]
    assert "batch4" not in d["roofline"]["solve"] and d["roofline"]["traffic_detail"]["source"].startswith("committed summary")
    outside = wall - (steps + warmup) * d["ms_per_step"] / 1e3
    assert outside < 30.0, f"{outside:.1f} s outside the warm-up and timed steps"


@pytest.mark.gpu
def test_full_run_adds_the_other_legs():
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "S-small", "--cpu-sample", "S-small", "--steps", "2", "--warmup", "1",
           "--full", "--no-live-pmc", "--no-sharded-model"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["config"]["inertia_ok"]
    b4 = d["roofline"]["solve"]["batch4"]
    assert b4["ms"] > 0 and b4["ms_per_rhs"] == b4["ms"] / 4
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == d["unit"] and c["value"] > 0 and c["ports_agree"] and "step_side_port" in c
    assert d["parity"]["inertia_equal"] and d["parity"]["sign_D_equal"] and d["parity"]["rel_err_x"] <= d["parity"]["tolerance_x"]
    assert d["vs_cpu_port"]["ratio"] > 0
    assert set(d["config"]["kkt_level"]) >= {"symmetric", "schur", "step_side"}
    assert "sharded_model" not in d["config"] and "sharded" not in d      # skipped on request
