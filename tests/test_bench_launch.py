"""bench.py --gpus N: the rank plan and the launch wiring (CPU; no rank touches the GPU under
--launch-check).  The driver's scaling run calls `python bench.py --gpus N` or launches the ranks
itself with torch.distributed.run; both must end with N ranks, and a WORLD_SIZE that disagrees with
--gpus must fail instead of reporting a rank count that did not run.  Also the options of a plain
run (--steps, --full off by default) and the --dump-outputs writer."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_rank_plan():
    assert bench.rank_plan(None, {}) == ("run", 1)
    assert bench.rank_plan(1, {}) == ("run", 1)
    assert bench.rank_plan(2, {}) == ("launch", 2)
    assert bench.rank_plan(8, {}) == ("launch", 8)
    assert bench.rank_plan(None, {"WORLD_SIZE": "4"}) == ("run", 4)
    assert bench.rank_plan(4, {"WORLD_SIZE": "4"}) == ("run", 4)
    with pytest.raises(SystemExit):
        bench.rank_plan(2, {"WORLD_SIZE": "4"})
    with pytest.raises(SystemExit):
        bench.rank_plan(0, {})


def test_launch_cmd_is_the_drivers_form():
    cmd = bench.launch_cmd(4, ["--gpus", "4", "--steps", "3"], 29600)
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--master-addr=127.0.0.1" in cmd and "--master-port=29600" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    assert cmd[cmd.index("--master-port=29600") + 1].endswith("bench.py")


def _run(args, extra_env=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=180)


def test_gpus_2_launches_two_ranks():
    r = _run(["--gpus", "2", "--launch-check"])
    assert r.returncode == 0, r.stderr
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    assert sorted(d["rank"] for d in lines) == [0, 1]
    assert all(d["world"] == 2 for d in lines)
    assert sorted(d["local_rank"] for d in lines) == [0, 1]
    assert all(d["master"].startswith("127.0.0.1:") for d in lines)


def test_gpus_1_runs_in_process():
    r = _run(["--launch-check"])
    assert r.returncode == 0, r.stderr
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    assert lines == [{"rank": 0, "world": 1, "local_rank": 0, "master": "None:None"}]


def test_world_size_mismatch_fails():
    r = _run(["--gpus", "2", "--launch-check"], {"WORLD_SIZE": "3", "RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=3" in r.stderr


def test_native_selfcheck_keeps_or_drops_the_native_exchange():
    """bench._native_selfcheck: the native communicator stays only if every rank's comparison with the
    torch.distributed exchange passed; a mismatch or an exception closes it and reports why (a
    one-rank gloo group in this process stands in for the ranks)."""
    import socket

    import torch.distributed as dist

    class Fake:
        closed = False

        def close(self):
            self.closed = True

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    own = not dist.is_initialized()
    if own:
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        f = Fake()
        kept, note = bench._native_selfcheck(f, dist, "cpu", lambda: True, "payload")
        assert kept is f and not f.closed and note.startswith("native == torch.distributed")
        f = Fake()
        kept, note = bench._native_selfcheck(f, dist, "cpu", lambda: False, "payload")
        assert kept is None and f.closed and "torch.distributed exchange used" in note

        def boom():
            raise RuntimeError("collective timed out")

        f = Fake()
        kept, note = bench._native_selfcheck(f, dist, "cpu", boom, "payload")
        assert kept is None and f.closed and "collective timed out" in note
    finally:
        if own:
            dist.destroy_process_group()


def test_full_is_off_by_default_and_steps_are_the_timed_steps():
    """A plain run does only what the headline needs: --full is an option, off by default; --steps is
    the number of timed steps (c1 / c3: search iterations, unless --iterations says otherwise)."""
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d" and a.steps == 20
    assert bench.parse(["--config", "c1", "--steps", "3"]).iterations == 3
    assert bench.parse(["--config", "c3", "--steps", "3", "--iterations", "2"]).iterations == 2
    assert bench.parse(["--config", "c1"]).iterations == 0  # (bench_search's own default)


def test_dump_outputs_writes_float_arrays(tmp_path):
    """--dump-outputs: one .npy per array; float64 stays, everything else becomes float32; every file is
    finite -- a floating-point output's non-finite entries are 0 in <name>.npy and classed in
    <name>_nonfinite.npy (1 +Inf, 2 -Inf, 3 NaN), the two files together restoring it exactly; an output
    past 2^20 elements is a fixed, seeded sample (the same elements from run to run, and in both of its files)."""
    import numpy as np

    big = np.arange(3 << 20, dtype=np.float64)
    big[::5] = np.inf
    arrays = {"losses": np.array([1.5, np.inf, np.nan, -np.inf, -0.25]), "did_succeed": np.array([True, False, True]),
              "fcalls": np.array([3, 4], np.int64), "big": big}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["big.npy", "big_nonfinite.npy", "did_succeed.npy", "fcalls.npy", "losses.npy",
                           "losses_nonfinite.npy"]
    assert all(np.all(np.isfinite(a)) and a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["losses.npy"].dtype == np.float64 and got["losses.npy"].tolist() == [1.5, 0.0, 0.0, 0.0, -0.25]
    assert got["losses_nonfinite.npy"].tolist() == [0.0, 1.0, 3.0, 2.0, 0.0]
    back = got["losses.npy"].copy()
    for code, v in ((1, np.inf), (2, -np.inf), (3, np.nan)):
        back[got["losses_nonfinite.npy"] == code] = v
    assert back.tobytes() == arrays["losses"].tobytes()
    assert got["did_succeed.npy"].dtype == np.float32 and got["did_succeed.npy"].tolist() == [1.0, 0.0, 1.0]
    assert got["fcalls.npy"].dtype == np.float32 and got["fcalls.npy"].tolist() == [3.0, 4.0]
    assert got["big.npy"].dtype == np.float64 and got["big.npy"].shape == got["big_nonfinite.npy"].shape == (1 << 20,)
    fin = got["big_nonfinite.npy"] == 0  # a sample of big's own elements, in order; every fifth was +Inf
    assert np.all(np.diff(got["big.npy"][fin]) > 0) and np.all(got["big.npy"][fin] % 5 != 0)
    assert np.all(got["big.npy"][~fin] == 0) and np.all(got["big_nonfinite.npy"][~fin] == 1)
    assert 0.15 < np.mean(~fin) < 0.25
    assert got["big.npy"].tobytes() == np.load(tmp_path / "b" / "big.npy").tobytes()
