"""bench.py's command line: a plain run does only what the headline figure
needs, ``--full`` adds the phase profile and the time-to-converge run, and
``--dump-outputs`` writes what the timed steps computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench


class _StubSolver:
    def __init__(self, field):
        self.field = field

    def gather(self):
        return self.field


def test_parse_args_plain_and_full():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2) and a.full is False and a.dump_outputs == ""
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(tmp_path):
    state = {"iter": 25, "last_residual": 0.125, "norm": 3.5}
    small = np.arange(5 * 6 * 7, dtype=np.float64).reshape(5, 6, 7)
    info = bench.dump_outputs(str(tmp_path / "a"), _StubSolver(small), state)
    assert info["field_sampled"] is False and info["files"] == ["field.npy", "state.npy"]
    f = np.load(tmp_path / "a" / "field.npy")
    assert f.dtype == np.float64 and np.array_equal(f, small)
    assert np.array_equal(np.load(tmp_path / "a" / "state.npy"), [25.0, 0.125, 3.5])
    # one value past the whole-field limit: a fixed sample, the same points every time
    n = bench.DUMP_FIELD_BYTES // 8 + 1
    big = np.arange(n, dtype=np.float64).reshape(1, 1, n)
    for d in ("b", "c"):
        info = bench.dump_outputs(str(tmp_path / d), _StubSolver(big), state)
        assert info["field_sampled"] is True and info["field_values"] == bench.DUMP_FIELD_BYTES // 8
    b, c = np.load(tmp_path / "b" / "field.npy"), np.load(tmp_path / "c" / "field.npy")
    assert b.dtype == np.float64 and b.nbytes == bench.DUMP_FIELD_BYTES <= 64e6 and np.array_equal(b, c)
    # the values are their own flat indices here: in range, sorted, spread over the field
    assert b[0] >= 0 and b[-1] < n and np.all(np.diff(b) >= 0) and b[-1] - b[0] > 0.99 * n
    # a rank that is not the root (gather gives None) writes nothing
    assert bench.dump_outputs(str(tmp_path / "e"), _StubSolver(None), state) is None
    assert not (tmp_path / "e").exists()


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_timed_field(h3d, gpu, tmp_path):
    """A plain ``bench.py --gpus 1`` run: --steps timed steps after --warmup,
    no time-to-converge run and no phase profile, and field.npy is bit for bit
    the field of a solver stepped warmup + steps times."""
    n, steps, warm = 65, 7, 3
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--grid", str(n),
                        "--steps", str(steps), "--warmup", str(warm), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=110, cwd=ROOT,
                       env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    j = json.loads(lines[0])
    assert j["steps"] == steps and j["warmup"] == warm and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "GLUPS" and j["higher_is_better"] is True and j["dtype"] == "fp64"
    assert j["full"] is False and j["time_to_converge"] is None and j["phases"] == [{"rank": 0}]
    assert sorted(os.listdir(tmp_path / "out")) == ["field.npy", "state.npy"]
    s = h3d.HeatSolver((n, n, n), 1 << 40, 0.0, backend="hip", device=0)
    s.step(warm)
    s.step(steps)
    s.synchronize()
    st = s.state()
    field = np.load(tmp_path / "out" / "field.npy")
    assert field.dtype == np.float64 and np.array_equal(field, s.gather())
    assert np.array_equal(np.load(tmp_path / "out" / "state.npy"),
                          [warm + steps, st["last_residual"], st["norm"]])
