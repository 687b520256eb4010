"""The --implicit flag of the heat3d CLI: its report, its JSON block, its conflicts."""
import json

import numpy as np

from conftest import run_cli


def test_cli(h3d, heat3d_bin, tmp_path):
    out = tmp_path / "r.json"
    N = (17, 19, 21)
    rc = h3d.HeatEquation3D(N).layered_capacity(1.0, 8.0)
    rc.astype("<f8").tofile(tmp_path / "rc.bin")
    p = run_cli([*N, 3, "1e-8", "--implicit", "64:0.5", "--backend", "cpu", "--capacity", tmp_path / "rc.bin",
                 "--heat-balance", "--json-out", out], tmp_path)
    assert p.returncode == 0, p.stderr
    assert "Implicit steps (theta = 0.5, conjugate gradients): 3 of 3 steps of 64 explicit steps each" in p.stdout, p.stdout
    assert "heat3d: implicit: status=converged" in p.stdout
    doc = json.loads(out.read_text())
    j = doc["implicit"]
    assert j["converged"] is True and j["steps_done"] == 3 and j["steps"] == 3 and j["status"] == "converged"
    assert j["m"] == 64.0 and j["theta"] == 0.5 and j["time_advanced"] == 192.0 and j["tol"] == 1e-8
    assert len(j["step_iterations"]) == 3 and sum(j["step_iterations"]) == j["iterations"] > 0
    assert j["true_residual"] <= 1e-8
    for key in ("residual", "r0_norm", "seconds", "restarts"):
        assert key in j
    assert doc["has_capacity"] is True and doc["heat_balance"]["capacity"] is True
    # the Python interface takes the same road
    s = h3d.HeatSolver(N, 3, 1e-8, backend="cpu", dtype="fp64")
    s.initialize()
    s.set_capacity(rc)
    r = s.step_implicit(3, 64.0, 0.5, tol=1e-8)
    assert r["step_iterations"] == j["step_iterations"] and r["true_residual"] == j["true_residual"]
    assert s.heat_balance()["heat"] == doc["heat_balance"]["heat"]
    # THETA defaults to 1
    p = run_cli([9, 9, 9, 2, "1e-8", "--implicit", "16", "--backend", "cpu", "--json-out", out], tmp_path)
    assert p.returncode == 0 and json.loads(out.read_text())["implicit"]["theta"] == 1.0
    assert "--implicit M[:THETA]" in run_cli(["--help"], tmp_path).stdout
    for bad in (["--dtype", "fp32"], ["--compat"], ["--steady-solve"]):
        q = run_cli([9, 9, 9, 2, "1e-8", "--implicit", "16", "--backend", "cpu"] + bad, tmp_path)
        assert q.returncode != 0 and "--implicit" in q.stderr, (bad, q.stderr)
    for spec in ("0", "-4", "16:0.4", "16:1.5", "nan", "16:x"):
        q = run_cli([9, 9, 9, 2, "1e-8", "--implicit", spec, "--backend", "cpu"], tmp_path)
        assert q.returncode != 0, spec
    q = run_cli([9, 9, 9, 2, "0", "--implicit", "16", "--backend", "cpu"], tmp_path)
    assert q.returncode != 0
    assert np.isfinite(j["r0_norm"])
