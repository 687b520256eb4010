"""The steady solve's stop logic and its operations past one pass, on the CPU
backend: the twins of tests/test_gpu_steady_control.py, which runs the same
bodies (tests/_steady_control.py) on gfx950.

A. the solver against a host-driven replica of its loop, bit for bit: caps
   around the polling interval, an uncapped run that stops between two polls,
   a second solve on a capped one's result;
B. the exits of the outer loop: already solved, non-finite fields, restarts,
   solving twice (a finished call never reports "running");
C. the shapes at which the gfx950 kernels take a second pass (here: their
   premises and the CPU definitions on those shapes);
D. the value classes of tests/_value_fields.py through the three operations."""
import pytest

import _steady_cases as sc
import _steady_control as ct
import _value_fields as vf

CPU = "cpu"


def test_the_solver_exposes_the_bits_of_D(h3d):
    """The replica takes D and dt from Solver.physics; the ops-level cases take
    sc.physics_D: the same bits on every box used here."""
    for N in (ct.BOX, ct.SOLVED, ct.LONG_ROWS, ct.STRIDED):
        assert tuple(sc.physics_D(h3d, N)) == tuple(h3d.native().physics(*N)["D"])
    s, _, _ = ct.start(h3d, "dirichlet", CPU)
    assert tuple(s.native.physics["D"]) == tuple(sc.physics_D(h3d, ct.BOX))


# ---- A ----------------------------------------------------------------------------
@pytest.mark.parametrize("cap", ct.CAPS)
@pytest.mark.parametrize("form", ["dirichlet", "mixed"])
def test_replica_capped(h3d, form, cap):
    ct.check_capped(h3d, CPU, form, cap)


@pytest.mark.parametrize("form", ["dirichlet", "mixed"])
def test_replica_stops_between_two_polls(h3d, form):
    ct.check_uncapped(h3d, CPU, form)


@pytest.mark.parametrize("form", ["dirichlet", "mixed"])
def test_replica_second_solve_on_a_capped_one(h3d, form):
    ct.check_two_calls(h3d, CPU, form)


# ---- B ----------------------------------------------------------------------------
def test_already_solved(h3d):
    ct.check_already_solved(h3d, CPU)


@pytest.mark.parametrize("kind", list(vf.KINDS) + ["huge"])
def test_nonfinite_field_is_a_breakdown(h3d, kind):
    ct.check_nonfinite(h3d, CPU, kind)


@pytest.mark.parametrize("case", list(ct.RESTART_CASES), ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-{c[3]}")
def test_restart(h3d, case):
    ct.check_restart(h3d, CPU, case)


def test_restarts_exhausted(h3d):
    ct.check_restarts_exhausted(h3d, CPU)


@pytest.mark.parametrize("name", ["reference33", "layered", "convective_slab"])
def test_solving_twice(h3d, name):
    ct.check_solving_twice(h3d, CPU, name)


# ---- C ----------------------------------------------------------------------------
def test_past_one_pass_premises(h3d):
    assert set(ct.past_one_pass_cases(h3d.native())) == {"long_rows", "strided", "strided_free", "strided_xplus"}


@pytest.mark.parametrize("residual", [False, True], ids=["A", "residual"])
@pytest.mark.parametrize("form", ["uniform", "conductivity_walls"])
@pytest.mark.parametrize("name", ["long_rows", "strided", "strided_free", "strided_xplus"])
def test_past_one_pass(h3d, name, form, residual):
    """The CPU definitions on the shapes of C: the fsum bound on the long rows
    and for one form of the 2.5 M-point box."""
    ct.check_past_one_pass(h3d, CPU, name, form, residual,
                           exact=name == "long_rows" or (name == "strided" and form == "uniform" and not residual))


# ---- D ----------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(sc.FORMS))
@pytest.mark.parametrize("cls", vf.CLASSES)
def test_value_classes_apply(h3d, cls, form):
    ct.check_value_apply(h3d, CPU, cls, form)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("cls", vf.CLASSES)
def test_value_classes_update_and_direction(h3d, cls, sign):
    ct.check_value_update(h3d, CPU, cls, sign)


@pytest.mark.parametrize("residual", [False, True], ids=["A", "residual"])
@pytest.mark.parametrize("form", ["walls", "conductivity_walls"])
def test_wall_vertices_may_hold_anything(h3d, form, residual):
    ct.check_wall_vertices_may_hold_anything(h3d, CPU, form, residual)


@pytest.mark.parametrize("residual", [False, True], ids=["A", "residual"])
@pytest.mark.parametrize("form", ["uniform", "conductivity_walls"])
@pytest.mark.parametrize("kind", list(vf.KINDS))
def test_one_spike(h3d, kind, form, residual):
    ct.check_one_spike(h3d, CPU, kind, form, residual)
