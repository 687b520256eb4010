"""The steady solve's stop logic and its kernels past one pass on gfx950
(csrc/kernels/steady_cg.hip, csrc/runtime/solver_steady.cpp): the bodies of
tests/_steady_control.py on the HIP backend; tests/test_steady_control_cpu.py
runs the same ones on the CPU backend.

A. the solver against a host-driven replica of its loop made of the same
   kernels, bit for bit: a kernel that ignored the stop flag between two polls,
   or read alpha / beta from the wrong place, fails here;
B. the exits of the outer loop (a finished call never reports "running");
C. the strided paths of the kernels (more tasks than workgroups, more rows than
   waves, more than one round of a row, more partials than threads) against the
   CPU definitions, bitwise;
D. NaN, Inf, subnormals, signed zeros and overflow through the three
   operations against the CPU definitions, bitwise; NaN at the wall vertices
   that the operator does not read.

Non-finite values are ordinary numbers in in-bounds arrays here."""
import pytest

import _steady_cases as sc
import _steady_control as ct
import _value_fields as vf

pytestmark = pytest.mark.gpu

HIP = "hip"


# ---- A ----------------------------------------------------------------------------
@pytest.mark.parametrize("cap", ct.CAPS)
@pytest.mark.parametrize("form", ["dirichlet", "mixed"])
def test_replica_capped(h3d, gpu, form, cap):
    ct.check_capped(h3d, HIP, form, cap)


@pytest.mark.parametrize("form", ["dirichlet", "mixed"])
def test_replica_stops_between_two_polls(h3d, gpu, form):
    ct.check_uncapped(h3d, HIP, form)


@pytest.mark.parametrize("form", ["dirichlet", "mixed"])
def test_replica_second_solve_on_a_capped_one(h3d, gpu, form):
    ct.check_two_calls(h3d, HIP, form)


# ---- B ----------------------------------------------------------------------------
def test_already_solved(h3d, gpu):
    ct.check_already_solved(h3d, HIP)


@pytest.mark.parametrize("kind", list(vf.KINDS) + ["huge"])
def test_nonfinite_field_is_a_breakdown(h3d, gpu, kind):
    ct.check_nonfinite(h3d, HIP, kind)


@pytest.mark.parametrize("case", list(ct.RESTART_CASES), ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}-{c[3]}")
def test_restart(h3d, gpu, case):
    ct.check_restart(h3d, HIP, case)


def test_restarts_exhausted(h3d, gpu):
    ct.check_restarts_exhausted(h3d, HIP)


@pytest.mark.parametrize("name", ["reference33", "layered", "convective_slab"])
def test_solving_twice(h3d, gpu, name):
    ct.check_solving_twice(h3d, HIP, name)


# ---- C ----------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True], ids=["A", "residual"])
@pytest.mark.parametrize("form", ["uniform", "conductivity_walls"])
@pytest.mark.parametrize("name", ["long_rows", "strided", "strided_free", "strided_xplus"])
def test_past_one_pass(h3d, gpu, name, form, residual):
    """Written fields bitwise the CPU's, the same pair twice, the dot products
    within 2^-52 fsum|terms| of fsum (the long rows, and one form of the
    2.5 M-point box; the others: GPU and CPU pairs within twice that bound of
    each other)."""
    ct.check_past_one_pass(h3d, gpu, name, form, residual,
                           exact=name == "long_rows" or (name == "strided" and form == "uniform" and not residual))


# ---- D ----------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(sc.FORMS))
@pytest.mark.parametrize("cls", vf.CLASSES)
def test_value_classes_apply(h3d, gpu, cls, form):
    ct.check_value_apply(h3d, gpu, cls, form)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("cls", vf.CLASSES)
def test_value_classes_update_and_direction(h3d, gpu, cls, sign):
    ct.check_value_update(h3d, gpu, cls, sign)


@pytest.mark.parametrize("residual", [False, True], ids=["A", "residual"])
@pytest.mark.parametrize("form", ["walls", "conductivity_walls"])
def test_wall_vertices_may_hold_anything(h3d, gpu, form, residual):
    ct.check_wall_vertices_may_hold_anything(h3d, gpu, form, residual)


@pytest.mark.parametrize("residual", [False, True], ids=["A", "residual"])
@pytest.mark.parametrize("form", ["uniform", "conductivity_walls"])
@pytest.mark.parametrize("kind", list(vf.KINDS))
def test_one_spike(h3d, gpu, kind, form, residual):
    ct.check_one_spike(h3d, gpu, kind, form, residual)
