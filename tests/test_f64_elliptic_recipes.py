"""The conditions the GPU cases of test_gpu_f64_elliptic.py rely on, from the oracle alone (no GPU): at the listed seeds every env of
every one-step case has the cone zones it is meant to exercise, no contact sits within a relative 1e-3 of the cone's surface without
being on it, no narrow-phase decision grazes (1e-9), and the reference is converged - a 100 x tighter tolerance moves no field by 0.1 of
the one-step bound.  A seed at which a condition failed would be replaced by support_f64_elliptic.first_seed's and recorded in SEEDS."""
import numpy as np
import pytest

import support_f64_elliptic as E

CASES = [(name, False, 1.0) for name in E.ONE_STEP] + list(E.FURTHER)


@pytest.mark.parametrize('name,friction0,impratio', CASES, ids=[f"{n}{'-friction0' if f else ''}{'-impratio4' if i != 1.0 else ''}" for n, f, i in CASES])
def test_the_inputs_exercise_the_zones_and_the_reference_is_converged(oracle, name, friction0, impratio):
    integrators = ('euler', 'implicitfast') if (not friction0 and impratio == 1.0) else ('euler',)
    for integrator in integrators:
        m = E.make(name, integrator, friction0=friction0, impratio=impratio)
        ins = E.inputs(name, m)
        ok, ref, what = E.conditions(oracle, name, m, ins, want_zones=not friction0)
        print(name, integrator, what)
        assert ok, (name, integrator, what)
        assert ref['iterations'].max() < m.solver_iterations, ref['iterations']      # ended by the tolerance, not by the budget
        moved = E.moved_by_a_tighter_tolerance(oracle, m, ins, ref)
        print(name, integrator, 'a 100 x tighter tolerance moves the reference by (in bounds):', {k: round(v, 5) for k, v in moved.items()})
        assert max(moved.values()) <= 0.1, moved


def test_the_zone_helper_on_hand_made_records():
    """zones() on three records of known kind: no force, |f_t| = fr f_n, |f_t| = fr f_n / 2."""
    class M:
        geom_friction = np.array([[0.0, 0, 0], [0.8, 0, 0]])
    rec = np.zeros((1, 3, 15))
    rec[0, 1, 12:15] = (2.0, 0.8*2.0*0.6, 0.8*2.0*0.8)
    rec[0, 2, 12:15] = (2.0, 0.8, 0.0)
    ref = dict(ncon=np.array([3]), contact=rec, geoms=np.tile([0, 1], (1, 3, 1)))
    none, surface, inside, nearest = E.zones(M, ref)
    assert (none[0], surface[0], inside[0]) == (1, 1, 1) and abs(nearest[0] - 0.5) < 1e-12
