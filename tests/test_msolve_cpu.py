"""Mass-matrix solve view without a GPU: the numpy restatement of the tree LTDL
(tests/msolve_ref.py) against a dense solve, the conditioning that makes a float32 tolerance
meaningful, and the surface (header, ctypes binding, Python wrappers).

Condition numbers of Mt at random_state(seed=17), N = 257 (float64): Humanoid 6.9e3 (armature) and
3.3e3 (stepper), Ant 87 and 81, Cartpole 13; the bare rigid-body M of Humanoid exceeds 1e7, which
is why no bare-M mode exists."""
import os
import re

import numpy as np
import pytest

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.robots.articulations import ArticulationView
from omniisaacgymenvs_amd.robots.model import load_robot
from tests.link_ref import random_state
from tests.msolve_ref import MODES, MassSolve, pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBOTS = ("Humanoid", "Ant", "Cartpole")
DT, NENV = 0.0083, 257
_CACHE = {}


def ref(name, mode):
    if (name, mode) not in _CACHE:
        m = load_robot(name)
        st = random_state(m, NENV, np.zeros((NENV, 3)), seed=17)
        _CACHE[name, mode] = MassSolve(m, st, DT, mode)
    return _CACHE[name, mode]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ROBOTS)
def test_tree_solve_equals_dense_solve(name, mode):
    r = ref(name, mode)
    rhs = np.random.default_rng(0).uniform(-1, 1, size=(NENV, 7, r.nv))
    x = r.solve(rhs)
    dense = np.swapaxes(np.linalg.solve(r.Mt, np.swapaxes(rhs, 1, 2)), 1, 2)
    rel = np.abs(x - dense).max(axis=(1, 2)) / np.abs(dense).max(axis=(1, 2))
    print(f"{name} {mode}: tree solve vs dense, worst env {rel.max():.3e}")
    assert rel.max() < 1e-10
    assert np.abs(r.solve(rhs[:, 0]) - x[:, 0]).max() == 0.0           # [n,nv] is R = 1
    J, X, lam = r.task([r.model.num_links - 1])
    assert np.abs(lam - J @ np.linalg.solve(r.Mt, np.swapaxes(J, 1, 2))).max() <= 1e-10 * np.abs(lam).max()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", ROBOTS)
def test_no_fill_in(name, mode):
    r = ref(name, mode)
    off = ~pattern(r.par)
    assert np.all(r.H[:, off] == 0.0)
    # and the factor is a factor: L^T D L = Mt
    L = np.tril(r.H, -1) + np.eye(r.nv)
    D = np.einsum("nii->ni", r.H)
    back = np.swapaxes(L, 1, 2) @ (D[:, :, None] * L)
    assert np.abs(back - r.Mt).max() <= 1e-12 * np.abs(r.Mt).max()


@pytest.mark.parametrize("name", ROBOTS)
def test_condition_numbers(name):
    for mode in sorted(MODES):
        cond = float(np.linalg.cond(ref(name, mode).Mt).max())
        print(f"{name} {mode}: condition number of Mt up to {cond:.3e}")
        assert cond < 1e4
    if name == "Humanoid":
        bare = float(np.linalg.cond(ref(name, "stepper").dyn.M).max())
        print(f"{name}: condition number of the bare M up to {bare:.3e}")
        assert bare > 1e7


def test_header_and_binding():
    txt = open(os.path.join(ROOT, "include", "mi_sim.h")).read()
    assert re.search(r"#define\s+MI_ABI_VERSION\s+4\b", txt)
    assert re.search(r"MI_MASS_ARMATURE\s*=\s*0\b", txt) and re.search(r"MI_MASS_STEPPER\s*=\s*1\b", txt)
    assert (N.MI_MASS_ARMATURE, N.MI_MASS_STEPPER) == (0, 1)
    for fn in ("mi_solve_mass", "mi_get_forward_dynamics", "mi_get_link_task_inertia"):
        proto = re.search(r"^int\s+" + fn + r"\s*\(([^;]*)\)\s*;", txt, flags=re.M | re.S)
        assert proto, fn
        nargs = len(proto.group(1).split(","))
        res, args = N._SIGS[fn]
        assert len(args) == nargs, (fn, len(args), nargs)
    lib = N.load_library()
    for fn in ("mi_solve_mass", "mi_get_forward_dynamics", "mi_get_link_task_inertia"):
        assert hasattr(lib, fn)
    assert lib.mi_abi_version() == 4


def test_wrappers_reject_a_bad_mode_before_the_library():
    view = ArticulationView.__new__(ArticulationView)      # no handle, no library
    for mode in ("bare", "", None, 1):
        with pytest.raises(ValueError, match="stepper"):
            view.solve_mass_matrices(None, mode=mode)
        with pytest.raises(ValueError, match="stepper"):
            view.get_forward_dynamics(mode=mode)
        with pytest.raises(ValueError, match="stepper"):
            view.get_task_space_inertias(mode=mode)


def test_build_id_covers_the_new_header():
    import __graft_entry__ as g

    assert any(os.path.basename(d) == "mi_msolve.hpp" for d in g._deps("mi_sim.hip"))
