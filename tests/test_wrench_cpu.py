"""Body wrenches without a GPU (include/mi_sim.h mi_apply_link_wrenches): the numpy reference of
tests/wrench_ref.py against the virtual-power identity, and the surface (header, binding, views)."""
import os

import numpy as np
import pytest

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.robots.articulations import ArticulationView, RigidPrimView
from omniisaacgymenvs_amd.robots.model import load_robot
from tests import wrench_ref as ref
from tests.link_ref import Kinematics, random_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mi_apply_link_wrenches", "mi_clear_link_wrenches", "mi_get_applied_generalized_forces")


def frames_of(model):
    """K = 3: a leaf, an interior link, the root; nonzero offsets."""
    L = model.num_links
    parents = set(int(p) for p in model.parent[1:])
    leaf = max(l for l in range(1, L) if l not in parents)
    interior = max(l for l in parents if l > 0)
    links = np.array([leaf, interior, 0], np.int32)
    offs = np.array([[0.1, -0.2, 0.05], [0.0, 0.3, -0.1], [-0.2, 0.1, 0.4]], np.float32)
    return links, offs


@pytest.mark.parametrize("name", ["Ant", "Humanoid"])
@pytest.mark.parametrize("is_global", [True, False])
def test_virtual_power(name, is_global):
    """Q . u == sum_k f_k . v_k + tau_k . w_k with v, w from the frame velocities: no Jacobian on
    the right-hand side. float64 both sides: they agree to rounding of the largest term."""
    m, n = load_robot(name), 9
    st = random_state(m, n, np.zeros((n, 3)), seed=3)
    links, offs = frames_of(m)
    g = np.random.default_rng(5)
    f, t = g.uniform(-20, 20, (n, 3, 3)), g.uniform(-5, 5, (n, 3, 3))
    Q = ref.generalized_force(m, st, links, offs, f, t, is_global)
    u = Kinematics(m, st["pos"], st["rot"], st["vel"], st["q"], st["qd"]).u(st["vel"], st["qd"])
    power = ref.virtual_power(m, st, links, offs, f, t, is_global)
    scale = (np.abs(Q) * np.abs(u)).sum(axis=1)
    assert np.all(np.abs((Q * u).sum(axis=1) - power) <= 1e-13 * scale)
    assert float(np.abs(power).max()) > 1.0
    # force alone and torque alone are the two halves
    Qf = ref.generalized_force(m, st, links, offs, f, None, is_global)
    Qt = ref.generalized_force(m, st, links, offs, None, t, is_global)
    np.testing.assert_allclose(Qf + Qt, Q, rtol=0, atol=1e-12 * np.abs(Q).max())
    # DOFs that move none of the frames get nothing; with the root frame alone only the root's
    moved = ref.moved_columns(m, links)
    assert not Q[:, ~moved].any() and moved[:6].all()
    Q0 = ref.generalized_force(m, st, links[2:], None, f[:, 2:], t[:, 2:], True)
    assert not Q0[:, 6:].any()
    np.testing.assert_array_equal(Q0[:, :3], f[:, 2])
    np.testing.assert_array_equal(Q0[:, 3:6], t[:, 2])


def test_float32_reference_is_close():
    m, n = load_robot("Humanoid"), 5
    st = random_state(m, n, np.zeros((n, 3)), seed=4)
    links, offs = frames_of(m)
    f = np.random.default_rng(1).uniform(-20, 20, (n, 3, 3))
    Q64 = ref.generalized_force(m, st, links, offs, f, None, False)
    Q32 = ref.generalized_force(m, st, links, offs, f, None, False, dtype=np.float32)
    assert Q32.dtype == np.float32
    assert np.abs(Q32 - Q64).max() <= 1e-4 * np.abs(Q64).max()


def test_surface():
    """The three entry points are declared and bound, MI_ABI_VERSION stays 4, the four view methods
    exist with the reference's signatures."""
    hdr = open(os.path.join(ROOT, "include", "mi_sim.h")).read()
    assert "#define MI_ABI_VERSION 4" in hdr
    for name in SYMBOLS:
        assert f"int {name}(" in hdr, name
        assert name in N.EXPORTED_SYMBOLS, name
    assert len(N._SIGS["mi_apply_link_wrenches"][1]) == 11
    import inspect
    sig = inspect.signature(RigidPrimView.apply_forces_and_torques_at_pos)
    assert list(sig.parameters)[1:6] == ["forces", "torques", "positions", "indices", "is_global"]
    assert sig.parameters["is_global"].default is True
    assert list(inspect.signature(RigidPrimView.apply_forces).parameters)[1:] == ["forces", "indices", "is_global"]
    assert callable(ArticulationView.get_applied_generalized_forces)
    assert callable(ArticulationView.clear_body_wrenches)


def test_kernel_header_is_a_build_dependency():
    import __graft_entry__ as g
    assert any(os.path.basename(d) == "mi_wrench.hpp" for d in g._deps("mi_sim.hip"))
