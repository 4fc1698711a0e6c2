"""Inverse-dynamics view, the parts that need no GPU: the numpy reference's own consistency
(tests/idyn_ref.py, float64) against paths that share nothing with it, and the binding of the three
entry points.

Finite differences: central, h = 1e-5 along link_ref.integrate (velocities moved by h * acc), held
to 1e-6 of the largest acceleration of the batch (truncation h^2 |a'''| ~ 1e-10 |a|, rounding
eps |v| / h ~ 1e-11 |v|: both far below). Algebraic identities: 1e-12 of the quantity's scale, as
in tests/test_dyn_view_cpu.py. Round trip through the tree solve: 1e-9 relative (condition numbers
of Mt up to 7e3, tests/test_msolve_cpu.py)."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.robots.model import asset_path, load_robot
from tests.idyn_ref import InverseDynamics
from tests.link_ref import Kinematics, integrate, random_state
from tests.msolve_ref import MassSolve

ROBOTS = ["Humanoid", "Ant", "Cartpole"]
GRAVITY = np.array([0.3, -0.2, -9.81])          # off-axis: every component is exercised
H, FD_RTOL, ALG_TOL, SOLVE_TOL = 1e-5, 1e-6, 1e-12, 1e-9
NS, DT = 8, 1.0 / 120.0


@pytest.fixture(scope="module", params=ROBOTS)
def ref(request):
    m = load_robot(request.param)
    g = np.random.default_rng(5)
    st = {k: v.astype(np.float64) for k, v in random_state(m, NS, g.uniform(-20, 20, size=(NS, 3)), seed=3).items()}
    st["rot"] /= np.linalg.norm(st["rot"], axis=1, keepdims=True)
    idr = InverseDynamics(m, st, DT, gravity=GRAVITY)
    acc = g.uniform(-10, 10, size=(NS, idr.nv))
    offs = g.uniform(-0.3, 0.3, size=(m.num_links, 3))
    return dict(name=request.param, m=m, st=st, id=idr, acc=acc, offs=offs, g=g)


def _moved(m, st, acc, nr, h):
    """Kinematics of the state moved for time h along u, with u moved along acc."""
    p, r, q = integrate(m, st["pos"], st["rot"], st["vel"], st["q"], st["qd"], h)
    vel = st["vel"].copy()
    if nr:
        vel = vel + h * acc[:, :6]
    return Kinematics(m, p, r, vel, q, st["qd"] + h * acc[:, nr:])


@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("with_offsets", [False, True])
def test_frame_acceleration_is_the_derivative_of_the_frame_velocity(ref, with_acc, with_offsets):
    m, st, idr = ref["m"], ref["st"], ref["id"]
    links = list(range(m.num_links))
    offs = ref["offs"] if with_offsets else None
    acc = ref["acc"] if with_acc else np.zeros_like(ref["acc"])
    vp = _moved(m, st, acc, idr.nr, +H).frames(links, offs)[2]
    vm = _moved(m, st, acc, idr.nr, -H).frames(links, offs)[2]
    fd = (vp - vm) / (2 * H)
    got = idr.frame_accelerations(links, offs, acc if with_acc else None)
    assert got.shape == (NS, m.num_links, 6)
    np.testing.assert_allclose(got, fd, rtol=0, atol=FD_RTOL * float(np.abs(fd).max()))
    if m.root_free and not with_offsets:       # the root frame is the root's own entries of acc
        np.testing.assert_allclose(got[:, 0], acc[:, :6], rtol=0, atol=ALG_TOL * 10)


def test_wrench_identities(ref):
    """S_l . wrench[l] == tau_rigid[dof of l]; wrench[0] == tau_rigid[root] for a floating base."""
    m, idr, acc = ref["m"], ref["id"], ref["acc"]
    for a in (None, acc):
        tau, wr = idr.tau(a, "rigid"), idr.joint_wrenches(a)
        scale = float(np.abs(wr).max())
        S = idr.joint_subspaces()
        np.testing.assert_allclose((S * wr).sum(-1)[:, 1:], tau[:, idr.nr:], rtol=0, atol=ALG_TOL * scale)
        if m.root_free:
            np.testing.assert_allclose(wr[:, 0], tau[:, :6], rtol=0, atol=ALG_TOL * scale)
    # rigid tau is M a + c + g, and at rest without acceleration the wrench on link 0 carries the weight
    d = idr.dyn
    np.testing.assert_allclose(idr.tau(acc, "rigid"), np.einsum("nij,nj->ni", d.M, acc) + d.c + d.g, rtol=0,
                               atol=ALG_TOL * float(np.abs(d.M).max()) * 10)
    rest = dict(ref["st"], vel=0 * ref["st"]["vel"], qd=0 * ref["st"]["qd"])
    w0 = InverseDynamics(m, rest, DT, gravity=GRAVITY).joint_wrenches()[:, 0, :3]
    np.testing.assert_allclose(w0, np.broadcast_to(-m.mass.sum() * GRAVITY, (NS, 3)), rtol=0, atol=1e-9)


def test_momentum_identities(ref):
    m, st, idr = ref["m"], ref["st"], ref["id"]
    mo = idr.momentum()
    assert mo["com"].shape == (NS, 3) and mo["mom"].shape == (NS, 6) and mo["cmm"].shape == (NS, 6, idr.nv)
    assert mo["energy"].shape == (NS, 2)
    np.testing.assert_allclose(mo["mom"], np.einsum("nrk,nk->nr", mo["cmm"], idr.u), rtol=0, atol=ALG_TOL)
    # frames at the centres of mass: a path that touches no Jacobian
    pc, _, vel = idr.kin.frames(list(range(m.num_links)), m.com)
    lin = np.einsum("l,nlc->nc", m.mass, vel[..., :3])
    scale = max(1.0, float(np.abs(lin).max()))
    np.testing.assert_allclose(mo["mom"][:, :3], lin, rtol=0, atol=ALG_TOL * scale)
    com = np.einsum("l,nlc->nc", m.mass, pc) / m.mass.sum()
    np.testing.assert_allclose(mo["com"], com, rtol=0, atol=ALG_TOL * 100)
    ang = np.zeros((NS, 3))
    T = np.zeros(NS)
    for l in range(m.num_links):
        v, w = vel[:, l, :3], vel[:, l, 3:]
        ang += np.cross(pc[:, l] - com, m.mass[l] * v) + np.einsum("nij,nj->ni", idr.dyn.Iw[:, l], w)
        T += 0.5 * m.mass[l] * (v * v).sum(1) + 0.5 * np.einsum("ni,nij,nj->n", w, idr.dyn.Iw[:, l], w)
    np.testing.assert_allclose(mo["mom"][:, 3:], ang, rtol=0, atol=ALG_TOL * scale)
    np.testing.assert_allclose(mo["energy"][:, 0], T, rtol=ALG_TOL, atol=ALG_TOL)
    np.testing.assert_allclose(mo["energy"][:, 0], 0.5 * np.einsum("ni,nij,nj->n", idr.u, idr.dyn.M, idr.u), rtol=ALG_TOL)
    np.testing.assert_allclose(mo["energy"][:, 1], -m.mass.sum() * (com * GRAVITY).sum(1), rtol=1e-12)
    # rows 0..2 / total mass are the Jacobian of the centre of mass: difference it along u
    cp = _moved(m, st, 0 * ref["acc"], idr.nr, +H).frames(list(range(m.num_links)), m.com)[0]
    cm = _moved(m, st, 0 * ref["acc"], idr.nr, -H).frames(list(range(m.num_links)), m.com)[0]
    dcom = np.einsum("l,nlc->nc", m.mass, (cp - cm) / (2 * H)) / m.mass.sum()
    np.testing.assert_allclose(mo["mom"][:, :3] / m.mass.sum(), dcom, rtol=0, atol=FD_RTOL * max(1.0, float(np.abs(dcom).max())))
    # no DOF of these robots leaves all mass where it is: no cmm column is all zero
    assert not np.all(mo["cmm"] == 0.0, axis=(0, 1)).any()


@pytest.mark.parametrize("mode", ["armature", "stepper"])
def test_round_trip_through_forward_dynamics(ref, mode):
    m, st, idr, g = ref["m"], ref["st"], ref["id"], np.random.default_rng(9)
    ms = MassSolve(m, st, DT, mode, gravity=GRAVITY)
    eff = g.uniform(-5, 5, size=(NS, m.num_dof))
    acc = ms.forward_dynamics(eff)
    tau = idr.tau(acc, mode)
    scale = float(np.abs(ms.forward_rhs(eff)).max())
    np.testing.assert_allclose(tau[:, idr.nr:], eff, rtol=0, atol=SOLVE_TOL * scale)
    np.testing.assert_allclose(tau[:, :idr.nr], 0.0, rtol=0, atol=SOLVE_TOL * scale)
    back = ms.forward_dynamics(tau[:, idr.nr:])
    np.testing.assert_allclose(back, acc, rtol=0, atol=SOLVE_TOL * float(np.abs(acc).max()))
    # the modes differ by their diagonal and the damping term only
    diff = idr.tau(acc, mode) - idr.tau(acc, "rigid")
    assert np.all(diff[:, :idr.nr] == 0.0)
    if np.any(m.armature[1:] > 0) or np.any(m.damping[1:] > 0):       # Cartpole's model has neither
        assert np.abs(diff[:, idr.nr:]).max() > 0


def test_per_env_parameters_and_float32():
    m = load_robot("Ant")
    g = np.random.default_rng(2)
    st = random_state(m, 4, np.zeros((4, 3)), seed=1)
    grav = g.uniform(-12, 12, size=(4, 3))
    arm, damp = g.uniform(0.01, 0.1, size=(4, m.num_dof)), g.uniform(0.1, 2.0, size=(4, m.num_dof))
    acc = g.uniform(-10, 10, size=(4, 6 + m.num_dof))
    one = InverseDynamics(m, st, DT, gravity=grav, armature=arm, damping=damp)
    for e in range(4):
        s1 = {k: v[e:e + 1] for k, v in st.items()}
        solo = InverseDynamics(m, s1, DT, gravity=grav[e], armature=arm[e:e + 1], damping=damp[e:e + 1])
        for mode in ("rigid", "armature", "stepper"):
            np.testing.assert_allclose(solo.tau(acc[e:e + 1], mode), one.tau(acc, mode)[e:e + 1], rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(solo.momentum()["energy"], one.momentum()["energy"][e:e + 1], rtol=1e-13)
    r32 = InverseDynamics(m, st, DT, dtype=np.float32)
    r64 = InverseDynamics(m, st, DT)
    links = list(range(m.num_links))
    pairs = [(r32.tau(acc, "stepper"), r64.tau(acc, "stepper")), (r32.joint_wrenches(acc), r64.joint_wrenches(acc)),
             (r32.frame_accelerations(links, None, acc), r64.frame_accelerations(links, None, acc))]
    pairs += [(r32.momentum()[k], r64.momentum()[k]) for k in ("com", "mom", "cmm", "energy")]
    for a, b in pairs:
        assert a.dtype == np.float32 and b.dtype == np.float64
        assert 0 < np.abs(a - b).max() < 1e-2


# ---- surface: these fail without the feature ----
def test_header_declares_the_entry_points():
    hdr = open(asset_path("../../../include/mi_sim.h")).read()
    for name, nargs in (("mi_get_inverse_dynamics", 6), ("mi_get_link_acceleration", 7), ("mi_get_momentum", 6)):
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert re.search(r"MI_MASS_RIGID\s*=\s*2\b", hdr)
    assert re.search(r"#define MI_ABI_VERSION 4\b", hdr)


def test_native_carries_the_signatures():
    p, i32 = C.c_void_p, C.c_int32
    assert N.MI_MASS_RIGID == 2 and (N.MI_MASS_ARMATURE, N.MI_MASS_STEPPER) == (0, 1)
    want = {"mi_get_inverse_dynamics": [p, i32, p, p, p, p],
            "mi_get_link_acceleration": [p, N._i32p, N._f32p, i32, p, p, p],
            "mi_get_momentum": [p, p, p, p, p, p]}
    for name, args in want.items():
        assert name in N.EXPORTED_SYMBOLS
        res, got = N._SIGS[name]
        assert res is C.c_int and got == args, name


def test_views_have_the_methods():
    from omniisaacgymenvs_amd.robots.articulations import ArticulationView, RigidPrimView
    for name in ("get_inverse_dynamics", "get_joint_reaction_wrenches", "get_coms", "get_momenta",
                 "get_centroidal_momentum_matrices", "get_energies"):
        assert callable(getattr(ArticulationView, name)), name
    sig = inspect.signature(ArticulationView.get_inverse_dynamics)
    assert list(sig.parameters)[1:] == ["accelerations", "mode", "indices", "clone"]
    assert sig.parameters["mode"].default == "rigid" and sig.parameters["accelerations"].default is None
    sig = inspect.signature(RigidPrimView.get_accelerations)
    assert list(sig.parameters)[1:] == ["accelerations", "indices", "clone"]
    # "rigid" is known to the inverse direction only
    with pytest.raises(ValueError):
        ArticulationView._mass_mode("rigid")


def test_library_exports_the_symbols():
    lib = C.CDLL(N.LIB_PATH)
    for name in ("mi_get_inverse_dynamics", "mi_get_link_acceleration", "mi_get_momentum"):
        assert getattr(lib, name) is not None
    lib = N.load_library()
    assert lib.mi_abi_version() == 4
    assert lib.mi_get_inverse_dynamics(None, 2, None, None, None, None) == -1      # MI_E_NULL: no sim
    assert lib.mi_get_link_acceleration(None, None, None, 1, None, None, None) == -1
    assert lib.mi_get_momentum(None, None, None, None, None, None) == -1
