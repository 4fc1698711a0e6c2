"""Dynamics view on the GPU (include/mi_sim.h mi_get_dynamics, ArticulationView.get_mass_matrices /
get_coriolis_and_centrifugal_forces / get_generalized_gravity_forces) against the numpy reference
of tests/dyn_ref.py.

Tolerance: the rule of tests/test_gpu_link_view.py. The reference runs twice on the float32 state
read back from the device, in float64 and in float32; the device may be off the float64 run by 4x
the float32 run's worst deviation per output, floored at 2 ulp of the output's magnitude. Measured
(MI355X, N = 257, device error / bound): Humanoid M 4.2e-6 / 1.7e-5, cor 1.5e-4 / 3.5e-4, grav
5.6e-5 / 1.4e-4; Ant M 5.2e-8 / 2.2e-7, cor 1.1e-6 / 1.5e-6, grav 4.4e-7 / 2.1e-6; Cartpole M
3.2e-7 / 1.1e-6, cor 4.4e-7 / 1.5e-6, grav 1.5e-6 / 7.3e-6. Every case prints its own figures
(pytest -s); profiles/dyn_view/README.md has the table.

Stepper consistency: r = (M + diag(armature + dt damping)) (u1 - u0) / dt - (tau - c - g - damping u0)
over one mi_sim_step(1) in free flight, once with the device's M, c, g and once with the
reference's float64 terms. The float64 residual (the stepper's own float32 rounding) must be below
1e-3 of |tau - c - g|; the device residual within 2x the float64 one plus bound(M) |(u1 - u0) / dt|.
Measured (N = 16, float64 terms / device terms / limit): Ant 5.6e-6 / 4.9e-6 / 8.6e-5 at
|tau - c - g| = 9.1; Humanoid 2.1e-4 / 2.5e-4 / 5.4e-3 at 430."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.utils.task_util import make_env
from tests.dyn_ref import Dynamics
from tests.link_ref import random_state
from tests.test_gpu_link_view import read_state, write_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("Humanoid", 257), ("Ant", 257), ("Cartpole", 257), ("Ant", 1)]
EPS = float(np.finfo(np.float32).eps)
KINDS = ("M", "cor", "grav")


def dynamics(view, M=True, cor=True, grav=True, offset=0):
    """mi_get_dynamics into fresh NaN-filled buffers -> (rc, dict of numpy arrays); skipped outputs
    pass NULL. ``offset``: floats the M buffer is shifted off its 16-B alignment."""
    n, nv = view.count, view.num_gen_vel
    t = {k: torch.full((int(np.prod(s)) + (offset if k == "M" else 0),), np.nan, device="cuda:0") if on else None
         for k, s, on in (("M", (n, nv, nv), M), ("cor", (n, nv), cor), ("grav", (n, nv), grav))}
    p = {k: None if v is None else v.data_ptr() + (4 * offset if k == "M" else 0) for k, v in t.items()}
    rc = N.lib().mi_get_dynamics(view.handle, p["M"], p["cor"], p["grav"], view.stream())
    torch.cuda.synchronize()
    shape = {"M": (n, nv, nv), "cor": (n, nv), "grav": (n, nv)}
    return rc, {k: v.cpu().numpy()[(offset if k == "M" else 0):].reshape(shape[k]) for k, v in t.items() if v is not None}


def refs_and_bounds(model, st, gravity):
    args = (st["pos"], st["rot"], st["vel"], st["q"], st["qd"])
    d64 = Dynamics(model, *args, gravity=gravity)
    d32 = Dynamics(model, *args, gravity=gravity, dtype=np.float32)
    r64 = {"M": d64.M, "cor": d64.c, "grav": d64.g}
    r32 = {"M": d32.M, "cor": d32.c, "grav": d32.g}
    bound = {k: max(4.0 * float(np.abs(r32[k] - r64[k]).max()), 2.0 * EPS * float(np.abs(r64[k]).max())) for k in r64}
    return d64, r64, bound


def check(tag, got, r64, bound, kinds=KINDS):
    for k in kinds:
        g = got[k].astype(np.float64)
        err = float(np.abs(g - r64[k]).max())
        print(f"{tag} {k}: device error {err:.3e} bound {bound[k]:.3e} ratio {err / bound[k]:.2f}")
        assert np.isfinite(g).all(), (tag, k)
        assert err <= bound[k], (tag, k, err, bound[k])


def sim_gravity(view):
    return np.array([float(x) for x in view.sim_params.gravity], dtype=np.float32)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def case(request, gpu):
    name, n = request.param
    env = make_env(name, num_envs=n, device="cuda:0", seed=11)
    env.reset()
    view = env.task.get_robot()
    m = view.model
    write_state(view, random_state(m, n, view.env_origins, seed=17))
    st = read_state(view)
    c = dict(name=name, n=n, env=env, view=view, model=m, st=st, tag=f"{name}-{n}")
    c["ref"] = refs_and_bounds(m, st, sim_gravity(view))
    rc, c["got"] = dynamics(view)
    assert rc == 0
    yield c
    env.close()


def test_parity(case):
    _, r64, bound = case["ref"]
    nv = case["view"].num_gen_vel
    assert case["got"]["M"].shape == (case["n"], nv, nv)
    check(case["tag"], case["got"], r64, bound)


def test_structure_is_bit_exact(case):
    view, m, n, got = case["view"], case["model"], case["n"], case["got"]
    M = got["M"]
    assert np.array_equal(M, M.transpose(0, 2, 1))
    dead = ~case["ref"][0].pattern()
    assert np.all(M[:, dead] == 0.0) and not np.signbit(M[:, dead]).any()
    assert np.all(np.linalg.eigvalsh(M.astype(np.float64)) > 0)
    if m.root_free:      # the root's z entry of grav is +9.81 total mass
        np.testing.assert_allclose(got["grav"][:, 2], -sim_gravity(view)[2] * m.mass.sum(), rtol=4 * EPS * m.num_links)
    if n < 2:
        return
    # grav (M, cor too) of two envs with one orientation, q and velocity at different places
    st = {k: v.copy() for k, v in case["st"].items()}
    for k in ("rot", "vel", "q", "qd"):
        st[k][n - 1] = st[k][0]
    assert np.abs(st["pos"][n - 1] - st["pos"][0]).max() > 0.5
    try:
        write_state(view, st)
        rc, two = dynamics(view)
        assert rc == 0
        for k in KINDS:
            assert np.array_equal(two[k][0], two[k][n - 1]), k
            assert np.array_equal(two[k][0], got[k][0]), k
    finally:
        write_state(view, case["st"])
        torch.cuda.synchronize()


def test_output_selection(case):
    view, got, n = case["view"], case["got"], case["n"]
    for k in KINDS:
        rc, one = dynamics(view, **{x: x == k for x in KINDS})
        assert rc == 0 and list(one) == [k] and np.array_equal(one[k], got[k]), k
    rc, none = dynamics(view, M=False, cor=False, grav=False)
    assert rc == -1 and none == {} and b"all null" in N.lib().mi_last_error()       # MI_E_NULL
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        view._dynamics(False, False, False)
    # the Python surface
    M, c, g = view.get_dynamics()
    for t, k in ((M, "M"), (c, "cor"), (g, "grav")):
        assert np.array_equal(t.cpu().numpy(), got[k])
    assert torch.equal(view.get_mass_matrices(), M)
    assert torch.equal(view.get_coriolis_and_centrifugal_forces(), c)
    assert torch.equal(view.get_generalized_gravity_forces(), g)
    idx = torch.tensor([n - 1, 0, n // 2], device="cuda:0")
    assert torch.equal(view.get_mass_matrices(indices=idx), M[idx])
    assert torch.equal(view.get_coriolis_and_centrifugal_forces(indices=idx), c[idx])
    assert torch.equal(view.get_generalized_gravity_forces(indices=idx), g[idx])
    for fn in (view.get_mass_matrices, view.get_coriolis_and_centrifugal_forces, view.get_generalized_gravity_forces):
        a, b, cl = fn(clone=False), fn(clone=False), fn()
        assert a.data_ptr() == b.data_ptr() != cl.data_ptr() and torch.equal(a, cl)


def test_unaligned_buffer(case):
    """An M buffer one float off a 16-B boundary takes the dword stores: same bits."""
    rc, off = dynamics(case["view"], cor=False, grav=False, offset=1)
    assert rc == 0 and np.array_equal(off["M"], case["got"]["M"])


_CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, {root!r})
from omniisaacgymenvs_amd.utils.task_util import make_env
from tests.test_gpu_link_view import write_state
from tests.test_gpu_dyn_view import dynamics
st = dict(np.load({state!r}))
env = make_env({name!r}, num_envs=st["q"].shape[0], device="cuda:0", seed=11)
env.reset()
view = env.task.get_robot()
write_state(view, st)
rc, got = dynamics(view)
assert rc == 0
np.savez({out!r}, path=view.sim_kernel_path()[0], **got)
env.close()
"""


@pytest.mark.parametrize("name", ["Humanoid", "Ant"])
def test_both_state_layouts(gpu, name, tmp_path):
    """The same state on the default sim (paired kernels) and on an MI_WAVE_PAIR=0 sim in a fresh
    child process (one env per wavefront, per-env records): identical bits."""
    n = 64
    env = make_env(name, num_envs=n, device="cuda:0", seed=11)
    env.reset()
    view = env.task.get_robot()
    st = random_state(view.model, n, view.env_origins, seed=31)
    write_state(view, st)
    rc, here = dynamics(view)
    path = view.sim_kernel_path()[0]
    env.close()
    assert rc == 0
    np.savez(tmp_path / "state.npz", **st)
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT, state=str(tmp_path / "state.npz"), name=name, out=str(tmp_path / "out.npz")))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, MI_WAVE_PAIR="0"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    there = np.load(tmp_path / "out.npz")
    assert int(there["path"]) == 1 and path != 1, (path, int(there["path"]))
    for k in KINDS:
        assert np.array_equal(here[k], there[k]), k


@pytest.mark.parametrize("name", ["Humanoid", "Ant", "Cartpole"])
def test_after_stepping(gpu, name):
    """Three mi_sim_step calls left deferred: the getter issues them itself; its result is the
    reference's on the state read back afterwards."""
    n = 257
    env = make_env(name, num_envs=n, device="cuda:0", seed=23)
    env.reset()
    view = env.task.get_robot()
    gen = torch.Generator().manual_seed(4)
    for _ in range(3):
        env.step((torch.rand((n, env.num_actions), generator=gen) * 2 - 1).cuda())
    before = read_state(view)
    for _ in range(3):
        view.sim_step(1)                                   # deferred
    rc, got = dynamics(view)                               # must flush
    assert rc == 0
    st = read_state(view)
    assert not np.array_equal(st["q"], before["q"])
    _, r64, bound = refs_and_bounds(view.model, st, sim_gravity(view))
    check(f"{name} after stepping", got, r64, bound)
    env.close()


def test_capture(case):
    """The call inside torch.cuda.graph, replayed after the state changed, equals the eager result
    bit for bit; the view's getters allocate nothing after their first call."""
    view, m, n = case["view"], case["model"], case["n"]
    nv = view.num_gen_vel
    M, c, g = (torch.zeros(s, device="cuda:0") for s in ((n, nv, nv), (n, nv), (n, nv)))

    def call():
        assert N.lib().mi_get_dynamics(view.handle, M.data_ptr(), c.data_ptr(), g.data_ptr(), view.stream()) == 0

    call()
    view.get_dynamics(clone=False)
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    for _ in range(3):
        view.get_dynamics(clone=False)
        view.get_mass_matrices(clone=False)
    assert torch.cuda.memory_allocated() == mem
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            call()
    torch.cuda.current_stream().wait_stream(s)
    try:
        write_state(view, random_state(m, n, view.env_origins, seed=29))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.cpu().numpy().copy() for t in (M, c, g)]
        for t in (M, c, g):
            t.zero_()
        call()
        torch.cuda.synchronize()
        for a, t in zip(replayed, (M, c, g)):
            assert np.array_equal(a, t.cpu().numpy())
        assert not np.array_equal(replayed[1], case["got"]["cor"])       # the state did change
    finally:
        write_state(view, case["st"])
        torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["Humanoid", "Ant", "Cartpole"])
def test_per_env_gravity(gpu, name):
    n = 66
    env = make_env(name, num_envs=n, device="cuda:0", seed=11)
    env.reset()
    view = env.task.get_robot()
    m = view.model
    write_state(view, random_state(m, n, view.env_origins, seed=17))
    st = read_state(view)
    rc, first = dynamics(view)
    assert rc == 0
    grav = np.random.default_rng(7).uniform(-12, 12, size=(n, 3)).astype(np.float32)
    view.set_env_gravity(torch.from_numpy(grav).cuda())
    rc, got = dynamics(view)
    assert rc == 0
    _, r64, bound = refs_and_bounds(m, st, grav)
    check(f"{name} per-env gravity", got, r64, bound, ("grav",))
    assert np.array_equal(got["M"], first["M"]) and np.array_equal(got["cor"], first["cor"])
    assert not np.array_equal(got["grav"], first["grav"])
    torch.cuda.synchronize()
    view.clear_env_params()
    rc, back = dynamics(view)
    assert rc == 0
    for k in KINDS:
        assert np.array_equal(back[k], first[k]), k
    env.close()


# ---- the getter's terms are the stepper's ----
def _free_flight(name, n, seed, moving):
    env = make_env(name, num_envs=n, device="cuda:0", seed=seed,
                   overrides=["solver_type=0", f"task.sim.{name}.enable_self_collisions=False",
                              f"task.sim.{name}.angular_damping=0.0"])
    env.reset()
    view = env.task.get_robot()
    m = view.model
    assert float(view.sim_params.angular_damping) == 0.0 and int(view.sim_params.solver_type) == 0
    g = np.random.default_rng(seed)
    lo, hi = m.lower[1:].copy(), m.upper[1:].copy()
    free = lo >= hi
    lo[free], hi[free] = 0.0, 0.0
    st = random_state(m, n, view.env_origins, seed=seed)
    st["q"] = np.broadcast_to(((lo + hi) / 2).astype(np.float32), (n, m.num_dof)).copy()
    st["pos"] = (np.asarray(view.env_origins, np.float32).reshape(n, 3) + np.array([0, 0, 5], np.float32))
    amp = 1.0 if moving else 0.0
    st["vel"] = (amp * g.uniform(-1, 1, size=(n, 6))).astype(np.float32)
    st["qd"] = (amp * g.uniform(-1, 1, size=(n, m.num_dof))).astype(np.float32)
    write_state(view, st)
    return env, view, g


def _residual(view, M, c, g, tau, u0, u1, dt):
    m = view.model
    nr = 6
    damp = view.get_joint_dampings().cpu().numpy().astype(np.float64)
    arm = view.get_armatures().cpu().numpy().astype(np.float64)
    extra = np.zeros_like(u0)
    extra[:, nr:] = arm + dt * damp
    ud = (u1 - u0) / dt
    rhs = -c - g
    rhs[:, nr:] += tau - damp * u0[:, nr:]
    r = np.einsum("nij,nj->ni", M, ud) + extra * ud - rhs
    return float(np.abs(r).max()), float(np.abs(ud).max()), float(np.abs(rhs).max())


def _u(st):
    return np.concatenate([st["vel"], st["qd"]], axis=1).astype(np.float64)


@pytest.mark.parametrize("name", ["Ant", "Humanoid"])
def test_consistency_with_the_stepper(gpu, name):
    n = 16
    env, view, g = _free_flight(name, n, seed=5, moving=True)
    m, dt = view.model, float(view.sim_params.dt)
    tau = g.uniform(-5, 5, size=(n, m.num_dof)).astype(np.float32)
    view.set_joint_efforts(torch.from_numpy(tau).cuda())
    st0 = read_state(view)
    rc, dev = dynamics(view)
    assert rc == 0
    view.sim_step(1)
    st1 = read_state(view)
    _, r64, bound = refs_and_bounds(m, st0, sim_gravity(view))
    u0, u1 = _u(st0), _u(st1)
    args = (tau.astype(np.float64), u0, u1, dt)
    r_ref, ud, scale = _residual(view, r64["M"], r64["cor"], r64["grav"], *args)
    r_dev, _, _ = _residual(view, *(dev[k].astype(np.float64) for k in KINDS), *args)
    limit = 2.0 * r_ref + bound["M"] * ud
    print(f"{name} stepper: residual float64 terms {r_ref:.3e}, device terms {r_dev:.3e} (limit {limit:.3e}); "
          f"|tau - c - g| {scale:.3e}, |du/dt| {ud:.3e}")
    assert r_ref < 1e-3 * scale, "a limit or contact row fired: choose another state"
    assert r_dev <= limit
    env.close()


def _step_from_rest(view, tau):
    """One substep under efforts tau; the residual figures and the bound on |u1 - prediction|: a
    residual force r changes u by dt M~^-1 r, at most dt |r|_2 / lambda_min(M~) with |r|_2 <= sqrt(nv) |r|_inf."""
    m, dt, nv, nr = view.model, float(view.sim_params.dt), view.num_gen_vel, 6 if view.model.root_free else 0
    view.set_joint_efforts(tau)
    st0 = read_state(view)
    rc, dev = dynamics(view)
    assert rc == 0
    view.sim_step(1)
    st1 = read_state(view)
    _, r64, bound = refs_and_bounds(m, st0, sim_gravity(view))
    u = lambda st: _u(st)[:, 6 - nr:]
    u0, u1 = u(st0), u(st1)
    damp = view.get_joint_dampings().cpu().numpy().astype(np.float64)
    arm = view.get_armatures().cpu().numpy().astype(np.float64) if nr else np.zeros_like(damp)
    ud = (u1 - u0) / dt
    res = {}
    for tag, (M, c, g) in (("ref", (r64["M"], r64["cor"], r64["grav"])), ("dev", tuple(dev[k].astype(np.float64) for k in KINDS))):
        Mt = M.copy()
        Mt[:, range(nr, nv), range(nr, nv)] += arm + dt * damp
        rhs = -c - g
        rhs[:, nr:] += tau.cpu().numpy().astype(np.float64) - damp * u0[:, nr:]
        res[tag] = float(np.abs(np.einsum("nij,nj->ni", Mt, ud) - rhs).max())
        res[tag + "_pred"] = u0 + dt * np.linalg.solve(Mt, rhs[:, :, None])[:, :, 0]
        res["lmin"] = float(np.linalg.eigvalsh(Mt).min())
    limit = 2.0 * res["ref"] + bound["M"] * float(np.abs(ud).max())
    return st1, u1, ud, res, limit, dt * np.sqrt(nv) * limit / res["lmin"]


@pytest.mark.parametrize("name", ["Cartpole", "Ant", "Humanoid"])
def test_gravity_compensation(gpu, name):
    """The controller the getters are for. A supported base (Cartpole's rail): efforts = grav hold
    every joint from rest; after one substep the joint velocities are zero within the
    stepper-consistency bound. A free-flying base (Ant, Humanoid; the stepper check's set-up at
    rest) needs no joint effort to keep its joints still, which the terms say themselves:
    grav[:, 6:] = -M[:, 6:, :3] gravity. There the efforts grav[:, 6:] are applied all the same and
    the step is the one the device's M, c, g predict, u0 + dt M~^-1 (tau - c - g), within the same
    bound, root rows included; with zero efforts the joints stay and the root falls at gravity."""
    n = 16
    if name == "Cartpole":
        env = make_env(name, num_envs=n, device="cuda:0", seed=6)
        env.reset()
        view = env.task.get_robot()
        st = random_state(view.model, n, view.env_origins, seed=6)
        st["rot"][:] = read_state(view)["rot"]
        st["qd"][:] = 0.0
        write_state(view, st)
        tau = view.get_generalized_gravity_forces()
        assert float(tau[:, 1].abs().max()) > 0.1                       # the pole does need holding
        st1, u1, ud, res, limit, du_limit = _step_from_rest(view, tau)
        print(f"{name} gravity compensation: |qd| {np.abs(st1['qd']).max():.3e} (limit {du_limit:.3e}), residual device "
              f"{res['dev']:.3e} float64 {res['ref']:.3e}")
        assert res["dev"] <= limit and np.abs(st1["qd"]).max() <= du_limit
        env.close()
        return
    env, view, _ = _free_flight(name, n, seed=6, moving=False)
    grav3 = sim_gravity(view)
    M, _, g = view.get_dynamics()
    pull = -(M[:, 6:, :3].double() @ torch.from_numpy(grav3).double().cuda()).cpu().numpy()
    _, r64, bound = refs_and_bounds(view.model, read_state(view), grav3)
    assert np.abs(pull - g[:, 6:].cpu().numpy()).max() <= bound["grav"] + 3 * float(np.abs(grav3).max()) * bound["M"]
    st1, u1, ud, res, limit, du_limit = _step_from_rest(view, g[:, 6:].contiguous())
    err = float(np.abs(u1 - res["dev_pred"]).max())
    print(f"{name} efforts = grav[:, 6:] in free flight: |u1 - predicted| {err:.3e} (limit {du_limit:.3e}), residual device "
          f"{res['dev']:.3e} float64 {res['ref']:.3e}, |qd| {np.abs(st1['qd']).max():.3e}")
    assert res["dev"] <= limit and err <= du_limit
    env.close()
    env, view, _ = _free_flight(name, n, seed=6, moving=False)
    st1, u1, ud, res, limit, du_limit = _step_from_rest(view, torch.zeros((n, view.num_dof), device="cuda:0"))
    print(f"{name} zero efforts in free flight: |qd| {np.abs(st1['qd']).max():.3e} (limit {du_limit:.3e}), root dv/dt {ud[:, :3].mean(0)}")
    assert res["dev"] <= limit and np.abs(st1["qd"]).max() <= du_limit
    np.testing.assert_allclose(ud[:, :3], np.broadcast_to(grav3, (n, 3)), rtol=0, atol=du_limit / float(view.sim_params.dt))
    env.close()
