"""Mass-matrix solve view on the GPU (include/mi_sim.h mi_solve_mass / mi_get_forward_dynamics /
mi_get_link_task_inertia, ArticulationView.solve_mass_matrices / get_forward_dynamics /
get_task_space_inertias) against the numpy reference of tests/msolve_ref.py.

Tolerance: the rule of tests/test_gpu_link_view.py and tests/test_gpu_dyn_view.py, applied per env
because |x| varies by orders of magnitude between envs. The reference runs on the float32 state
read back from the device, in float64 and in float32 (the same elimination order); an env's error
is max|x - x64| / max|x64| of that env and output; the device's worst env may be off by 4x the
float32 run's worst env, floored at 2 ulp. Every check prints device error, bound and ratio
(pytest -s); profiles/msolve/README.md has the measured table.

Measured (MI355X, N = 257 unless named, worst device error / bound ratio of the row over both modes
and R = 1, 7, 32, 70 / K = 1, all bodies): Humanoid solve 8.8e-6 / 2.9e-5 (0.35 at R = 70), forward
dynamics 0.17, minv_jt 0.19, lam_inv 0.32, lam_inv vs J minv_jt^T 0.15; Ant solve 0.26, forward
dynamics 0.25, minv_jt 0.23, lam_inv 0.29; Cartpole solve 0.20, forward dynamics 0.23, minv_jt 0.13,
lam_inv 0.18; Ant with one env solve 0.25, minv_jt 0.33, lam_inv 0.34. The residual is at most 5 %
of its limit. With the mass matrix assembled in float about one common point Humanoid in mode
"armature" was at 1.02 .. 1.42 (solves) and 4.6 (minv_jt): the kernel forms it in double.

Stepper consistency: (u1 - u0) / dt over one mi_sim_step(1) in free flight against
get_forward_dynamics(mode="stepper"), within sqrt(nv) limit / lambda_min(Mt), limit = 2 x the
float64-terms residual + bound(M) |du/dt| (tests/test_gpu_dyn_view.py _step_from_rest)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.utils.task_util import make_env
from tests.link_ref import random_state
from tests.msolve_ref import MODES, MassSolve
from tests.test_gpu_dyn_view import _free_flight, _u, refs_and_bounds, sim_gravity
from tests.test_gpu_link_view import read_state, write_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("Humanoid", 257), ("Ant", 257), ("Cartpole", 257), ("Ant", 1)]
EPS = float(np.finfo(np.float32).eps)
E_NULL, E_SHAPE, E_ARG = -1, -2, -5
NAN = float("nan")


# ---- device calls ----
def _dev(a, offset=0):
    """numpy -> device floats, shifted `offset` floats off the allocation's alignment."""
    flat = torch.full((a.size + offset,), NAN, device="cuda:0")
    flat[offset:] = torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()
    return flat


def solve(view, which, rhs, alias=False, offset=0):
    n, R, nv = rhs.shape
    src = _dev(rhs, offset)
    dst = src if alias else torch.full((rhs.size + offset,), NAN, device="cuda:0")
    rc = N.lib().mi_solve_mass(view.handle, which, src.data_ptr() + 4 * offset, R, dst.data_ptr() + 4 * offset, view.stream())
    torch.cuda.synchronize()
    return rc, dst.cpu().numpy()[offset:].reshape(n, R, nv)


def forward(view, which, tau=None):
    acc = torch.full((view.count, view.num_gen_vel), NAN, device="cuda:0")
    t = None if tau is None else torch.from_numpy(np.ascontiguousarray(tau, np.float32)).cuda()
    rc = N.lib().mi_get_forward_dynamics(view.handle, which, N.ptr(t), acc.data_ptr(), view.stream())
    torch.cuda.synchronize()
    return rc, acc.cpu().numpy()


def task(view, which, links, offs, minv=True, lam=True, K=None):
    ids = np.ascontiguousarray(links, dtype=np.int32)
    o = None if offs is None else np.ascontiguousarray(offs, dtype=np.float32)
    K = len(ids) if K is None else K
    n, nv, Q = view.count, view.num_gen_vel, 6 * max(K, 1)
    t = {"minv_jt": torch.full((n, Q, nv), NAN, device="cuda:0") if minv else None,
         "lam_inv": torch.full((n, Q, Q), NAN, device="cuda:0") if lam else None}
    rc = N.lib().mi_get_link_task_inertia(view.handle, which, N.iptr(ids), N.fptr(o), K, N.ptr(t["minv_jt"]),
                                          N.ptr(t["lam_inv"]), view.stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in t.items() if v is not None}


# ---- the bound ----
def rel_env(x, x64):
    ax = tuple(range(1, x64.ndim))
    return np.abs(np.asarray(x, np.float64) - x64).max(axis=ax) / np.abs(x64).max(axis=ax)


def bound_of(x32, x64):
    return max(4.0 * float(rel_env(x32, x64).max()), 2.0 * EPS)


def check(tag, dev, x32, x64):
    bound = bound_of(x32, x64)
    err = float(rel_env(dev, x64).max())
    print(f"{tag}: device error {err:.3e} bound {bound:.3e} ratio {err / bound:.2f}")
    assert np.isfinite(dev).all(), tag
    assert err <= bound, (tag, err, bound)
    return bound


def refs(view, st, mode, **kw):
    args = (view.model, st, float(view.sim_params.dt), mode)
    g = kw.pop("gravity", sim_gravity(view))
    return MassSolve(*args, gravity=g, **kw), MassSolve(*args, gravity=g, dtype=np.float32, **kw)


def frames(view, which):
    m = view.model
    if which == "one":            # one foot, or the pole: the last body
        links, offs = view._frames([m.body_names[-1]])
    else:
        links, offs = view._frames(None)
    return links, offs


def rhs_of(n, R, nv):
    return np.random.default_rng(0).uniform(-1, 1, size=(n, R, nv)).astype(np.float32)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def case(request, gpu):
    name, n = request.param
    env = make_env(name, num_envs=n, device="cuda:0", seed=11)
    env.reset()
    view = env.task.get_robot()
    write_state(view, random_state(view.model, n, view.env_origins, seed=17))
    tau = np.random.default_rng(3).uniform(-5, 5, size=(n, view.num_dof)).astype(np.float32)
    view.set_joint_efforts(torch.from_numpy(tau).cuda())
    st = read_state(view)
    c = dict(name=name, n=n, env=env, view=view, model=view.model, st=st, tau=tau, tag=f"{name}-{n}")
    c["ref"] = {mode: refs(view, st, mode) for mode in MODES}
    c["boundM"] = refs_and_bounds(view.model, st, sim_gravity(view))[2]["M"]
    yield c
    env.close()


@pytest.mark.parametrize("R", [1, 7, 32, 70])     # 70: more than one LDS tile of 64 vectors, the last ragged
def test_solve_parity_and_residual(case, R):
    view, n, nv = case["view"], case["n"], case["view"].num_gen_vel
    rhs = rhs_of(n, R, nv)
    for mode, which in MODES.items():
        r64, r32 = case["ref"][mode]
        rc, x = solve(view, which, rhs)
        assert rc == 0
        x64 = r64.solve(rhs)
        bound = check(f"{case['tag']} solve {mode} R={R}", x, r32.solve(rhs), x64)
        # residual against the float64 matrix: a wrong diagonal or a transposed factor shows here
        xd = x.astype(np.float64)
        res = np.abs(np.einsum("nij,nrj->nri", r64.Mt, xd) - rhs).max(axis=(1, 2))
        xmax = np.abs(xd).max(axis=(1, 2))
        lim = bound * np.abs(r64.Mt).sum(axis=2).max(axis=1) * xmax + case["boundM"] * xmax
        print(f"{case['tag']} residual {mode} R={R}: worst residual / limit {float((res / lim).max()):.2f}")
        assert np.all(res <= lim)


def test_alias_alignment_and_errors(case):
    view, n, nv = case["view"], case["n"], case["view"].num_gen_vel
    lib, h, st = N.lib(), view.handle, view.stream()
    for R in (1, 7):
        rhs = rhs_of(n, R, nv)
        rc, x = solve(view, 1, rhs)
        rc1, xa = solve(view, 1, rhs, alias=True)
        rc2, xo = solve(view, 1, rhs, offset=1)
        rc3, xao = solve(view, 1, rhs, alias=True, offset=1)
        assert rc == rc1 == rc2 == rc3 == 0
        assert np.array_equal(x, xa) and np.array_equal(x, xo) and np.array_equal(x, xao)
    buf = torch.zeros((n, nv), device="cuda:0")
    p = buf.data_ptr()
    ids = np.zeros(1, np.int32)
    assert lib.mi_solve_mass(h, 1, p, 0, p, st) == E_SHAPE and b"R=0" in lib.mi_last_error()
    assert lib.mi_solve_mass(h, 2, p, 1, p, st) == E_ARG and b"which=2" in lib.mi_last_error()
    assert lib.mi_get_forward_dynamics(h, 2, None, p, st) == E_ARG and b"which=2" in lib.mi_last_error()
    assert lib.mi_solve_mass(h, 1, p, 1, None, st) == E_NULL and b"null" in lib.mi_last_error()
    assert lib.mi_solve_mass(h, 1, None, 1, p, st) == E_NULL
    assert lib.mi_get_forward_dynamics(h, 1, None, None, st) == E_NULL and b"null" in lib.mi_last_error()
    assert lib.mi_get_link_task_inertia(h, 1, N.iptr(ids), None, 1, None, None, st) == E_NULL
    assert b"both null" in lib.mi_last_error()
    assert lib.mi_get_link_task_inertia(h, 1, N.iptr(ids), None, 0, p, None, st) == E_SHAPE and b"K=0" in lib.mi_last_error()
    assert lib.mi_get_link_task_inertia(h, 2, N.iptr(ids), None, 1, p, None, st) == E_ARG
    bad = np.array([view.model.num_links], np.int32)
    assert lib.mi_get_link_task_inertia(h, 1, N.iptr(bad), None, 1, p, None, st) == E_ARG
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                   # no refused call wrote anything


def test_forward_dynamics_parity_and_null_tau(case):
    view = case["view"]
    for mode, which in MODES.items():
        r64, r32 = case["ref"][mode]
        rc, acc = forward(view, which, case["tau"])
        rc0, acc0 = forward(view, which, None)             # the efforts last set
        assert rc == 0 and rc0 == 0 and np.array_equal(acc, acc0)
        check(f"{case['tag']} forward dynamics {mode}", acc, r32.forward_dynamics(case["tau"]),
              r64.forward_dynamics(case["tau"]))
        # the same right-hand side through mi_solve_mass: the two entry points share the factor
        rc, x = solve(view, which, r32.forward_rhs(case["tau"])[:, None, :])
        assert rc == 0
        check(f"{case['tag']} forward dynamics via solve {mode}", x[:, 0], r32.forward_dynamics(case["tau"]),
              r64.forward_dynamics(case["tau"]))


@pytest.mark.parametrize("K", ["one", "all"])
def test_task_inertia(case, K):
    view = case["view"]
    links, offs = frames(view, K)
    for mode, which in MODES.items():
        r64, r32 = case["ref"][mode]
        rc, got = task(view, which, links, offs)
        assert rc == 0
        J64, X64, lam64 = r64.task(links, offs)
        _, X32, lam32 = r32.task(links, offs)
        tag = f"{case['tag']} task {mode} K={len(links)}"
        check(tag + " minv_jt", got["minv_jt"], X32, X64)
        bound = check(tag + " lam_inv", got["lam_inv"], lam32, lam64)
        lam = got["lam_inv"]
        assert np.array_equal(lam, lam.transpose(0, 2, 1))
        # lam_inv = J minv_jt^T from the device's own outputs (J from mi_get_link_jacobian)
        jac = view.get_jacobians(None if K == "all" else [view.model.body_names[-1]]).cpu().numpy().astype(np.float64)
        own = jac.reshape(jac.shape[0], -1, jac.shape[-1]) @ got["minv_jt"].astype(np.float64).transpose(0, 2, 1)
        err = float(rel_env(lam, own).max())
        print(f"{tag} lam_inv vs J minv_jt^T: {err:.3e} bound {bound:.3e} ratio {err / bound:.2f}")
        assert err <= bound
        if K == "one":
            # positive definite where it can be: six rows of a model with nv < 6 (Cartpole) span
            # nv directions only; the other eigenvalues are rounding of zero
            ev = np.linalg.eigvalsh(lam.astype(np.float64))
            rank = min(6, view.num_gen_vel)
            assert np.all(ev[:, 6 - rank:] > 0)
            assert np.all(np.abs(ev[:, :6 - rank]) <= bound * ev[:, -1:])
        for k in ("minv_jt", "lam_inv"):
            rc, one = task(view, which, links, offs, minv=k == "minv_jt", lam=k == "lam_inv")
            assert rc == 0 and list(one) == [k] and np.array_equal(one[k], got[k]), k


@pytest.mark.parametrize("name", ["Cartpole", "Ant", "Humanoid"])
def test_forward_dynamics_predicts_the_stepper(gpu, name):
    n = 16
    if name == "Cartpole":
        env = make_env(name, num_envs=n, device="cuda:0", seed=6)
        env.reset()
        view = env.task.get_robot()
        st = random_state(view.model, n, view.env_origins, seed=6)
        st["rot"][:] = read_state(view)["rot"]
        st["qd"][:] = 0.0
        write_state(view, st)
        g = np.random.default_rng(6)
    else:
        env, view, g = _free_flight(name, n, seed=5, moving=True)
    m, dt, nv, nr = view.model, float(view.sim_params.dt), view.num_gen_vel, 6 if view.model.root_free else 0
    tau = g.uniform(-5, 5, size=(n, m.num_dof)).astype(np.float32)
    view.set_joint_efforts(torch.from_numpy(tau).cuda())
    st0 = read_state(view)
    acc = view.get_forward_dynamics(mode="stepper").cpu().numpy().astype(np.float64)
    view.sim_step(1)
    st1 = read_state(view)
    _, r64, bound = refs_and_bounds(m, st0, sim_gravity(view))
    u0, u1 = _u(st0)[:, 6 - nr:], _u(st1)[:, 6 - nr:]
    damp = view.get_joint_dampings().cpu().numpy().astype(np.float64)
    arm = view.get_armatures().cpu().numpy().astype(np.float64) if nr else np.zeros_like(damp)
    Mt = r64["M"].copy()
    Mt[:, range(nr, nv), range(nr, nv)] += arm + dt * damp
    rhs = -r64["cor"] - r64["grav"]
    rhs[:, nr:] += tau.astype(np.float64) - damp * u0[:, nr:]
    ud = (u1 - u0) / dt
    r_ref = float(np.abs(np.einsum("nij,nj->ni", Mt, ud) - rhs).max())
    scale = float(np.abs(rhs).max())
    limit = 2.0 * r_ref + bound["M"] * float(np.abs(ud).max())
    acc_limit = np.sqrt(nv) * limit / float(np.linalg.eigvalsh(Mt).min())
    err = float(np.abs(ud - acc).max())
    print(f"{name} stepper: |du/dt - acc| {err:.3e} (limit {acc_limit:.3e}); residual float64 terms {r_ref:.3e}, "
          f"|tau - c - g| {scale:.3e}, |du/dt| {float(np.abs(ud).max()):.3e}")
    assert r_ref < 1e-3 * scale, "a limit or contact row fired: choose another state"
    assert err <= acc_limit
    env.close()


def outputs(view, tau):
    """Every entry point once: the bits the layout / capture / table tests compare."""
    n, nv = view.count, view.num_gen_vel
    links, offs = frames(view, "all")
    out = {}
    for mode, which in MODES.items():
        rc, out[f"solve_{mode}"] = solve(view, which, rhs_of(n, 7, nv))
        assert rc == 0
        rc, out[f"fd_{mode}"] = forward(view, which, tau)
        assert rc == 0
    rc, t = task(view, 1, links, offs)
    assert rc == 0
    out.update(t)
    return out


@pytest.mark.parametrize("name", ["Cartpole", "Ant", "Humanoid"])
def test_per_env_table(gpu, name):
    n = 66
    env = make_env(name, num_envs=n, device="cuda:0", seed=11)
    env.reset()
    view = env.task.get_robot()
    m = view.model
    write_state(view, random_state(m, n, view.env_origins, seed=17))
    st = read_state(view)
    tau = np.random.default_rng(3).uniform(-5, 5, size=(n, view.num_dof)).astype(np.float32)
    first = outputs(view, tau)
    idx = np.arange(0, n, 3)
    g = np.random.default_rng(9)
    damp = (view.get_joint_dampings().cpu().numpy()[idx] * g.uniform(0.5, 2, size=(len(idx), m.num_dof))
            + g.uniform(0.1, 1, size=(len(idx), m.num_dof))).astype(np.float32)
    view.set_joint_dampings(torch.from_numpy(damp).cuda(), indices=torch.from_numpy(idx).cuda())
    if name != "Cartpole":         # the analytic cart-pole has no armature
        arm = (view.get_armatures().cpu().numpy()[idx] * g.uniform(0.5, 2, size=(len(idx), m.num_dof))
               + g.uniform(0.01, 0.05, size=(len(idx), m.num_dof))).astype(np.float32)
        view.set_armatures(torch.from_numpy(arm).cuda(), indices=torch.from_numpy(idx).cuda())
    got = outputs(view, tau)
    same = np.ones(n, bool)
    same[idx] = False
    for k in first:
        moved = np.array([not np.array_equal(got[k][e], first[k][e]) for e in range(n)])
        if k.endswith("_armature") and name == "Cartpole" and k.startswith("solve"):
            assert not moved.any(), k               # only the damping changed: mode "armature" ignores it
        else:
            assert np.array_equal(moved, ~same), (k, np.flatnonzero(moved != ~same))
    kw = dict(damping=view.get_joint_dampings().cpu().numpy(),
              armature=None if name == "Cartpole" else view.get_armatures().cpu().numpy())
    rhs = rhs_of(n, 7, view.num_gen_vel)
    for mode in MODES:
        r64, r32 = refs(view, st, mode, **kw)
        check(f"{name} per-env table solve {mode}", got[f"solve_{mode}"], r32.solve(rhs), r64.solve(rhs))
        check(f"{name} per-env table fd {mode}", got[f"fd_{mode}"], r32.forward_dynamics(tau), r64.forward_dynamics(tau))
    torch.cuda.synchronize()
    view.clear_env_params()
    back = outputs(view, tau)
    for k in first:
        assert np.array_equal(back[k], first[k]), k
    env.close()


_CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, {root!r})
from omniisaacgymenvs_amd.utils.task_util import make_env
from tests.test_gpu_link_view import write_state
from tests.test_gpu_msolve import outputs
d = dict(np.load({state!r}))
tau = d.pop("tau")
env = make_env({name!r}, num_envs=d["q"].shape[0], device="cuda:0", seed=11)
env.reset()
view = env.task.get_robot()
write_state(view, d)
got = outputs(view, tau)
np.savez({out!r}, path=view.sim_kernel_path()[0], **got)
env.close()
"""


@pytest.mark.parametrize("name", ["Humanoid", "Ant"])
def test_both_state_layouts(gpu, name, tmp_path):
    """The same state on the default sim (paired kernels) and on an MI_WAVE_PAIR=0 sim in a fresh
    child process (per-env records): identical bits."""
    n = 64
    env = make_env(name, num_envs=n, device="cuda:0", seed=11)
    env.reset()
    view = env.task.get_robot()
    st = random_state(view.model, n, view.env_origins, seed=31)
    tau = np.random.default_rng(3).uniform(-5, 5, size=(n, view.num_dof)).astype(np.float32)
    write_state(view, st)
    here = outputs(view, tau)
    path = view.sim_kernel_path()[0]
    env.close()
    np.savez(tmp_path / "state.npz", tau=tau, **st)
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT, state=str(tmp_path / "state.npz"), name=name, out=str(tmp_path / "out.npz")))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, MI_WAVE_PAIR="0"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    there = np.load(tmp_path / "out.npz")
    assert int(there["path"]) == 1 and path != 1, (path, int(there["path"]))
    for k in here:
        assert np.array_equal(here[k], there[k]), k


@pytest.mark.parametrize("name", ["Humanoid", "Cartpole"])
def test_deferred_substeps_are_flushed(gpu, name):
    n = 33
    env = make_env(name, num_envs=n, device="cuda:0", seed=23)
    env.reset()
    view = env.task.get_robot()
    gen = torch.Generator().manual_seed(4)
    for _ in range(3):
        env.step((torch.rand((n, env.num_actions), generator=gen) * 2 - 1).cuda())
    before = read_state(view)
    links, offs = frames(view, "one")
    for call in (lambda: forward(view, 1), lambda: solve(view, 1, rhs_of(n, 2, view.num_gen_vel)),
                 lambda: task(view, 1, links, offs)):
        for _ in range(3):
            view.sim_step(1)                                # deferred
        rc, a = call()                                      # must issue them first
        st = read_state(view)                               # (this would, too)
        rc2, b = call()
        assert rc == 0 and rc2 == 0
        for x, y in zip(*(v.values() if isinstance(v, dict) else [v] for v in (a, b))):
            assert np.array_equal(x, y)
        assert not np.array_equal(st["q"], before["q"])
        before = st
    env.close()


def test_capture_and_python_surface(case):
    view, m, n, nv = case["view"], case["model"], case["n"], case["view"].num_gen_vel
    lib, h = N.lib(), view.handle
    links, offs = frames(view, "all")
    Q = 6 * len(links)
    rhs = torch.from_numpy(rhs_of(n, 7, nv)).cuda()
    tau = torch.from_numpy(case["tau"]).cuda()
    x, acc, mj, lam = (torch.zeros(s, device="cuda:0") for s in ((n, 7, nv), (n, nv), (n, Q, nv), (n, Q, Q)))

    def call():
        st = view.stream()
        assert lib.mi_solve_mass(h, 1, rhs.data_ptr(), 7, x.data_ptr(), st) == 0
        assert lib.mi_get_forward_dynamics(h, 0, None, acc.data_ptr(), st) == 0
        assert lib.mi_get_link_task_inertia(h, 1, N.iptr(links), N.fptr(offs), len(links), mj.data_ptr(), lam.data_ptr(), st) == 0

    call()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (x, acc, mj, lam)]
    # the Python surface: what the raw calls return
    assert torch.equal(view.solve_mass_matrices(rhs), eager[0])
    assert torch.equal(view.solve_mass_matrices(rhs[:, 0]), eager[0][:, 0])
    assert torch.equal(view.get_forward_dynamics(mode="armature"), eager[1])
    assert torch.equal(view.get_forward_dynamics(tau, mode="armature"), eager[1])
    pm, pl = view.get_task_space_inertias()
    assert torch.equal(pm, eager[2]) and torch.equal(pl, eager[3])
    one = view.get_task_space_inertias([m.body_names[-1]], mode="armature")
    assert one[0].shape == (n, 6, nv) and one[1].shape == (n, 6, 6)
    idx = torch.tensor([n - 1, 0, n // 2], device="cuda:0")
    assert torch.equal(view.get_forward_dynamics(mode="armature", indices=idx), eager[1][idx])
    a, b, cl = (view.get_forward_dynamics(clone=False), view.get_forward_dynamics(clone=False), view.get_forward_dynamics())
    assert a.data_ptr() == b.data_ptr() != cl.data_ptr() and torch.equal(a, cl)
    a, b = view.solve_mass_matrices(rhs, clone=False), view.solve_mass_matrices(rhs, clone=False)
    assert a.data_ptr() == b.data_ptr() != rhs.data_ptr()
    with pytest.raises(ValueError):
        view.solve_mass_matrices(rhs, mode="bare")
    with pytest.raises(ValueError):
        view.solve_mass_matrices(rhs[:, :, :-1])
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    for _ in range(3):
        view.solve_mass_matrices(rhs, clone=False)
        view.get_forward_dynamics(clone=False)
        view.get_task_space_inertias(clone=False)
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
        replayed = [t.cpu().numpy().copy() for t in (x, acc, mj, lam)]
        for t in (x, acc, mj, lam):
            t.zero_()
        call()
        torch.cuda.synchronize()
        for r, t in zip(replayed, (x, acc, mj, lam)):
            assert np.array_equal(r, t.cpu().numpy())
        assert not np.array_equal(replayed[0], eager[0].cpu().numpy())      # the state did change
    finally:
        write_state(view, case["st"])
        torch.cuda.synchronize()
