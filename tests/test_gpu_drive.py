"""Implicit PD joint drives on the GPU (include/mi_sim.h mi_set_drive_gains / mi_set_drive_targets /
mi_get_drives / mi_clear_drives, ArticulationView.set_gains / set_joint_position_targets / ...).

The main check is exact: a sim with drives steps to the SAME BITS as a twin without drives whose
damping record holds mi_drive_damping and whose efforts hold mi_drive_effort (include/mi_drive.h),
formed in torch float32 in the header's order from the same values and the twin's current q, with
contacts and joint-limit rows active, on the paired kernels (both solvers) and the one-lane kernel.

Against float64 (tests/drive_ref.py), one contact-free, limit-free substep in flight. The bound is
measured, not fixed: e0 = max |u+ - u+_64| of the drive-free substep of the same build on the same
states (the parent's code path: table present, no drive records); the drive may miss by 4 e0, one
more product and sum entering rhs and diag. The gains there are sized so that F_d is of the size of
the efforts (|tau| <= 5): the error scales with the right-hand side, and e0 is measured at that
scale. Likewise |u+ - (u + dt get_forward_dynamics("stepper"))| under a drive against 4 x the same
mismatch without one. Measured: test_one_substep_against_float64's docstring and DESIGN.md section 2.

Every check prints its figures (pytest -s)."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.robots.articulations import ArticulationView
from omniisaacgymenvs_amd.utils.task_util import make_env
from tests import drive_ref as ref
from tests.helpers import rand_actions
from tests.link_ref import random_state
from tests.msolve_ref import MassSolve
from tests.test_gpu_dyn_view import _u, sim_gravity
from tests.test_gpu_link_view import read_state, write_state
from tests.test_gpu_msolve import check as ms_check
from tests.test_gpu_msolve import rhs_of
from tests.test_gpu_pairing import _loads, _restore, _snap, _step
from tests.test_gpu_wrench import flight_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_ARG, E_STATE = -1, -2, -5, -7
SELF = "task.sim.Humanoid.enable_self_collisions=True"
# N = 34: two full 16-env workgroups of the paired kernels and a partial one; N = 2: one wave
SHAPES = [("Ant", 34, ["solver_type=0"]), ("Humanoid", 34, [SELF]), ("Ant", 2, [])]
IDS = ["Ant-34-pgs", "Humanoid-34-self-tgs", "Ant-2-tgs"]


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()


def drives(model, n, seed, kp_hi=400.0, kd_hi=4.0):
    """Gains and targets that differ per env and DOF: some entries kp = 0, some kd = 0, env 0 all
    zeros (where n > 1); targets inside the joint limits."""
    g = np.random.default_rng(seed)
    D = model.num_dof
    lo, hi = model.lower[1:].astype(np.float64), model.upper[1:].astype(np.float64)
    free = lo >= hi
    lo, hi = np.where(free, -0.5, lo), np.where(free, 0.5, hi)
    kp = g.uniform(0.1 * kp_hi, kp_hi, (n, D))
    kd = g.uniform(0.1 * kd_hi, kd_hi, (n, D))
    kp[g.random((n, D)) < 0.2] = 0.0
    kd[g.random((n, D)) < 0.2] = 0.0
    kp[-1, 0], kd[-1, -1] = 0.0, 0.0
    if n > 1:
        kp[0], kd[0] = 0.0, 0.0
    qt = lo + (hi - lo) * g.uniform(0.2, 0.8, (n, D))
    qdt = g.uniform(-0.5, 0.5, (n, D))
    assert np.all((qt > lo) & (qt < hi))
    return tuple(x.astype(np.float32) for x in (kp, kd, qt, qdt))


def set_drives(view, kp, kd, qt, qdt):
    view.set_gains(dev(kp), dev(kd))
    view.set_joint_position_targets(dev(qt))
    view.set_joint_velocity_targets(dev(qdt))


def get_drives(view):
    out = [torch.full((view.count, view.num_dof), float("nan"), device="cuda:0") for _ in range(4)]
    assert N.lib().mi_get_drives(view.handle, *[t.data_ptr() for t in out], view.stream()) == 0
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rail(n=5):
    """The Cartpole's link tree as a fixed-base articulation on the one-lane-per-env kernels, as
    tests/test_gpu_wrench.py::test_fixed_base_on_the_one_lane_path builds it."""
    src = make_env("Cartpole", num_envs=n, device="cuda:0", seed=2)
    sp = N.MiSimParams.from_buffer_copy(src.task.get_robot().sim_params)
    model = dataclasses.replace(src.task.get_robot().model, dyn_kind=N.MI_DYN_ARTICULATION)
    origins = np.array(src.task.get_robot().env_origins, np.float32)
    src.close()
    sp.angular_damping = 0.0

    def make():
        view = ArticulationView(model, name="rail")
        view.initialize(sp, n, origins, "cuda:0", seed=2)
        assert view.sim_kernel_path()[0] == 0 and not model.root_free
        st = random_state(model, n, origins, seed=4)
        st["q"][:] *= 0.1
        write_state(view, st)
        return view
    return make


def grounded_pair(name, n, ov):
    """Two sims from one seed, stepped to the ground by the same actions, then given the same state
    with one joint of the last env pushed onto its lower limit."""
    envs = [make_env(name, num_envs=n, device="cuda:0", seed=21, overrides=ov) for _ in range(2)]
    for env in envs:
        env.reset()
        for k in range(30):
            env.step(rand_actions(n, env.num_actions, 300 + k).cuda())
    va, vb = (env.task.get_robot() for env in envs)
    assert va.sim_kernel_path()[0] == 2
    st = read_state(va)
    m = va.model
    j = int(np.argmax(m.lower[1:] < m.upper[1:]))
    st["q"][-1, j] = m.lower[1 + j] + 1e-4
    st["qd"][-1, j] = -2.0
    for v in (va, vb):
        write_state(v, st)
    return envs, va, vb


def limit_rows(model, st, dt):
    lo, hi = model.lower[1:], model.upper[1:]
    q, qp = st["q"], st["q"] + np.float32(dt) * st["qd"]
    return (lo < hi) & ((q < lo) | (qp < lo) | (q > hi) | (qp > hi))


def snapshot(view):
    st = read_state(view)
    if view.num_sensors:
        st["sens"] = view._physics_view.get_force_sensor_forces().cpu().numpy().copy()
    return st


def twin_inputs(view_b, damp0, kp, kd, qt, qdt, tau, dt):
    """B's damping record and efforts from A's drive, in torch float32 in the header's order; the
    numpy restatement gives the same bits."""
    q = view_b.get_joint_positions()
    t = lambda a: dev(a)
    be = (t(damp0) + t(kd)) + torch.tensor(np.float32(dt)) * t(kp)
    eff = (t(tau) + t(kp) * (t(qt) - q)) + t(kd) * t(qdt)
    assert np.array_equal(bits(be.cpu().numpy()), bits(ref.drive_damping(damp0, kp, kd, np.float32(dt))))
    assert np.array_equal(bits(eff.cpu().numpy()), bits(ref.drive_effort(tau, kp, kd, q.cpu().numpy(), qt, qdt)))
    return be, eff


def run_twins(tag, va, vb, n, steps=8, contacts=None):
    m, dt = va.model, float(va.sim_params.dt)
    kp, kd, qt, qdt = drives(m, n, 7)
    tau = np.random.default_rng(8).uniform(-5, 5, (n, m.num_dof)).astype(np.float32)
    damp0 = vb.get_joint_dampings().cpu().numpy()
    set_drives(va, kp, kd, qt, qdt)
    va.set_joint_efforts(dev(tau))
    assert np.array_equal(va.get_joint_dampings().cpu().numpy(), damp0)     # kd is not the damping slot
    moved = 0.0
    for step in range(steps):
        be, eff = twin_inputs(vb, damp0, kp, kd, qt, qdt, tau, dt)
        if step == 0:
            vb.set_joint_dampings(be)
        vb.set_joint_efforts(eff)
        before = read_state(va)
        va.sim_step(1)
        vb.sim_step(1)
        a, b = snapshot(va), snapshot(vb)
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), (tag, step, k, float(np.abs(a[k] - b[k]).max()))
        moved = max(moved, float(np.abs(a["qd"] - before["qd"]).max()))
    print(f"{tag}: {steps} single substeps equal bit for bit; max |dqd| per substep {moved:.3e}")
    assert moved > 1e-3 and np.isfinite(a["q"]).all()


@pytest.mark.parametrize("name,n,ov", SHAPES, ids=IDS)
def test_the_step_equals_its_twin_bit_for_bit(gpu, name, n, ov):
    envs, va, vb = grounded_pair(name, n, ov)
    st, dt = read_state(va), float(va.sim_params.dt)
    cnt = va.get_contact_data()[0].cpu().numpy()
    rows = limit_rows(va.model, st, dt)
    print(f"{name}-{n}: envs in contact {int((cnt > 0).sum())}/{n}, contacts {int(cnt.sum())}, limit rows {int(rows.sum())}")
    assert (cnt > 0).any() and rows[-1].any()                  # in contact, and a limit row is active
    run_twins(f"{name}-{n}", va, vb, n)
    for env in envs:
        env.close()


def test_the_step_equals_its_twin_on_the_one_lane_path(gpu):
    make = rail()
    va, vb = make(), make()
    run_twins("rail", va, vb, va.count)
    va.close()
    vb.close()


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def case(request, gpu):
    name, n, ov = request.param
    env = make_env(name, num_envs=n, device="cuda:0", seed=11, overrides=ov)
    env.reset()
    view = env.task.get_robot()
    assert view.sim_kernel_path()[0] == 2
    write_state(view, random_state(view.model, n, view.env_origins, seed=17))
    tau = np.random.default_rng(3).uniform(-5, 5, size=(n, view.num_dof)).astype(np.float32)
    view.set_joint_efforts(dev(tau))
    yield dict(name=name, n=n, env=env, view=view, model=view.model, st=read_state(view), tau=tau, tag=f"{name}-{n}")
    env.close()


def ms_outputs(view):
    """Every output of the mass-solve family, both modes."""
    nv = view.num_gen_vel
    rhs = dev(rhs_of(view.count, 3, nv))
    out = {}
    for mode in ("stepper", "armature"):
        out[f"solve {mode}"] = view.solve_mass_matrices(rhs, mode=mode).cpu().numpy()
        out[f"fd {mode}"] = view.get_forward_dynamics(mode=mode).cpu().numpy()
        for k, t in zip(("minv_jt", "lam_inv"), view.get_task_space_inertias([view.body_names[-1]], mode=mode)):
            out[f"{k} {mode}"] = t.cpu().numpy()
    return out


def test_readback_indexing_and_views(case):
    """Readback (zeros before any call, idx in i64 and i32, partial pointers, clear by index, the
    same bits back) and the mass-solve views under a drive, on one sim per shape: the "before any
    drive call" outputs need a sim that never had one."""
    view, m, n, st = case["view"], case["model"], case["n"], case["st"]
    D, dt = m.num_dof, float(view.sim_params.dt)
    before = ms_outputs(view)
    assert not any(a.any() for a in get_drives(view))                        # zeros before any call
    view.clear_joint_drives()                                                # and nothing to clear
    kp, kd, qt, qdt = drives(m, n, 5)
    set_drives(view, kp, kd, qt, qdt)
    for got, want in zip(get_drives(view), (kp, kd, qt, qdt)):
        assert np.array_equal(bits(got), bits(want))
    for got, want in zip(view.get_gains() + (view.get_joint_position_targets(), view.get_joint_velocity_targets()),
                         (kp, kd, qt, qdt)):
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    # ---- the views under the drive
    BE = ref.drive_damping(m.damping[1:], kp, kd, np.float32(dt))
    g = sim_gravity(view)
    r64 = MassSolve(m, st, dt, "stepper", gravity=g, damping=BE.astype(np.float64))
    r32 = MassSolve(m, st, dt, "stepper", gravity=g, damping=BE, dtype=np.float32)
    under = ms_outputs(view)
    rhs = rhs_of(n, 3, view.num_gen_vel)
    ms_check(f"{case['tag']} solve stepper under a drive", under["solve stepper"], r32.solve(rhs), r64.solve(rhs))
    links, offs = view._frames([view.body_names[-1]])
    (_, X64, L64), (_, X32, L32) = r64.task(links, offs), r32.task(links, offs)
    ms_check(f"{case['tag']} minv_jt stepper under a drive", under["minv_jt stepper"], X32, X64)
    ms_check(f"{case['tag']} lam_inv stepper under a drive", under["lam_inv stepper"], L32, L64)
    assert not np.array_equal(under["solve stepper"], before["solve stepper"])
    for k in ("solve armature", "minv_jt armature", "lam_inv armature"):      # continuous time: the same matrix
        assert np.array_equal(bits(under[k]), bits(before[k])), k
    # forward dynamics: B_E u and tau + F_d (stepper); B + kd and tau + F_d (armature)
    eff = ref.drive_effort(case["tau"], kp, kd, st["q"], qt, qdt)
    ms_check(f"{case['tag']} fd stepper under a drive", under["fd stepper"],
             r32.forward_dynamics(eff), r64.forward_dynamics(eff.astype(np.float64)))
    Bc = ref.drive_damping(m.damping[1:], 0 * kp, kd, np.float32(dt))
    a64 = MassSolve(m, st, dt, "armature", gravity=g, damping=Bc.astype(np.float64))
    a32 = MassSolve(m, st, dt, "armature", gravity=g, damping=Bc, dtype=np.float32)
    ms_check(f"{case['tag']} fd armature under a drive", under["fd armature"],
             a32.forward_dynamics(eff), a64.forward_dynamics(eff.astype(np.float64)))
    # ---- indexing: a strict subset out of order, an id out of range (ignored), i64 and i32 ids
    idx = np.array([n - 1, 0, n + 5], np.int64) if n > 2 else np.array([1, 7], np.int64)
    named = [int(i) for i in idx if i < n]
    rows = [r for r, i in enumerate(idx) if i < n]
    others = [i for i in range(n) if i not in named]
    k2, d2, q2, v2 = drives(m, len(idx), 6)
    view.set_gains(dev(k2), None, indices=dev(idx, torch.int64))             # kp only
    view.set_joint_position_targets(dev(q2), indices=dev(idx, torch.int32))  # q* only, i32 ids
    got = get_drives(view)
    for g_, old, new in zip(got, (kp, kd, qt, qdt), (k2, None, q2, None)):
        assert np.array_equal(bits(g_[others]), bits(old[others]))
        assert np.array_equal(bits(g_[named]), bits(old[named] if new is None else new[rows]))
    # refused calls write nothing
    lib, h, s = N.lib(), view.handle, view.stream()
    t = dev(k2)
    assert lib.mi_set_drive_gains(h, None, None, None, n, s) == E_NULL and b"both null" in lib.mi_last_error()
    assert lib.mi_set_drive_targets(h, None, None, None, n, s) == E_NULL
    assert lib.mi_set_drive_gains(h, t.data_ptr(), None, None, n + 1, s) == E_SHAPE
    assert lib.mi_set_drive_targets(h, t.data_ptr(), None, None, -1, s) == E_SHAPE
    assert lib.mi_clear_drives(h, None, n + 1, s) == E_SHAPE
    for a, b in zip(get_drives(view), got):
        assert np.array_equal(bits(a), bits(b))
    # clear by index, then everything: exact zeros, and the views are back at their first bits
    view.clear_joint_drives(indices=dev(idx, torch.int64))
    for g_, old in zip(get_drives(view), got):
        assert not g_[named].any() and np.array_equal(bits(g_[others]), bits(old[others]))
    view.clear_joint_drives()
    assert not any(a.any() for a in get_drives(view))
    after = ms_outputs(view)
    for k in before:
        assert np.array_equal(bits(after[k]), bits(before[k])), k


def test_substeps_re_evaluate_the_spring(gpu):
    """sim_step(2) in one launch == two sim_step(1) launches (the coalescing contract), and both
    differ from the twin whose efforts were frozen over the two substeps."""
    name, n, ov = SHAPES[0]
    outs = {}
    for mode in ("one launch", "two launches", "frozen"):
        env, view = flight_env(name, n, ov)
        m, dt = view.model, float(view.sim_params.dt)
        kp, kd, qt, qdt = drives(m, n, 7)
        tau = np.zeros((n, m.num_dof), np.float32)
        if mode == "frozen":
            damp0 = view.get_joint_dampings().cpu().numpy()
            be, eff = twin_inputs(view, damp0, kp, kd, qt, qdt, tau, dt)
            view.set_joint_dampings(be)
            view.set_joint_efforts(eff)
        else:
            set_drives(view, kp, kd, qt, qdt)
            view.set_joint_efforts(dev(tau))
        if mode == "two launches":
            view.sim_step(1)
            read_state(view)                        # a getter issues the deferred substep: its own launch
            view.sim_step(1)
        else:
            view.sim_step(2)
        outs[mode] = read_state(view)
        env.close()
    for k in outs["one launch"]:
        assert np.array_equal(bits(outs["one launch"][k]), bits(outs["two launches"][k])), k
    d = float(np.abs(outs["one launch"]["qd"] - outs["frozen"]["qd"]).max())
    print(f"{name}-{n}: frozen efforts differ from the drive by {d:.3e} in qd after two substeps")
    assert d > 1e-4


@pytest.mark.parametrize("name,n,ov", SHAPES, ids=IDS)
def test_one_substep_against_float64(gpu, name, n, ov):
    """Bound 4 e0 (module docstring). Measured on one MI355X, e0 then the error under a drive: Ant 34
    PGS 9.806e-07, 1.002e-06; Humanoid 34 TGS 2.858e-05, 3.916e-05; Ant 2 TGS 2.731e-07, 2.461e-07.
    |u+ - (u + dt get_forward_dynamics("stepper"))| without, then with a drive (bound 4 x the
    former): 8.743e-07, 7.848e-07; 2.815e-05, 3.858e-05; 3.514e-07, 3.514e-07."""
    res = {}
    for with_drive in (False, True):
        env, view = flight_env(name, n, [o for o in ov if o != SELF])
        m, dt = view.model, float(view.sim_params.dt)
        tau = np.random.default_rng(2).uniform(-5, 5, size=(n, m.num_dof)).astype(np.float32)
        view.set_joint_efforts(dev(tau))
        view.set_armatures(view.get_armatures())             # the table, nominal values: the EnvP kernels
        kp, kd, qt, qdt = drives(m, n, 9, kp_hi=20.0, kd_hi=1.0)
        if with_drive:
            set_drives(view, kp, kd, qt, qdt)
        else:
            kp, kd = 0 * kp, 0 * kd
        st0 = read_state(view)
        fd = view.get_forward_dynamics(mode="stepper").cpu().numpy().astype(np.float64)
        view.sim_step(1)
        u0, u1 = _u(st0), _u(read_state(view))
        u64 = ref.implicit_substep(m, st0, dt, tau, kp, kd, qt, qdt, gravity=sim_gravity(view))
        res[with_drive] = (st0, float(np.abs(u1 - u64).max()), float(np.abs(u1 - (u0 + dt * fd)).max()), u1)
        lo, hi = m.lower[1:], m.upper[1:]
        qp = st0["q"] + dt * np.maximum(np.abs(u0[:, 6:]), np.abs(u1[:, 6:])) * np.array([[-1.0], [1.0]])[:, None]
        assert np.all((lo >= hi) | ((qp.min(0) > lo) & (qp.max(0) < hi))), "a limit row fired: choose smaller gains"
        env.close()
    (sa, e0, f0, ua), (sb, e1, f1, ub) = res[False], res[True]
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k                # the same start
    print(f"{name}-{n}: against float64 e0 {e0:.3e}, under a drive {e1:.3e} (bound {4 * e0:.3e}); "
          f"|u+ - (u + dt fd)| without {f0:.3e}, with {f1:.3e} (bound {4 * f0:.3e}); the drive moves u+ by {np.abs(ub - ua).max():.3e}")
    assert np.abs(ub - ua).max() > 100 * e0                   # the drive did act
    assert e1 <= 4.0 * e0 and f1 <= 4.0 * f0


def test_it_holds_a_pose(gpu):
    """Ant in flight, per-env gravity 0, zero velocity, q* = q + 0.1 on every joint, kd = 0 and
    dt^2 kp = 10 x the largest diagonal entry of the mass matrix (above 8 x: an explicit spring cannot
    be stable there). Substeps until max |q - q*| < 1 % of 0.1: the float64 reference and the device
    print their counts; the device may take 1.5 x the reference's. Measured on one MI355X: kp 1.322e+05,
    max diag M 0.911; float64 1 substep, device 1 (allowed 2)."""
    n, delta = 2, 0.1
    env, view = flight_env("Ant", n, [], moving=False)
    m, dt = view.model, float(view.sim_params.dt)
    view.set_env_gravity(torch.zeros((n, 3)))
    st = read_state(view)
    Mdiag = float(torch.diagonal(view.get_mass_matrices(), dim1=1, dim2=2).max())
    kp = np.full((n, m.num_dof), 10.0 * Mdiag / dt ** 2, np.float32)
    assert dt * dt * float(kp[0, 0]) > 8.0 * Mdiag
    qt = (st["q"] + np.float32(delta)).astype(np.float32)
    assert np.all((qt > m.lower[1:]) & (qt < m.upper[1:]))
    tol = 0.01 * delta
    errs = ref.hold_pose(m, st, dt, kp, 0.0, qt, 200, tol=tol)
    assert errs[-1] < tol, errs[-5:]
    want = len(errs)
    allowed = int(np.ceil(1.5 * want))
    view.set_gains(dev(kp), dev(0 * kp))
    view.set_joint_position_targets(dev(qt))
    got = None
    for k in range(allowed):
        view.sim_step(1)
        e = float(np.abs(read_state(view)["q"] - qt).max())
        assert view.nan_count() == 0
        if e < tol:
            got = k + 1
            break
    print(f"hold a pose: kp {kp[0, 0]:.3e}, max diag M {Mdiag:.3e}; substeps to 1 %: float64 {want}, device {got} (allowed {allowed})")
    assert got is not None
    env.close()


def test_record_follows_the_env_under_pairing_by_load(gpu):
    env = make_env("Humanoid", num_envs=32, device="cuda:0", seed=5)
    view = env.task.get_robot()
    kp, kd, qt, qdt = drives(view.model, 32, 12, kp_hi=100.0, kd_hi=2.0)
    set_drives(view, kp, kd, qt, qdt)
    env.reset()
    for k in range(3):
        _step(env, rand_actions(32, env.num_actions, 50 + k).cuda())
    snap = _snap(env)
    acts = rand_actions(32, env.num_actions, 60).cuda()
    # keys that rank every workgroup's envs so that partners are non-adjacent slots
    keys = np.tile(np.array([40, 1, 2, 39, 3, 4, 38, 5, 6, 37, 7, 8, 36, 9, 10, 35], np.int32), 2)
    outs = []
    for pairing in (0, 1):
        _restore(env, snap)
        _loads(view, keys, pairing)
        outs.append(_step(env, acts))
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)
    env.close()


@pytest.mark.parametrize("name", ["Ant", "Humanoid"])
def test_fused_equals_modular_under_a_drive(gpu, name):
    n = 34
    ea = make_env(name, num_envs=n, device="cuda:0", seed=13)
    eb = make_env(name, num_envs=n, device="cuda:0", seed=13)
    eb.use_fused(False)
    assert ea.fused and not eb.fused
    kp, kd, qt, qdt = drives(ea.task.get_robot().model, n, 14, kp_hi=100.0, kd_hi=2.0)
    for env in (ea, eb):
        env.reset()
        set_drives(env.task.get_robot(), kp, kd, qt, qdt)
    undriven = make_env(name, num_envs=n, device="cuda:0", seed=13)
    undriven.reset()
    for step in range(3):
        acts = rand_actions(n, ea.num_actions, step).to("cuda:0")
        oa, ra, da, _ = ea.step(acts)
        ob, rb, db, _ = eb.step(acts)
        oc, _, _, _ = undriven.step(acts)
        torch.cuda.synchronize()
        np.testing.assert_allclose(oa["obs"].cpu().numpy(), ob["obs"].cpu().numpy(), rtol=1e-5, atol=1e-5, err_msg=f"{name} step {step}")
        np.testing.assert_allclose(ra.cpu().numpy(), rb.cpu().numpy(), rtol=1e-5, atol=1e-5)
        assert torch.equal(da, db)
    assert np.abs(oa["obs"].cpu().numpy() - oc["obs"].cpu().numpy()).max() > 1e-3     # the drive is felt
    for env in (ea, eb, undriven):
        env.close()


def test_off_means_off(gpu):
    """Two sims with the table; one set drives and cleared them: identical bits after stepping."""
    n = 34
    envs = [make_env("Humanoid", num_envs=n, device="cuda:0", seed=7) for _ in range(2)]
    for k, env in enumerate(envs):
        env.reset()
        view = env.task.get_robot()
        view.set_armatures(view.get_armatures())
        if k:
            set_drives(view, *drives(view.model, n, 15))
            assert get_drives(view)[0].any()
            view.clear_joint_drives()
    for step in range(3):
        acts = rand_actions(n, envs[0].num_actions, 40 + step).cuda()
        outs = [env.step(acts) for env in envs]
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0]["obs"], outs[1][0]["obs"]) and torch.equal(outs[0][1], outs[1][1])
    a, b = (read_state(env.task.get_robot()) for env in envs)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    for env in envs:
        env.close()


def test_graph_capture(gpu):
    n = 32
    ea = make_env("Ant", num_envs=n, device="cuda:0", seed=23)
    eb = make_env("Ant", num_envs=n, device="cuda:0", seed=23)
    m = ea.task.get_robot().model
    kp, kd, qt, qdt = drives(m, n, 16, kp_hi=100.0, kd_hi=2.0)
    targets = [dev(drives(m, n, 17 + k)[2]) for k in range(3)]
    acts = [rand_actions(n, ea.num_actions, 90 + k).cuda() for k in range(3)]
    ea.step(acts[0]); eb.step(acts[0])                        # warm-up outside the capture
    va, vb = ea.task.get_robot(), eb.task.get_robot()
    lib = N.lib()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # the first call allocates: refused inside a capture, and nothing is captured
        torch.cuda.synchronize()
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s):
            targets[0].mul_(1.0)                              # (a graph with one node)
            rc = lib.mi_set_drive_targets(va.handle, targets[0].data_ptr(), None, None, n, va.stream())
        assert rc == E_STATE and b"before the capture" in lib.mi_last_error()
    torch.cuda.synchronize()
    assert not any(a.any() for a in get_drives(va))
    for v in (va, vb):
        v.set_gains(dev(kp), dev(kd))                         # eager first use
    ea.step(acts[0]); eb.step(acts[0])                        # and the table-reading kernels' first launch
    ta, tb = ea.task, eb.task
    cur = targets[0].clone()
    out = tuple(torch.empty_like(t) for t in (ta.obs_buf, ta.rew_buf, ta.reset_buf))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            va.set_joint_position_targets(cur)
            ta.fused_step(acts[1], out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in range(3):
        cur.copy_(targets[k])                                 # new target values in place
        g.replay()
        torch.cuda.synchronize()
        vb.set_joint_position_targets(targets[k])
        eo = tuple(torch.empty_like(t) for t in out)
        tb.fused_step(acts[1], out=eo)
        torch.cuda.synchronize()
        for a, b in zip(out, eo):
            assert torch.equal(a, b), k
    a, b = read_state(va), read_state(vb)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(bits(get_drives(va)[2]), bits(targets[2].cpu().numpy()))
    ea.close()
    eb.close()


_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, {root!r})
from omniisaacgymenvs_amd.utils.task_util import make_env
env = make_env("Ant", num_envs=33, device="cuda:0", seed=1)
view = env.task.get_robot()
assert view.sim_kernel_path()[0] == 1
try:
    view.set_gains(torch.zeros((33, view.num_dof), device="cuda:0"), None)
except RuntimeError as e:
    print("REFUSED", e)
assert not view.get_gains()[0].any()
env.close()
"""


def test_refusals(gpu, tmp_path):
    lib = N.lib()
    # odd N: the wavefront-per-env path has no per-env-table kernels (a fresh process)
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "REFUSED" in r.stdout and "(-7)" in r.stdout and "wavefront-per-env" in r.stdout, r.stdout
    env = make_env("Cartpole", num_envs=4, device="cuda:0", seed=1)
    cart = env.task.get_robot()
    z = torch.zeros((4, cart.num_dof), device="cuda:0")
    s = cart.stream()
    assert lib.mi_set_drive_gains(cart.handle, z.data_ptr(), None, None, 4, s) == E_ARG and b"cart-pole" in lib.mi_last_error()
    assert lib.mi_set_drive_targets(cart.handle, z.data_ptr(), None, None, 4, s) == E_ARG
    assert lib.mi_get_drives(cart.handle, z.data_ptr(), None, None, None, s) == E_ARG
    assert lib.mi_clear_drives(cart.handle, None, 4, s) == E_ARG
    env.close()
