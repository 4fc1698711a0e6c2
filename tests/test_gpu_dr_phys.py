"""GPU: per-env physics parameters and physics domain randomization (include/mi_sim.h
mi_set_env_params / mi_sim_set_phys_dr / mi_dr_phys_step).

The oracle is per sim, so env e of the device is checked against its own single-env OracleSim
(num_envs = 1, env id offset + e, origin row e) carrying env e's gravity and friction in its
MiSimParams and its damping / armature in a replaced CompiledModel, synced to the device state.

Ranges of test 1 (numpy generator 2024): gravity z nominal + U(-2, 2), gravity x, y U(-0.5, 0.5),
friction U(0.5, 1.25), damping nominal x logU(0.5, 2), armature nominal + U(0, 0.02). The shipped
Cartpole has zero nominal damping, which a scaling would leave at zero, so its damping is additive:
cart nominal + U(0.05, 0.5), pole nominal + U(0.002, 0.02) (and an additive uniform schedule with
the same bounds in the Cartpole leg of the schedule tests).

Checked on the CPU with the per-env twins alone (configs composed without a device, zero origins,
seed 31, the test's generator and actions): over the compared steps - and the three warm-up steps
the locomotion shapes take first, which bring more bodies into contact - all four shapes give no
NaN and no reset besides the initial one, so the ranges above are the final ones (the test asserts
it); with the Cartpole damping above instead of the nominal zero the observations move by up to
0.14 (tolerance 1e-4), so a kernel that ignored or swapped the two damping entries fails. Cartpole
takes no warm-up steps: with three of them 11 of its 64 envs reset inside the compared steps.
"""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.utils.task_util import make_env
from oracle.oracle import OracleSim, make_buffers
from tests import dr_phys_ref as ref
from tests.helpers import rand_actions, reset_counts, task_buffers
from tests.test_gpu_pairing import _loads, _restore, _snap, _step
from tests.test_gpu_parity import check_device_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRK = "task.domain_randomization"
RP = f"{DRK}.randomization_params"


def _nominal(view):
    m, sp = view.model, view.sim_params
    D = view.num_dof
    return {0: np.array(list(sp.gravity), np.float32), 1: np.array([sp.friction], np.float32),
            2: np.asarray(m.damping[1:1 + D], np.float32), 3: np.asarray(m.armature[1:1 + D], np.float32)}


def _params(view):
    """The table as numpy {attr: [N, dim]} (mi_get_env_params through the view getters)."""
    out = {0: view.get_env_gravity(), 2: view.get_joint_dampings()}
    if view.model.dyn_kind != N.MI_DYN_CARTPOLE:
        out[1], out[3] = view.get_friction_coefficients(), view.get_armatures()
    torch.cuda.synchronize()
    return {a: t.cpu().numpy() for a, t in out.items()}


def _twin(env, seed, e, prm):
    """Single-env oracle twin of env e with env e's parameters (not yet synced)."""
    task, view = env.task, env.task.get_robot()
    sp = N.MiSimParams.from_buffer_copy(view.sim_params)
    sp.gravity[:] = [float(x) for x in prm[0][e]]
    model = task.model
    D = view.num_dof
    if model.dyn_kind == N.MI_DYN_CARTPOLE:
        damping = np.array(model.damping, np.float32)
        damping[1:1 + D] = prm[2][e]
        model = dataclasses.replace(model, damping=damping, cartpole=dict(
            model.cartpole, cart_damping=float(prm[2][e][0]), pole_damping=float(prm[2][e][1])))
    else:
        sp.friction = float(prm[1][e][0])
        damping, armature = np.array(model.damping, np.float32), np.array(model.armature, np.float32)
        damping[1:1 + D], armature[1:1 + D] = prm[2][e], prm[3][e]
        model = dataclasses.replace(model, damping=damping, armature=armature)
    orc = OracleSim(model, sp, 1, task.env_pos_cpu[e:e + 1], seed=seed, env_id_offset=env.env_id_offset + e)
    orc.configure(task.task_params(), keep=task)
    return orc


def _step_against_twins(env, seed, acts, prm, name, tol, no_new_reset=False):
    """One fused device step; every env against its freshly synced single-env twin. Returns the
    device's (obs, rew, resets). no_new_reset: no env may reset that was not flagged coming in."""
    task, view = env.task, env.task.get_robot()
    n = task.num_envs
    torch.cuda.synchronize()
    p, q = view.get_world_poses()
    st = [t.cpu().numpy() for t in (p, q, view.get_velocities(), view.get_joint_positions(),
                                    view.get_joint_velocities())]
    rc = reset_counts(view)
    b = task_buffers(env)
    obs_dict, rew, resets, _ = env.step(acts.to("cuda:0"))
    torch.cuda.synchronize()
    O, A = task.num_observations, task.num_actions
    obs, rw, rs, margin = np.zeros((n, O), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int64), np.zeros(n)
    for e in range(n):
        orc = _twin(env, seed, e, prm)
        orc.set_root_state(st[0][e:e + 1], st[1][e:e + 1], st[2][e:e + 1])
        orc.set_dof_state(st[3][e:e + 1], st[4][e:e + 1])
        orc.set_reset_count(rc[e:e + 1])
        be = make_buffers(1, O, A)
        for k in ("reset", "progress", "pot", "prev"):
            if be.get(k) is not None and b.get(k) is not None:
                be[k][:] = b[k][e:e + 1]
        orc.env_step(acts.numpy()[e:e + 1], task.control_frequency_inv, be)
        obs[e], rw[e], rs[e] = be["obs"][0], be["rew"][0], be["reset"][0]
        margin[e] = orc.decision_margin()[0]
        orc.close()
    check_device_pair(name, obs_dict["obs"].cpu().numpy(), rew.cpu().numpy(), obs, rw, tol, margin)
    assert np.array_equal(resets.cpu().numpy(), rs), f"{name}: reset mismatch"
    assert np.isfinite(obs).all() and view.nan_count() == 0, f"{name}: non-finite state"
    if no_new_reset:
        assert not rs[b["reset"] == 0].any(), f"{name}: envs {np.nonzero(rs)[0]} reset inside the compared steps"
    return obs_dict["obs"].cpu().numpy(), rew.cpu().numpy(), resets.cpu().numpy()


def _random_params(view, g):
    nom, n, D = _nominal(view), view.count, view.num_dof
    grav = np.tile(nom[0], (n, 1))
    grav[:, 2] += g.uniform(-2, 2, n)
    grav[:, :2] = g.uniform(-0.5, 0.5, (n, 2))
    prm = {0: grav.astype(np.float32)}
    if view.model.dyn_kind == N.MI_DYN_CARTPOLE:   # zero nominal damping: additive (module docstring)
        prm[2] = (nom[2] + np.stack([g.uniform(0.05, 0.5, n), g.uniform(0.002, 0.02, n)], 1)).astype(np.float32)
    else:
        prm[2] = (nom[2] * np.exp(g.uniform(np.log(0.5), np.log(2.0), (n, D)))).astype(np.float32)
        prm[1] = g.uniform(0.5, 1.25, (n, 1)).astype(np.float32)
        prm[3] = (nom[3] + g.uniform(0, 0.02, (n, D))).astype(np.float32)
    return prm


def _set_params(view, prm, indices=None):
    view.set_env_gravity(torch.from_numpy(prm[0]), indices)
    view.set_joint_dampings(torch.from_numpy(prm[2]), indices)
    if 1 in prm:
        view.set_friction_coefficients(torch.from_numpy(prm[1]), indices)
        view.set_armatures(torch.from_numpy(prm[3]), indices)


@pytest.mark.parametrize("name,n,overrides", [
    ("Humanoid", 32, []), ("Humanoid", 34, ["solver_type=0"]), ("Ant", 32, []), ("Cartpole", 64, [])])
def test_setters_match_per_env_oracles(gpu, name, n, overrides):
    """Ranges: see the module docstring."""
    env = make_env(name, num_envs=n, device="cuda:0", seed=31, overrides=overrides)
    view = env.task.get_robot()
    if name != "Cartpole":
        assert view.sim_kernel_path()[0] == 2
    nom = _params(view)                                  # before the table: nominal, broadcast
    for a, v in _nominal(view).items():
        if a in nom:
            np.testing.assert_array_equal(nom[a], np.tile(v, (n, 1)))
    prm = _random_params(view, np.random.default_rng(2024))
    half = torch.arange(0, n, 2, device="cuda:0")
    _set_params(view, {a: v[::2] for a, v in prm.items()}, half)       # indexed, then the rest
    _set_params(view, {a: v[1::2] for a, v in prm.items()}, torch.arange(1, n, 2, device="cuda:0"))
    got = _params(view)
    for a in prm:
        np.testing.assert_array_equal(got[a], prm[a])
    env.reset()
    if name != "Cartpole":      # more bodies in contact in the compared steps (friction observable)
        for k in (3, 2, 1):
            env.step(rand_actions(n, env.num_actions, 300 - k).cuda())
    else:
        assert float(prm[2].min()) > 0.0
    for step in range(4):
        acts = rand_actions(n, env.num_actions, 300 + step)
        _step_against_twins(env, 31, acts, prm, name, 1e-4 if name == "Cartpole" else 2e-3, no_new_reset=True)
    env.close()


def test_table_is_read_by_the_kernels(gpu):
    """The same step with and without per-env gravity differs (a table the kernels ignored would
    pass a comparison of nominal twins)."""
    outs = []
    for with_table in (False, True):
        env = make_env("Ant", num_envs=32, device="cuda:0", seed=3)
        view = env.task.get_robot()
        if with_table:
            g = np.tile(np.array([0.0, 0.0, -4.0], np.float32), (32, 1))
            view.set_env_gravity(torch.from_numpy(g))
        env.reset()
        outs.append(_step(env, rand_actions(32, env.num_actions, 1).cuda())["obs"])
        env.close()
    assert not np.allclose(outs[0], outs[1], atol=1e-3)


def test_record_follows_the_env_under_pairing_by_load(gpu):
    env = make_env("Humanoid", num_envs=32, device="cuda:0", seed=5)
    view = env.task.get_robot()
    prm = _random_params(view, np.random.default_rng(7))
    _set_params(view, prm)
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


def _yaml_overrides():
    o = [f"+{DRK}.randomize=True", f"+{DRK}.min_frequency=2"]

    def sched(path, when, op, dist, params, freq=None):
        r = [f"+{RP}.{path}.{when}.operation={op}", f"+{RP}.{path}.{when}.distribution={dist}",
             f"+{RP}.{path}.{when}.distribution_parameters={params}"]
        return r + ([f"+{RP}.{path}.{when}.frequency_interval={freq}"] if freq else [])
    return o, sched


def _dr_overrides(view_name, cartpole=False):
    o, sched = _yaml_overrides()
    o += sched("simulation.gravity", "on_reset", "additive", "gaussian", "[0.0,0.4]")
    if cartpole:   # zero nominal damping: an additive schedule (cart, pole)
        o += sched(f"articulation_views.{view_name}.damping", "on_interval", "additive", "uniform",
                   "[[0.05,0.002],[0.5,0.02]]", 2)
    else:
        o += sched(f"articulation_views.{view_name}.damping", "on_interval", "scaling", "uniform", "[0.8,1.25]", 2)
    if not cartpole:
        o += sched(f"articulation_views.{view_name}.material_properties", "on_reset", "scaling", "uniform",
                   "[[1.0,0.7,1.0],[1.0,1.2,1.0]]")
    return o


VIEWS = {"Ant": "ant_view", "Humanoid": "humanoid_view", "Cartpole": "cartpole_view"}


def test_schedule_through_the_yaml(gpu):
    n, seed = 32, 19
    env = make_env("Ant", num_envs=n, device="cuda:0", seed=seed, overrides=_dr_overrides("ant_view"))
    task, view = env.task, env.task.get_robot()
    rnd = task._dr_randomizer
    assert set(rnd.active_domain_randomizations) == {
        ("simulation", "gravity", "on_reset"), ("articulation_views", "ant_view", "damping", "on_interval"),
        ("articulation_views", "ant_view", "material_properties", "on_reset")}
    nom = _nominal(view)
    D = view.num_dof
    f32 = lambda *v: np.array(v, np.float32)
    sched = {(0, "on_reset"): (0, 0, np.zeros(3, np.float32), np.full(3, 0.4, np.float32)),
             (1, "on_reset"): (1, 1, f32(0.7), f32(1.2)),
             (2, "on_interval"): (1, 1, np.full(D, 0.8, np.float32), np.full(D, 1.25, np.float32))}
    rs = ref.Schedule(nom, sched, 2, 2, seed, n)
    # env 3: resets at steps 2, 4, 6 (epochs 1..3), the request at step 3 is inside min_frequency
    forced = {2: [3, 4, 9], 3: [3], 4: [3], 5: [4, 31], 6: [3, 0], 7: [9]}
    for step in range(8):
        for e in forced.get(step, []):
            task.reset_buf[e] = 1
        torch.cuda.synchronize()
        rs.step(task.reset_buf.cpu().numpy())
        acts = rand_actions(n, env.num_actions, 700 + step)
        # the step randomizes first: the twins carry the values the restatement predicts, read back
        # from the device after the step (the table only changes in the schedule kernel)
        pre = _snap(env)
        ran = _step(env, acts.cuda())
        np.testing.assert_array_equal(view.phys_dr_state(), rs.state, err_msg=f"step {step}")
        got = _params(view)
        for a in nom:
            tol = rs.err[a] + 2.0 ** -24 * np.abs(rs.val[a])
            assert (np.abs(got[a] - rs.val[a]) <= tol).all(), (step, a, np.abs(got[a] - rs.val[a]).max())
        _restore(env, pre)
        saved = rs.state.copy()
        # the step that ran with the schedules on (schedule kernel, then the fused launch) equals,
        # bit for bit, the rerun from the same state on the table it left
        obs, rew, resets = _step_against_twins_no_dr(env, seed, acts, got, "Ant", 2e-3)
        for k, v in (("obs", obs), ("rew", rew), ("reset", resets)):
            np.testing.assert_array_equal(ran[k], v, err_msg=f"step {step} {k}")
        again = _snap(env)
        for k in ("q", "qd", "pos", "quat", "vel"):
            np.testing.assert_array_equal(ran[k], again[k].cpu().numpy(), err_msg=f"step {step} {k}")
        np.testing.assert_array_equal(view.phys_dr_state(), saved)
    assert rs.state[:, 2].max() >= 2 and rs.state[:, 3].max() >= 3
    env.close()


def _step_against_twins_no_dr(env, seed, acts, prm, name, tol):
    """Re-run the step from the restored state with the schedules off (the table keeps its
    values) against the per-env twins, then turn them on again with their state untouched."""
    view = env.task.get_robot()
    N.check(N.lib().mi_sim_set_phys_dr(view.handle, None), "mi_sim_set_phys_dr")
    try:
        return _step_against_twins(env, seed, acts, prm, name, tol)
    finally:
        env.task._dr_randomizer._register_physics()


@pytest.mark.parametrize("name", ["Cartpole", "Ant", "Humanoid"])
def test_fused_equals_modular_with_physics_dr(gpu, name):
    o = _dr_overrides(VIEWS[name], cartpole=name == "Cartpole")
    ea = make_env(name, num_envs=96, device="cuda:0", seed=13, overrides=o)
    eb = make_env(name, num_envs=96, device="cuda:0", seed=13, overrides=o)
    eb.use_fused(False)
    assert ea.fused and not eb.fused
    for step in range(5):
        acts = rand_actions(96, ea.num_actions, step).to("cuda:0")
        oa, ra, da, _ = ea.step(acts)
        ob, rb, db, _ = eb.step(acts)
        torch.cuda.synchronize()
        np.testing.assert_allclose(oa["obs"].cpu().numpy(), ob["obs"].cpu().numpy(), rtol=1e-5, atol=1e-5,
                                   err_msg=f"{name} step {step}")
        np.testing.assert_allclose(ra.cpu().numpy(), rb.cpu().numpy(), rtol=1e-5, atol=1e-5)
        assert torch.equal(da, db)
        np.testing.assert_array_equal(ea.task.get_robot().phys_dr_state(), eb.task.get_robot().phys_dr_state())
    assert ea.task.get_robot().phys_dr_state()[:, 3].max() >= 2
    if name == "Cartpole":      # the additive schedule left non-zero damping (nominal: zero)
        assert float(_params(ea.task.get_robot())[2].min()) >= 0.002
    ea.close()
    eb.close()


def test_graph_capture_equals_eager(gpu):
    o = _dr_overrides("ant_view")
    ea = make_env("Ant", num_envs=32, device="cuda:0", seed=23, overrides=o)
    eb = make_env("Ant", num_envs=32, device="cuda:0", seed=23, overrides=o)
    acts = [rand_actions(32, ea.num_actions, 90 + k).cuda() for k in range(3)]
    ea.step(acts[0]); eb.step(acts[0])                                   # warm-up outside the capture
    ta, tb = ea.task, eb.task
    outs = [tuple(torch.empty_like(t) for t in (ta.obs_buf, ta.rew_buf, ta.reset_buf)) for _ in range(3)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    state = ea.task.get_robot().phys_dr_state()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for k in range(3):
                ta.fused_step(acts[k], out=outs[k])
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    # the capture ran nothing: replay once, against three eager steps of the twin
    np.testing.assert_array_equal(ea.task.get_robot().phys_dr_state(), state)
    g.replay()
    torch.cuda.synchronize()
    for k in range(3):
        tb.fused_step(acts[k], out=tuple(torch.empty_like(t) for t in outs[k]))
    torch.cuda.synchronize()
    sa, sb = _snap(ea), _snap(eb)
    for k in ("pos", "quat", "vel", "q", "qd", "reset", "prog", "pot"):
        assert torch.equal(sa[k], sb[k]), k
    np.testing.assert_array_equal(ea.task.get_robot().phys_dr_state(), eb.task.get_robot().phys_dr_state())
    pa, pb = _params(ea.task.get_robot()), _params(eb.task.get_robot())
    for a in pa:
        np.testing.assert_array_equal(pa[a], pb[a])
    ea.close()
    eb.close()


@pytest.mark.parametrize("name", ["Cartpole", "Ant", "Humanoid"])
def test_off_means_off(gpu, name):
    """No table, no schedule == a sim that had both and dropped them: bit-identical."""
    ea = make_env(name, num_envs=32, device="cuda:0", seed=29)
    eb = make_env(name, num_envs=32, device="cuda:0", seed=29,
                  overrides=_dr_overrides(VIEWS[name], cartpole=name == "Cartpole"))
    vb = eb.task.get_robot()
    _set_params(vb, _random_params(vb, np.random.default_rng(1)))
    torch.cuda.synchronize()
    N.check(N.lib().mi_sim_set_phys_dr(vb.handle, None), "mi_sim_set_phys_dr")
    vb.clear_env_params()
    for step in range(5):
        acts = rand_actions(32, ea.num_actions, 10 + step).cuda()
        a, b = _step_plain(ea, acts), _step_plain(eb, acts)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name} step {step} {k}")
    ea.close()
    eb.close()


def _step_plain(env, acts):
    t, v = env.task, env.task.get_robot()
    o, r, d, _ = env.step(acts)
    torch.cuda.synchronize()
    return {"obs": o["obs"].cpu().numpy().copy(), "rew": r.cpu().numpy().copy(), "reset": d.cpu().numpy().copy(),
            "q": v.get_joint_positions().cpu().numpy(), "qd": v.get_joint_velocities().cpu().numpy()}


_CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
from omniisaacgymenvs_amd.utils.task_util import make_env
env = make_env("Ant", num_envs=32, device="cuda:0", seed=1)
view = env.task.get_robot()
assert view.sim_kernel_path()[0] == 1
try:
    view.set_env_gravity(torch.zeros((32, 3)))
except RuntimeError as e:
    print("REFUSED", e)
env.close()
"""


def test_refusals(gpu, tmp_path):
    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, MI_WAVE_PAIR="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "REFUSED" in r.stdout and "(-7)" in r.stdout and "wavefront-per-env" in r.stdout, r.stdout
    env = make_env("Cartpole", num_envs=64, device="cuda:0", seed=1)
    view = env.task.get_robot()
    with pytest.raises(RuntimeError, match=r"\(-5\).*armature"):
        view.set_armatures(torch.zeros((64, 2)))
    with pytest.raises(RuntimeError, match=r"\(-5\).*friction"):
        view.set_friction_coefficients(torch.ones((64, 1)))
    env.close()
