"""Force sensors and the lambda publish run in the final substep of a launch only (mi_pair.hpp
pair_artic_substep, mi_wave.hpp wave_artic_substep: P11a and the s_ad lambda stores sit under
store_state), and the paired narrow sweeps keep each lane's own row's lambda inside the sweep.

Small launches of Humanoid and Ant under both solvers, 33 envs (one env per wave) and 34 (the paired
kernel), with controlFrequencyInv 1, 2 and 3: 3 gives two substeps that skip the sensors ahead of
the final one, 1 gives none. Every case starts from a few fused steps of random actions, so that
contacts are active (asserted: some env has nonzero sensor forces; otherwise the case shows
nothing). From that state:
  * one fused env-step stays within the one-step bounds of tests/parity_bounds.py against the
    oracle (state, sensors, obs and reward: the obs groups and the reward);
  * the state and the sensor wrenches after the fused step (one launch of k substeps, sensors in
    the last only) are bit-equal to those of k World.step() calls from the same state with the
    efforts the fused step set (k launches of one substep: each is a final substep, so each
    evaluates the sensors as every substep did before). Envs that the fused step resets are left
    out (the reset is the fused step's own). Measured bit-equal on the commit before this change
    as well;
  * partner independence in the paired kernel (34 envs): two runs from the same state that differ
    in the actions of three envs; outputs, sensors and next state of every other env, the wave
    partners of those three included, are bit-identical in both runs."""
import numpy as np
import pytest
import torch

from omniisaacgymenvs_amd.utils.task_util import make_env
from tests import parity_bounds as PB
from tests.helpers import oracle_sensitivity, oracle_twin, rand_actions, task_buffers
from tests.test_gpu_ltdl_lean import _restore, _snap

pytestmark = pytest.mark.gpu

SEED = 17
WARM = 6            # fused steps of random actions before the checked one


def _make(name, solver, n, cfi):
    env = make_env(name, num_envs=n, device="cuda:0", seed=SEED,
                   overrides=[f"solver_type={solver}", f"task.env.controlFrequencyInv={cfi}"])
    view = env.task.get_robot()
    assert env.task.control_frequency_inv == cfi
    assert view.sim_params.solver_type == solver
    assert view.sim_kernel_path()[0] == (2 if n % 2 == 0 else 1), "34 envs: paired kernel; 33: one env per wave"
    return env


def _warm(env, n):
    env.reset()
    for k in range(WARM):
        env.step(rand_actions(n, env.task.num_actions, 20 + k).to("cuda:0"))
    torch.cuda.synchronize()


def _sensors(view):
    return view._physics_view.get_force_sensor_forces().cpu().numpy().copy()


def _state(view):
    torch.cuda.synchronize()
    p, q = view.get_world_poses()
    return {"pos": p.cpu().numpy(), "quat": q.cpu().numpy(), "vel": view.get_velocities().cpu().numpy(),
            "q": view.get_joint_positions().cpu().numpy(), "qd": view.get_joint_velocities().cpu().numpy(),
            "sens": _sensors(view)}


def _same(x, y):
    x, y = x.reshape(len(x), -1), y.reshape(len(y), -1)
    return np.all((x == y) | (np.isnan(x) & np.isnan(y)), axis=1)


@pytest.mark.parametrize("cfi", [1, 2, 3])
@pytest.mark.parametrize("n", [33, 34])
@pytest.mark.parametrize("solver", [1, 0])
@pytest.mark.parametrize("name", ["Humanoid", "Ant"])
def test_fused_step_matches_oracle_and_world_steps(gpu, name, solver, n, cfi):
    env = _make(name, solver, n, cfi)
    task, view = env.task, env.task.get_robot()
    _warm(env, n)
    snap = _snap(env)
    acts = rand_actions(n, task.num_actions, 7)
    orc = oracle_twin(env, seed=SEED)
    b = task_buffers(env)
    groups = PB.group_slices(task.model.num_dof, task.model.num_sensors)
    sg, sr, _ = oracle_sensitivity(env, SEED, acts.numpy(), cfi, b, groups)
    sens = np.maximum(np.max(np.stack(list(sg.values())), axis=0), sr)
    obs_dict, rew, resets, _ = env.step(acts.to("cuda:0"))
    fused = _state(view)
    print(f"[substep-dead] {name} solver {solver} n {n} cfi {cfi}: envs with sensor force "
          f"{int(np.any(fused['sens'] != 0, axis=(1, 2)).sum())}, max |sensor| {np.abs(fused['sens']).max():.4g}")
    assert np.any(fused["sens"] != 0), "no env has contact forces on a sensor: the case shows nothing"
    orc.env_step(acts.numpy(), cfi, b)
    PB.check(PB.bounds_key(name, solver), groups, obs_dict["obs"].cpu().numpy(), rew.cpu().numpy(),
             b["obs"], b["rew"], orc.decision_margin(), sens=sens,
             pot=np.maximum(np.abs(b["pot"]), np.abs(b["prev"])), quantiles=False)
    assert np.array_equal(resets.cpu().numpy(), b["reset"])
    orc.close()
    # the same k substeps as k World.step() launches, from the same state, with the efforts the
    # fused step left in the state
    keep = snap["reset"].cpu().numpy() == 0
    assert keep.sum() >= n // 2, "most envs must take part in the comparison"
    _restore(env, snap)
    for _ in range(cfi):
        env._world.step()
    world = _state(view)
    diff = {}
    for kk in fused:
        bad = ~_same(fused[kk], world[kk]) & keep
        if bad.any():
            d = np.abs(fused[kk].astype(np.float64) - world[kk]).reshape(n, -1)[bad]
            diff[kk] = (np.nonzero(bad)[0].tolist(), float(np.nanmax(d)))
    print(f"[substep-dead] {name} solver {solver} n {n} cfi {cfi}: fused vs {cfi} x World.step, "
          f"{int(keep.sum())} envs compared, differing {diff}")
    assert not diff, f"fused step and World.step path differ: {diff}"
    env.close()


CHANGED = (0, 5, 17)     # envs whose actions differ between the two runs


@pytest.mark.parametrize("cfi", [2, 3])
@pytest.mark.parametrize("solver", [1, 0])
@pytest.mark.parametrize("name", ["Humanoid", "Ant"])
def test_partner_outputs_do_not_depend_on_an_envs_actions(gpu, name, solver, cfi):
    n = 34
    env = _make(name, solver, n, cfi)
    task, view = env.task, env.task.get_robot()
    _warm(env, n)
    snap = _snap(env)
    acts = rand_actions(n, task.num_actions, 8)
    other = acts.clone()
    for e in CHANGED:
        other[e] = -0.5 * acts[e]
    outs = []
    for a_ in (acts, other):
        _restore(env, snap)
        o, r, d, _ = env.step(a_.to("cuda:0"))
        out = _state(view)
        out.update(obs=o["obs"].cpu().numpy().copy(), rew=r.cpu().numpy().copy(), reset=d.cpu().numpy().copy())
        outs.append(out)
    a, b = outs
    rest = np.ones(n, bool)
    rest[list(CHANGED)] = False
    diff = {kk: np.nonzero(~_same(a[kk], b[kk]) & rest)[0].tolist() for kk in a
            if not (_same(a[kk], b[kk]) | ~rest).all()}
    print(f"[substep-dead] {name} solver {solver} cfi {cfi}: envs with the same actions that differ {diff}")
    assert not diff, f"an env's results depend on another env's actions: {diff}"
    assert np.any(a["sens"][rest] != 0), "no env has contact forces on a sensor: the case shows nothing"
    assert np.isfinite(a["obs"]).all() and np.isfinite(a["q"]).all()
    live = [e for e in CHANGED if int(snap["reset"][e]) == 0]
    assert live and all(not np.array_equal(a["qd"][e], b["qd"][e]) for e in live), \
        "the changed actions must change those envs' own results"
    env.close()
