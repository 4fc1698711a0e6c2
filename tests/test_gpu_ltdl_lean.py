"""The lean in-register LTDL (mi_wave.hpp ct_ltdl, mi_pair.hpp ct_ltdl_pair: one scale per pivot,
ancestor updates in every lane) on small launches, Humanoid and Ant under both solvers.

The factorisation leaves junk above the diagonal of each lane's column registers: values that
differ per column and per env and that nothing may read. Two checks, from the seeded reset:
  * one fused env-step within the one-step bounds of tests/parity_bounds.py against the oracle,
    at 33 envs (an odd count runs the one-env-per-wave kernel, ct_ltdl) and at 34 (the paired
    kernel needs an even count: two full workgroups plus a workgroup holding a single wave);
  * partner independence in the paired kernel (34 envs): slot 5 of the first workgroup holds a
    copy of env 0, and the load keys of mi_sim_pair_load (as in tests/test_gpu_pairing.py) pair
    env 0 with that copy in one run and with another env in the other, which gives every env of
    the workgroup another partner too. Outputs and next state of every env must be bit-identical
    in both runs, and the copy's equal to env 0's: the path by which one half's junk could leak
    into the other half, or into anything that is read."""
import numpy as np
import pytest
import torch

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.utils.task_util import make_env
from tests import parity_bounds as PB
from tests.helpers import oracle_sensitivity, oracle_twin, rand_actions, reset_counts, task_buffers

pytestmark = pytest.mark.gpu

SEED = 13
COPY = 5            # slot of the first workgroup that holds the copy of env 0
OTHER = 9           # env 0's partner in the second run


def _make(name, solver, n):
    env = make_env(name, num_envs=n, device="cuda:0", seed=SEED, overrides=[f"solver_type={solver}"])
    view = env.task.get_robot()
    assert view.sim_params.solver_type == solver
    assert view.sim_kernel_path()[0] == (2 if n % 2 == 0 else 1), "34 envs: paired kernel; 33: one env per wave"
    return env


@pytest.mark.parametrize("n", [33, 34])
@pytest.mark.parametrize("solver", [1, 0])
@pytest.mark.parametrize("name", ["Humanoid", "Ant"])
def test_one_step_from_reset_matches_oracle(gpu, name, solver, n):
    env = _make(name, solver, n)
    task = env.task
    env.reset()
    torch.cuda.synchronize()
    acts = rand_actions(n, task.num_actions, 7)
    orc = oracle_twin(env, seed=SEED)
    b = task_buffers(env)
    groups = PB.group_slices(task.model.num_dof, task.model.num_sensors)
    sg, sr, _ = oracle_sensitivity(env, SEED, acts.numpy(), task.control_frequency_inv, b, groups)
    sens = np.maximum(np.max(np.stack(list(sg.values())), axis=0), sr)
    obs_dict, rew, resets, _ = env.step(acts.to("cuda:0"))
    torch.cuda.synchronize()
    orc.env_step(acts.numpy(), task.control_frequency_inv, b)
    PB.check(PB.bounds_key(name, solver), groups, obs_dict["obs"].cpu().numpy(), rew.cpu().numpy(),
             b["obs"], b["rew"], orc.decision_margin(), sens=sens,
             pot=np.maximum(np.abs(b["pot"]), np.abs(b["prev"])), quantiles=False)
    assert np.array_equal(resets.cpu().numpy(), b["reset"])
    assert np.array_equal(task.progress_buf.cpu().numpy(), b["progress"])
    orc.close()
    env.close()


def _loads(view, keys=None, pairing=-1):
    out = np.zeros(view.count, np.int32)
    kin = None if keys is None else np.ascontiguousarray(keys, np.int32)
    N.check(N.lib().mi_sim_pair_load(view.handle, out.ctypes.data,
                                     None if kin is None else kin.ctypes.data, int(pairing)),
            "mi_sim_pair_load")
    return out


def _snap(env):
    t, v = env.task, env.task.get_robot()
    torch.cuda.synchronize()
    p, q = v.get_world_poses()
    return {"pos": p.clone(), "quat": q.clone(), "vel": v.get_velocities().clone(),
            "q": v.get_joint_positions().clone(), "qd": v.get_joint_velocities().clone(),
            "reset": t.reset_buf.clone(), "prog": t.progress_buf.clone(),
            "pot": t.potentials.clone(), "prev": t.prev_potentials.clone(), "rc": reset_counts(v)}


def _restore(env, s):
    t, v = env.task, env.task.get_robot()
    v.set_world_poses(s["pos"], s["quat"])
    v.set_velocities(s["vel"])
    v.set_joint_positions(s["q"])
    v.set_joint_velocities(s["qd"])
    t.reset_buf.copy_(s["reset"])
    t.progress_buf.copy_(s["prog"])
    t.potentials.copy_(s["pot"])
    t.prev_potentials.copy_(s["prev"])
    N.check(N.lib().mi_set_reset_count(v.handle, np.ascontiguousarray(s["rc"]).ctypes.data),
            "mi_set_reset_count")
    torch.cuda.synchronize()


def _step(env, acts):
    t, v = env.task, env.task.get_robot()
    o, r, d, _ = env.step(acts)
    torch.cuda.synchronize()
    p, q = v.get_world_poses()
    return {"obs": o["obs"].cpu().numpy().copy(), "rew": r.cpu().numpy().copy(),
            "reset": d.cpu().numpy().copy(), "prog": t.progress_buf.cpu().numpy().copy(),
            "pot": t.potentials.cpu().numpy().copy(), "pos": p.cpu().numpy(), "quat": q.cpu().numpy(),
            "vel": v.get_velocities().cpu().numpy(), "q": v.get_joint_positions().cpu().numpy(),
            "qd": v.get_joint_velocities().cpu().numpy()}


def _keys(n, partner):
    """Load keys that pair env 0 (heaviest: rank 0) with `partner` (lightest: rank 15) in the
    first workgroup; the other slots get distinct keys in between, the second run's shifted by
    one place so that their partners change as well."""
    keys = np.zeros(n, np.int32)
    rest = [j for j in range(1, 16) if j != partner]
    if partner == OTHER:
        rest = rest[1:] + rest[:1]
    for r_, j in enumerate(rest):
        keys[j] = 50 + r_
    keys[0], keys[partner] = 100, 1
    keys[16:] = 1
    return keys


@pytest.mark.parametrize("solver", [1, 0])
@pytest.mark.parametrize("name", ["Humanoid", "Ant"])
def test_result_does_not_depend_on_the_wave_partner(gpu, name, solver):
    n = 34
    env = _make(name, solver, n)
    task, view = env.task, env.task.get_robot()
    env.reset()
    torch.cuda.synchronize()
    snap = _snap(env)
    # the copy takes env 0's whole state, its reset count (the seed of its reset noise) included;
    # the task's observations are relative to the walk target, so the copy sits at env 0's world
    # position (as the copies of tests/test_gpu_pair_slab.py do)
    for kk in ("pos", "quat", "vel", "q", "qd", "reset", "prog", "pot", "prev", "rc"):
        snap[kk][COPY] = snap[kk][0]
    acts = rand_actions(n, task.num_actions, 8)
    acts[COPY] = acts[0].clone()
    outs = []
    for partner in (COPY, OTHER):
        _restore(env, snap)
        _loads(view, keys=_keys(n, partner), pairing=1)
        outs.append(_step(env, acts.to("cuda:0")))
    _loads(view, pairing=0)
    a, b = outs
    diff = {}
    for kk in a:
        x, y = a[kk].reshape(n, -1), b[kk].reshape(n, -1)
        bad = ~np.all((x == y) | (np.isnan(x) & np.isnan(y)), axis=1)
        if bad.any():
            diff[kk] = (np.nonzero(bad)[0].tolist(), float(np.nanmax(np.abs(x[bad].astype(np.float64) - y[bad]))))
    print(f"[ltdl-lean] {name} solver {solver}: envs differing between the two pairings {diff}")
    assert not diff, f"per-env results depend on the wave partner: {diff}"
    assert np.isfinite(a["obs"]).all() and np.isfinite(a["q"]).all()
    if int(snap["reset"][0]) == 0:
        # (a reset in this step draws noise by env id: the copy then starts from another state)
        for out in outs:
            for kk in ("obs", "rew", "q", "qd", "quat", "vel"):
                assert np.array_equal(out[kk][COPY], out[kk][0]), kk
    env.close()
