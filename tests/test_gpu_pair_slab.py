"""The paired kernel's W rows beyond LDS (mi_pair.hpp: the env's global slab), reached on purpose.

An env's W rows [0, w_rows_lds) sit in LDS, the rest of a row-heavy substep in its global slab.
The parity tests reach the slab only where their states happen to be heavy enough, so this file
crafts one workgroup (16 envs, the smallest launch with a full workgroup) per task and solver:
  * three copies of a robot lying on the ground in non-adjacent slots: more constraint rows than
    the narrow path takes (kLamRows) and at most 64, so their waves take the wide Delassus path;
    the Humanoid layout keeps 32 W rows in LDS, so these envs' rows 32.. are slab rows (set-up
    loads, u update, P9's slab stores);
  * one env pressed into the ground: more than 64 rows, the u-space fallback sweeps, whose rows
    64.. are slab rows in every layout (at most 64 rows fit LDS);
  * the rest as the reset left them (few rows: the narrow path).
The Ant layout keeps all 64 rows of the wide path in LDS (mi_sim_w_rows_lds reports 64), so no
pose can put a wide-path Ant env beyond its LDS rows: there the copies cover the wide path with
LDS rows only (Ant's kLamRows of 24 is below the register rows of the wide set-up, the other
compile-time choice of its groups), and the deep env is the one that leaves LDS.
It proves it got there: the oracle's contact count of the posed state (3 rows per contact) and
the device's own row count of the step (mi_sim_pair_load) must both put every copy on the wide
path, the deep env past 64 rows, and at least the deep env — with fewer than 64 LDS rows every
copy too — beyond the layout's LDS rows (mi_sim_w_rows_lds). Then, over a few fused steps (reset
flags cleared in between, so the robots stay down and pick up velocities): every env within the
one-step bounds of tests/parity_bounds.py against the oracle from the identical state, and the
copies bit-identical to each other.

The launches pair the envs by index (envs 2w and 2w + 1 in wave w), not by load: which path a wave
takes is decided by its heavier half, and the u-space fallback sweeps are another algorithm than
the Delassus-space ones (the same solution up to rounding), so a copy that the load ranking puts
into the deep env's wave runs the fallback and differs from the other copies in the last bits
(Ant, measured: the copy in slot 0 was ranked next to the deep env in slot 6 and differed from
the copies in slots 3 and 9 by up to 7.5e-6 in obs; with the deep env in slot 7, or pairing by
index, all copies agree). With index pairing every copy's partner is a light env and the deep
env's partner is slot 7, as laid out above."""
import numpy as np
import pytest
import torch

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.utils.task_util import make_env
from tests import parity_bounds as PB
from tests.helpers import oracle_sensitivity, oracle_twin, task_buffers

pytestmark = pytest.mark.gpu

N_ENVS = 16                 # one workgroup of the paired kernel
COPIES = (0, 3, 9)          # the wide-path copies: no two adjacent, partners on the narrow path
DEEP = 6                    # the env past 64 rows
STEPS = 3
LAM_ROWS = {"Humanoid": 32, "Ant": 24}     # mi_topo.hpp kLamRows: more rows leave the narrow path
# root height of the lying copies (rotated 90 deg about y); root height of the deep env and
# whether it lies as well (the Ant has most contacts upright, legs and torso on the ground)
POSE_Z = {"Humanoid": (0.08, 0.03, True), "Ant": (0.2, 0.05, False)}


def _w_rows_lds(view):
    import ctypes as C

    r = C.c_int32(-1)
    N.check(N.lib().mi_sim_w_rows_lds(view.handle, C.byref(r)), "mi_sim_w_rows_lds")
    return int(r.value)


def _loads(view, pairing=-1):
    out = np.zeros(view.count, np.int32)
    N.check(N.lib().mi_sim_pair_load(view.handle, out.ctypes.data, None, int(pairing)), "mi_sim_pair_load")
    return out


@pytest.mark.parametrize("solver", [1, 0])
@pytest.mark.parametrize("name", ["Humanoid", "Ant"])
def test_slab_rows_match_oracle_and_copies_agree(gpu, name, solver):
    env = make_env(name, num_envs=N_ENVS, device="cuda:0", seed=9, overrides=[f"solver_type={solver}"])
    task, view = env.task, env.task.get_robot()
    assert view.sim_kernel_path()[0] == 2, "the paired kernel is the default"
    assert view.sim_params.solver_type == solver
    w_lds = _w_rows_lds(view)
    assert w_lds >= LAM_ROWS[name] and w_lds % 4 == 0, w_lds
    A = task.num_actions
    _loads(view, pairing=0)     # index pairing: no copy shares a wave with the deep env (see above)
    assert all((sl ^ 1) not in COPIES + (DEEP,) for sl in COPIES) and (DEEP ^ 1) not in COPIES
    env.reset()
    torch.cuda.synchronize()
    pos, _ = view.get_world_poses()
    pos = pos.clone()
    s = float(np.sqrt(0.5))
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * N_ENVS, device="cuda:0")
    z_wide, z_deep, deep_lies = POSE_Z[name]
    for sl in COPIES:
        pos[sl] = pos[COPIES[0]]
        pos[sl, 2] = z_wide
    pos[DEEP, 2] = z_deep
    rot[list(COPIES) + ([DEEP] if deep_lies else [])] = torch.tensor([s, 0.0, s, 0.0], device="cuda:0")   # lying
    q = view.get_joint_positions().clone()
    qd = view.get_joint_velocities().clone()
    q[list(COPIES) + [DEEP]] = 0.0
    qd[list(COPIES) + [DEEP]] = 0.0
    vel = view.get_velocities().clone()
    vel[list(COPIES) + [DEEP]] = 0.0
    view.set_world_poses(pos, rot)
    view.set_velocities(vel)
    view.set_joint_positions(q)
    view.set_joint_velocities(qd)
    # the copies share every per-env input of the step (their env origins differ: the task's
    # observations use positions relative to the walk target, so the copies sit at one world
    # position instead, which the ground plane does not mind)
    task.reset_buf.zero_()
    for buf in (task.potentials, task.prev_potentials):
        buf[list(COPIES)] = buf[COPIES[0]].clone()
    torch.cuda.synchronize()
    groups = PB.group_slices(task.model.num_dof, task.model.num_sensors)
    key = PB.bounds_key(name, solver)
    g = torch.Generator().manual_seed(77)
    reached_slab, reached_fallback = False, False
    copies_differ = {}
    for k in range(STEPS):
        acts = torch.rand((N_ENVS, A), generator=g) * 0.6 - 0.3
        acts[list(COPIES)] = acts[COPIES[0]].clone()
        orc = oracle_twin(env, seed=9)
        b = task_buffers(env)
        rows_orc = np.array([3 * orc.contact_count(e) for e in range(N_ENVS)])   # limit rows come on top
        sg, sr, _ = oracle_sensitivity(env, 9, acts.numpy(), task.control_frequency_inv, b, groups)
        sens = np.maximum(np.max(np.stack(list(sg.values())), axis=0), sr)
        obs_dict, rew, resets, _ = env.step(acts.to("cuda:0"))
        torch.cuda.synchronize()
        orc.env_step(acts.numpy(), task.control_frequency_inv, b)
        rows_dev = _loads(view)     # most rows of any substep of this step, per env
        print(f"[slab] {name} solver {solver} step {k}: LDS rows {w_lds}, oracle rows at the start "
              f"{rows_orc.tolist()}, device rows {rows_dev.tolist()}")
        wide = [sl for sl in COPIES if LAM_ROWS[name] < rows_orc[sl] and LAM_ROWS[name] < rows_dev[sl] <= 64]
        beyond = [e for e in list(COPIES) + [DEEP] if w_lds < rows_orc[e] and w_lds < rows_dev[e]]
        reached_slab |= DEEP in beyond and (w_lds >= 64 or all(sl in beyond for sl in wide))
        reached_fallback |= rows_orc[DEEP] > 64 and rows_dev[DEEP] > 64
        obs, rw = obs_dict["obs"].cpu().numpy(), rew.cpu().numpy()
        PB.check(key, groups, obs, rw, b["obs"], b["rew"], orc.decision_margin(), sens=sens,
                 pot=np.maximum(np.abs(b["pot"]), np.abs(b["prev"])), quantiles=False)
        assert np.array_equal(resets.cpu().numpy(), b["reset"])
        orc.close()
        p_, q_ = view.get_world_poses()
        state = {"obs": obs, "rew": rw, "pos": p_.cpu().numpy(), "quat": q_.cpu().numpy(),
                 "vel": view.get_velocities().cpu().numpy(), "q": view.get_joint_positions().cpu().numpy(),
                 "qd": view.get_joint_velocities().cpu().numpy()}
        differ = {(kk, sl): float(np.abs(a[sl].astype(np.float64) - a[COPIES[0]]).max())
                  for kk, a in state.items() for sl in COPIES[1:] if not np.array_equal(a[sl], a[COPIES[0]])}
        print(f"[slab] {name} solver {solver} step {k}: copies differing from slot {COPIES[0]} "
              f"(field, slot): max |difference| {differ}")
        copies_differ[k] = differ       # asserted after the last step: the other checks of every step still run
        assert all(rows_dev[sl] == rows_dev[COPIES[0]] for sl in COPIES)
        if k == 0:
            # the crafted layout, before the robots move: the copies on the wide path next to
            # narrow-path envs, and beyond LDS wherever the wide path can be (fewer than 64 LDS
            # rows); the deep env beyond the wide path and beyond LDS
            assert len(wide) == len(COPIES), (w_lds, rows_orc[list(COPIES)], rows_dev[list(COPIES)])
            assert DEEP in beyond and rows_orc[DEEP] > 64 and rows_dev[DEEP] > 64, (w_lds, rows_orc[DEEP], rows_dev[DEEP])
            assert w_lds >= 64 or all(sl in beyond for sl in COPIES), (w_lds, beyond)
            light = [e for e in range(N_ENVS) if e not in COPIES and e != DEEP]
            assert rows_dev[light].max() <= LAM_ROWS[name], rows_dev[light]
        task.reset_buf.zero_()      # the robots stay down (below the termination height)
        torch.cuda.synchronize()
    assert not any(copies_differ.values()), f"the copies are not bit-identical: {copies_differ}"
    assert reached_slab, "no step with rows beyond the LDS rows"
    assert reached_fallback, "the deep env never had more than 64 rows: the fallback sweeps did not run"
    env.close()
