"""P2 (composite inertia / force sums) of the paired kernel on lane = (link, slot) items
(mi_pair.hpp pair_p2_composites, tests/test_p2_item_table.py for the table itself): the fold's
additions and their order are unchanged, so every output keeps its bits.

What this file can and cannot show: the fused step and World.step run the same P2, so a fold that
were wrong in the same way everywhere would pass here. The guard of the bits themselves is
tests/test_gpu_phase_share.py (arrays recorded before the item mapping) and tools/hash_run.py
against the previous build. This file covers what those do not: the smallest launch, ragged
launches, and that both halves of a wave and every wave of a ragged workgroup run the mapping
alike (a half that read the other half's items, or a lane past the last item that wrote, would
break the World.step equality or the oracle-free finiteness check).

Humanoid and Ant under TGS and PGS, 3 fused env steps of random actions from the seeded reset, at
  *  2 envs: one wave of the paired kernel, both halves;
  * 34 envs: the paired kernel with a ragged last workgroup (17 waves, 8 per workgroup);
  * 33 envs: odd, so mi_sim_create takes the one-env-per-wave kernel, which keeps lane = link:
    the case the issue names, here a check that the unchanged kernel stayed so.
Checked per case:
  * obs, reward, resets and the state after every step are bit-equal between the default kernel
    selection and MI_WAVE_PAIR=0 (one env per wave) wherever the commit before this change is
    bit-equal there too: PARENT_EQUAL below, recorded by running this file's `compare` against
    that commit's library;
  * the third fused step (one launch of k substeps) leaves the state and the sensor wrenches that
    k World.step() launches from the same state leave (as tests/test_gpu_substep_dead.py: envs the
    fused step resets are left out). This holds on the commit before this change as well, and is
    the check for the cases where the two kernels differ in some bits there."""
import numpy as np
import pytest
import torch

from omniisaacgymenvs_amd.utils.task_util import make_env
from tests.helpers import rand_actions
from tests.test_gpu_ltdl_lean import _restore, _snap, _step
from tests.test_gpu_substep_dead import _same, _state

pytestmark = pytest.mark.gpu

SEED = 23
STEPS = 3
NS = (2, 33, 34)
CASES = [(name, solver, n) for name in ("Humanoid", "Ant") for solver in (1, 0) for n in NS]

# (task, solver, envs) -> default selection and MI_WAVE_PAIR=0 bit-equal on the commit before
# this change. Recorded there: the paired and the one-env-per-wave kernels differ in some bits of
# obs, reward and state in every case with an even env count (both tasks, both solvers, 2 and 34
# envs), and are equal at 33 envs only, where both selections are the one-env-per-wave kernel. The
# World.step comparison held in all twelve cases there. So it is the check of the paired kernel.
PARENT_EQUAL = {c: c[2] % 2 == 1 for c in CASES}


def run(monkeypatch, name, solver, n, pair, world_check=False):
    """STEPS fused steps from the seeded reset; the per-step outputs, and with world_check what the
    last fused step and k World.step() launches from the same state leave."""
    if not pair:
        monkeypatch.setenv("MI_WAVE_PAIR", "0")
    env = make_env(name, num_envs=n, device="cuda:0", seed=SEED, overrides=[f"solver_type={solver}"])
    if not pair:
        monkeypatch.delenv("MI_WAVE_PAIR")
    view = env.task.get_robot()
    assert view.sim_kernel_path()[0] == (2 if pair and n % 2 == 0 else 1)
    env.reset()
    outs, world = [], None
    for k in range(STEPS):
        acts = rand_actions(n, env.task.num_actions, 40 + k).to("cuda:0")
        if world_check and k == STEPS - 1:
            snap = _snap(env)
            outs.append(_step(env, acts))
            fused = _state(view)
            keep = snap["reset"].cpu().numpy() == 0
            _restore(env, snap)
            for _ in range(env.task.control_frequency_inv):
                env._world.step()
            world = (fused, _state(view), keep)
        else:
            outs.append(_step(env, acts))
    env.close()
    return outs, world


def compare(monkeypatch, name, solver, n):
    """(keys that differ between the two selections, keys that differ fused vs World.step)"""
    a, world = run(monkeypatch, name, solver, n, True, world_check=True)
    b, _ = run(monkeypatch, name, solver, n, False)
    sel = sorted({f"{kk}@{s}" for s in range(STEPS) for kk in a[s] if not _same(a[s][kk], b[s][kk]).all()})
    fused, stepped, keep = world
    assert keep.sum() >= (n + 1) // 2, "most envs must take part in the comparison"
    wd = sorted(kk for kk in fused if (~_same(fused[kk], stepped[kk]) & keep).any())
    assert all(np.isfinite(a[s]["obs"]).all() for s in range(STEPS))
    return sel, wd


@pytest.mark.parametrize("name,solver,n", CASES)
def test_outputs_keep_their_bits(gpu, monkeypatch, name, solver, n):
    sel, wd = compare(monkeypatch, name, solver, n)
    print(f"[p2-lanes] {name} solver {solver} n {n}: default vs MI_WAVE_PAIR=0 differ in {sel}; "
          f"fused vs World.step differ in {wd}")
    assert not wd, f"fused step and World.step path differ: {wd}"
    if PARENT_EQUAL[(name, solver, n)]:
        assert not sel, f"paired and one-env-per-wave kernels differ: {sel}"
