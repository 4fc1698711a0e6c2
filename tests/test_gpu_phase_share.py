"""The substep phases and the task layer that the one-env-per-wave and the two-envs-per-wave
kernels share (csrc/mi_phase.hpp) compute what the two separate copies computed: the fused env
step of Humanoid (self-collision on, as its yaml has it) and Ant, bit for bit against arrays
recorded before the phases were merged, on every kernel the phases are instantiated in:

    pair     8 envs, default            path 2, two envs per wave (Grp32)
    pair0    8 envs, MI_WAVE_PAIR=0     path 1, one env per wave (Grp64), compiled topology
    odd      7 envs                     path 1 by the odd env count
    runtime  8 envs, MI_SIM_TOPO=runtime   path 1, runtime tables

each with the TGS and the PGS solver.

Fixtures: tests/golden/phase_share/<task>_<variant>_<solver>.npz, recorded on commit 29285bf
("Sim host side: one kernel selection, one launch path, staged create", the parent of the commit
that added mi_phase.hpp) on one MI355X with

    python tools/make_golden_phase_share.py

Each holds the last step's obs / reward / reset arrays and every step's reward and reset rows.
Actions are U(-1, 1) from numpy's PCG64(SEED). Eight Humanoids under such actions need about 25
steps before the first one falls and Ants do not terminate at all in a short run (tests/golden/
ant_steps.npz: no reset in 24 steps of 256 envs), so the episode length is cut to EPISODE steps:
every env runs into the time-out reset, is re-initialised by the next step's pre-physics reset and
lands again. The recorder then takes the smallest step count at which, for every fixture of the
task, a reset lies at least two steps back and the last step's force-sensor observations are not
all zero (the contact filing and the sensor loop have run with contacts). Both conditions are
asserted on the fixture itself before anything is compared."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phase_share")
TASKS = ("Humanoid", "Ant")
# variant -> (envs, environment read at create, expected (path, compiled topology?))
VARIANTS = {
    "pair": (8, {}, (2, True)),
    "pair0": (8, {"MI_WAVE_PAIR": "0"}, (1, True)),
    "odd": (7, {}, (1, True)),
    "runtime": (8, {"MI_SIM_TOPO": "runtime"}, (1, False)),
}
SOLVERS = {"tgs": 1, "pgs": 0}
SEED = 11
EPISODE = 6        # task.env.episodeLength of the runs
CASES = [(t, v, s) for t in TASKS for v in VARIANTS for s in SOLVERS]


def fixture_path(task, variant, solver):
    return os.path.join(GOLDEN, f"{task.lower()}_{variant}_{solver}.npz")


def sensor_block(obs, num_actions):
    """The force-sensor columns of an obs array [..., O]: O = 12 + 3 D + 6 S, sensors after the
    root block, DOF positions and DOF velocities (locomotion.py get_observations)."""
    return obs[..., 12 + 2 * num_actions: obs.shape[-1] - num_actions]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rollout(task, variant, solver, steps):
    """`steps` fused env steps after reset(); per step the obs, reward and reset arrays."""
    import torch

    from omniisaacgymenvs_amd.utils.task_util import make_env

    n, environ, (path, compiled) = VARIANTS[variant]
    saved = {k: os.environ.get(k) for k in environ}
    os.environ.update(environ)
    try:   # the variables are read at create
        env = make_env(task, num_envs=n, device="cuda:0", seed=SEED,
                       overrides=[f"solver_type={SOLVERS[solver]}", f"task.env.episodeLength={EPISODE}"])
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    got = env.task.get_robot().sim_kernel_path()
    assert got[0] == path and (got[1] != 0) == compiled, (task, variant, got)
    env.reset()
    rng = np.random.Generator(np.random.PCG64(SEED))
    out = {"obs": [], "rew": [], "reset": []}
    for _ in range(steps):
        a = rng.uniform(-1.0, 1.0, (n, env.num_actions)).astype(np.float32)
        o, r, d, _ = env.step(torch.from_numpy(a).to("cuda:0"))
        out["obs"].append(o["obs"].cpu().numpy().copy())
        out["rew"].append(r.cpu().numpy().copy())
        out["reset"].append(d.cpu().numpy().copy())
    na = env.num_actions
    env.close()
    return {k: np.stack(v) for k, v in out.items()}, na


@pytest.mark.parametrize("task,variant,solver", CASES)
def test_fused_step_equals_recording(gpu, task, variant, solver):
    fx = np.load(fixture_path(task, variant, solver))
    steps = int(fx["steps"])
    n = VARIANTS[variant][0]
    assert fx["rew_steps"].shape == (steps, n) and fx["reset_steps"].shape == (steps, n)
    # the recording exercises what moved: a reset at least two steps back (decided, then carried
    # out by the next pre-physics step), and contacts under a sensor in the last step
    assert fx["reset_steps"][:steps - 2].any(), "fixture without a reset"
    assert np.any(sensor_block(fx["obs"], int(fx["num_actions"])) != 0.0), "fixture without a sensor force"
    got, na = rollout(task, variant, solver, steps)
    assert na == int(fx["num_actions"])
    for k in ("rew", "reset"):
        for s in range(steps):
            assert same_bits(got[k][s], fx[k + "_steps"][s]), (k, "step", s)
    for k in ("obs", "rew", "reset"):
        assert same_bits(got[k][-1], fx[k]), k
