"""What mi_sim_create decides, pinned: kernel path, compiled topology, LDS bytes per env
(mi_sim_kernel_path) and the W rows kept in LDS (mi_sim_w_rows_lds), per model, env count, path
selection and self-collision setting. The table was recorded on commit 6668936 ("Paired env step:
sensors and lambda publish in the final substep only"), before mi_sim_create was split into
stages; a change of the layout formulas, the eligibility rules or the environment variables read
at create shows up here as a changed row.

34 envs: even, so the compiled topologies take the paired kernels; 33: odd, one env per wave.
The environment variables are read at create, so setting them before make_env works in-process."""
import ctypes as C

import pytest

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.utils.task_util import make_env

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "pair0": {"MI_WAVE_PAIR": "0"}, "runtime": {"MI_SIM_TOPO": "runtime"}}

# (task, envs, mode, self-collision) -> (path, topology, LDS bytes per env, W rows in LDS)
PINNED = {
    ("Humanoid", 34, "default", True): (2, 1, 10133, 32),
    ("Humanoid", 34, "default", False): (2, 1, 9871, 32),
    ("Humanoid", 34, "pair0", True): (1, 1, 20368, 33),
    ("Humanoid", 34, "pair0", False): (1, 1, 18352, 22),
    ("Humanoid", 34, "runtime", True): (1, 0, 24512, 0),
    ("Humanoid", 34, "runtime", False): (1, 0, 23680, 0),
    ("Humanoid", 33, "default", True): (1, 1, 20368, 33),
    ("Humanoid", 33, "default", False): (1, 1, 18352, 22),
    ("Humanoid", 33, "pair0", True): (1, 1, 20368, 33),
    ("Humanoid", 33, "pair0", False): (1, 1, 18352, 22),
    ("Humanoid", 33, "runtime", True): (1, 0, 24512, 0),
    ("Humanoid", 33, "runtime", False): (1, 0, 23680, 0),
    ("Ant", 34, "default", False): (2, 2, 7341, 64),
    ("Ant", 34, "pair0", False): (1, 2, 10228, 45),
    ("Ant", 34, "runtime", False): (1, 0, 15568, 0),
    ("Ant", 33, "default", False): (1, 2, 10228, 45),
    ("Ant", 33, "pair0", False): (1, 2, 10228, 45),
    ("Ant", 33, "runtime", False): (1, 0, 15568, 0),
}


def layout(monkeypatch, name, n, mode, self_on):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    ov = [] if name == "Cartpole" else [f"task.sim.{name}.enable_self_collisions={bool(self_on)}"]
    env = make_env(name, num_envs=n, device="cuda:0", seed=1, overrides=ov)
    for k in MODES[mode]:
        monkeypatch.delenv(k)
    view = env.task.get_robot()
    rows = C.c_int32(-1)
    N.check(N.lib().mi_sim_w_rows_lds(view.handle, C.byref(rows)), "mi_sim_w_rows_lds")
    got = (*view.sim_kernel_path(), int(rows.value))
    pairs = 0 if name == "Cartpole" else int(view.model.pairs.shape[0])
    env.close()
    return got, pairs


# self-collision on where the model has pairs (Humanoid; the shipped Ant has none), and off
CASES = [(name, n, mode, self_on) for name, selfs in (("Humanoid", (True, False)), ("Ant", (False,)))
         for n in (34, 33) for mode in MODES for self_on in selfs]


@pytest.mark.parametrize("name,n,mode,self_on", CASES)
def test_create_layout_is_pinned(gpu, monkeypatch, name, n, mode, self_on):
    got, pairs = layout(monkeypatch, name, n, mode, self_on)
    assert (pairs > 0) == (name == "Humanoid")
    assert got == PINNED[(name, n, mode, self_on)]
    # the table's own sanity: paired only for an even env count on a compiled topology
    assert got[0] == (2 if (n % 2 == 0 and mode == "default") else 1)
    assert (got[1] != 0) == (mode != "runtime")


def test_cartpole_is_one_lane_per_env(gpu, monkeypatch):
    got, _ = layout(monkeypatch, "Cartpole", 34, "default", False)
    assert got == (0, 0, 0, 0)
