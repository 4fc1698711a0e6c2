"""Launch timing through the C ABI (mi_sim_time_launches / mi_sim_launch_times, include/mi_sim.h):
the measurement bench.py's roofline and tools/fuse_roofline.py use. A timed launch is the same
kernel with a HIP event pair on its own dispatch, so its outputs must be bit-identical to an
untimed launch; launches into a capturing stream are not timed."""
import ctypes as C

import pytest
import torch

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.utils.task_util import make_env

pytestmark = pytest.mark.gpu


def _times(view, cap):
    buf = (C.c_float * cap)()
    n = C.c_int32(0)
    N.check(N.lib().mi_sim_launch_times(view.handle, buf, cap, C.byref(n)), "mi_sim_launch_times")
    return n.value, list(buf[:min(n.value, cap)])


@pytest.mark.parametrize("name", ["Humanoid", "Cartpole"])
def test_timed_launches_match_untimed(gpu, name):
    envs = [make_env(name, num_envs=512, device="cuda:0", seed=21) for _ in range(2)]
    acts = torch.rand((6, 512, envs[0].task.num_actions), device="cuda:0") * 2 - 1
    for e in envs:
        e.reset()
    view = envs[1].task.get_robot()
    N.check(N.lib().mi_sim_time_launches(view.handle, 2, 8), "mi_sim_time_launches")
    for k in range(6):
        o0 = envs[0].step(acts[k])
        o1 = envs[1].step(acts[k])
        for a, b in zip((o0[0]["obs"], o0[1], o0[2]), (o1[0]["obs"], o1[1], o1[2])):
            assert torch.equal(a, b)
    n, ms = _times(view, 8)
    assert n == 3                                   # launches 0, 2, 4 of six, every = 2
    assert all(0.0 < x < 50.0 for x in ms), ms
    N.check(N.lib().mi_sim_time_launches(view.handle, 0, 0), "mi_sim_time_launches")
    envs[1].step(acts[0])
    assert _times(view, 8)[0] == 0                  # timing off: nothing recorded
    for e in envs:
        e.close()


def test_post_step_timed_and_capture_untimed(gpu):
    env = make_env("Humanoid", num_envs=4096, device="cuda:0", seed=4)
    t = env.task
    env.reset()
    view = t.get_robot()
    h, s = view.handle, view.stream()
    args = (h, t.actions.data_ptr(), t.obs_buf.data_ptr(), t.rew_buf.data_ptr(), t.reset_buf.data_ptr(),
            t.progress_buf.data_ptr(), t.potentials.data_ptr(), t.prev_potentials.data_ptr(), s)
    N.check(N.lib().mi_sim_time_launches(h, 1, 4), "mi_sim_time_launches")
    N.check(N.lib().mi_task_post_step(*args), "mi_task_post_step")
    n, ms = _times(view, 4)
    assert n == 1 and 0.0 < ms[0] < 50.0
    # a step captured into a HIP graph is not timed (its dispatch cannot carry the events)
    N.check(N.lib().mi_sim_time_launches(h, 0, 0), "mi_sim_time_launches")
    a = torch.zeros((4096, t.num_actions), device="cuda:0")
    env.step(a)
    torch.cuda.synchronize()
    N.check(N.lib().mi_sim_time_launches(h, 1, 4), "mi_sim_time_launches")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.step(a)
    assert _times(view, 4)[0] == 0
    g.replay()
    torch.cuda.synchronize()
    N.check(N.lib().mi_sim_time_launches(h, 0, 0), "mi_sim_time_launches")
    env.close()


def _table(view, n):
    """A per-env parameter table (one attribute set): the EnvP kernel variants run from here on."""
    view.set_friction_coefficients(torch.linspace(0.6, 1.2, n, device="cuda:0").reshape(n, 1))


# every step-kernel family behind the one launch path: (task, envs, environment, table, kernel path)
STEP_FAMILIES = {
    "paired": ("Humanoid", 34, {}, False, 2),
    "paired_envp": ("Humanoid", 34, {}, True, 2),
    "wave": ("Humanoid", 33, {}, False, 1),
    "lane": ("Cartpole", 34, {}, False, 0),
    "lane_envp": ("Cartpole", 34, {}, True, 0),
}


@pytest.mark.parametrize("family", list(STEP_FAMILIES))
def test_each_step_family_timed_equals_untimed(gpu, family):
    """A timed fused env step (event pair on the dispatch) of each kernel family is bit-equal to
    the untimed one from the same state, and every timed launch yields one positive duration."""
    name, n, _, table, path = STEP_FAMILIES[family]
    envs = [make_env(name, num_envs=n, device="cuda:0", seed=21) for _ in range(2)]   # twins: one state
    acts = torch.rand((3, n, envs[0].task.num_actions), device="cuda:0") * 2 - 1
    for e in envs:
        e.reset()
        view = e.task.get_robot()
        assert view.sim_kernel_path()[0] == path
        if table and name == "Cartpole":
            view.set_env_gravity(torch.tensor([[0.0, 0.0, -9.0]], device="cuda:0").repeat(n, 1))
        elif table:
            _table(view, n)
    view = envs[1].task.get_robot()
    N.check(N.lib().mi_sim_time_launches(view.handle, 1, 8), "mi_sim_time_launches")
    for k in range(3):
        o0 = envs[0].step(acts[k])
        o1 = envs[1].step(acts[k])
        for a, b in zip((o0[0]["obs"], o0[1], o0[2]), (o1[0]["obs"], o1[1], o1[2])):
            assert torch.equal(a, b)
    cnt, ms = _times(view, 8)
    assert cnt == 3 and len(ms) == 3 and all(0.0 < x < 50.0 for x in ms), (cnt, ms)
    N.check(N.lib().mi_sim_time_launches(view.handle, 0, 0), "mi_sim_time_launches")
    for e in envs:
        e.close()


@pytest.mark.parametrize("var,kernel", [("32p", "k_loco_post_pipe"), ("32s", "k_loco_post_tiled<32s>")])
def test_each_post_step_kernel_timed_equals_untimed(gpu, monkeypatch, var, kernel):
    """The pipelined and the one-tile post-step through the one launch path: a timed launch writes
    what the untimed one writes from the same buffers. MI_POST_GRID=1 on 96 envs (three tiles on
    one workgroup) makes the pipelined kernel take this small a batch."""
    n = 96
    env = make_env("Humanoid", num_envs=n, device="cuda:0", seed=4)
    t, view = env.task, env.task.get_robot()
    env.reset()
    env.step(torch.rand((n, t.num_actions), device="cuda:0") * 2 - 1)
    t.obs_buf.zero_()           # the fused step already wrote this state's rows: start from blank ones
    t.rew_buf.zero_()
    torch.cuda.synchronize()
    monkeypatch.setenv("MI_POST_TILE", var)
    monkeypatch.setenv("MI_POST_GRID", "1")
    bufs = ("obs_buf", "rew_buf", "reset_buf", "progress_buf", "potentials", "prev_potentials")
    start = {b: getattr(t, b).clone() for b in bufs}
    h = view.handle
    out = []
    for every in (0, 1):
        for b in bufs:
            getattr(t, b).copy_(start[b])
        N.check(N.lib().mi_sim_time_launches(h, every, 4), "mi_sim_time_launches")
        N.check(N.lib().mi_task_post_step(h, t.actions.data_ptr(), t.obs_buf.data_ptr(), t.rew_buf.data_ptr(),
                                          t.reset_buf.data_ptr(), t.progress_buf.data_ptr(),
                                          t.potentials.data_ptr(), t.prev_potentials.data_ptr(), view.stream()),
                "mi_task_post_step")
        torch.cuda.synchronize()
        assert view.post_kernel()[0] == kernel
        out.append({b: getattr(t, b).clone() for b in bufs})
        if every:
            cnt, ms = _times(view, 4)
            assert cnt == 1 and 0.0 < ms[0] < 50.0, (cnt, ms)
    assert not torch.equal(out[0]["obs_buf"], start["obs_buf"])
    for b in bufs:
        assert torch.equal(out[0][b], out[1][b]), b
    N.check(N.lib().mi_sim_time_launches(h, 0, 0), "mi_sim_time_launches")
    env.close()
