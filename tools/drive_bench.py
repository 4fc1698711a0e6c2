"""Fused env-step time of 4096 Humanoid envs (one GPU) without the per-env parameter table, with it,
and with joint drives set (skipped on a build without them, so the same script times a parent
checkout): python tools/drive_bench.py [out.json]; profiles/drive/timing.json."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from omniisaacgymenvs_amd.utils.task_util import make_env

n = 4096
env = make_env("Humanoid", num_envs=n, device="cuda:0", seed=1)
env.reset()
view = env.task.get_robot()
gen = torch.Generator().manual_seed(1)
acts = [(torch.rand((n, env.num_actions), generator=gen) * 2 - 1).cuda() for _ in range(8)]

def timed(reps=200, rounds=5):
    out = []
    for _ in range(rounds):
        for k in range(20):
            env.step(acts[k % 8])
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(reps):
            env.step(acts[k % 8])
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))

res = {"env_step_plain_us": timed()}
view.set_armatures(view.get_armatures())
res["env_step_table_us"] = timed()
if hasattr(view, "set_gains"):
    D = view.num_dof
    lo, hi = view.model.lower[1:], view.model.upper[1:]
    view.set_gains(torch.full((n, D), 50.0), torch.full((n, D), 1.0))
    view.set_joint_position_targets(torch.as_tensor(np.tile((lo + hi) / 2, (n, 1)).astype(np.float32)))
    res["env_step_table_drive_us"] = timed()
    view.clear_joint_drives()
    res["env_step_table_drive_cleared_us"] = timed()
res["nan_count"] = view.nan_count()
print(json.dumps(res))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
env.close()
