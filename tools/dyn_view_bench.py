#!/usr/bin/env python
"""Store bandwidth of the dynamics view kernel (mi_get_dynamics, csrc/mi_dyn.hpp) at a user-sized
batch, next to the link-frame Jacobian kernel in the same process.

    python tools/dyn_view_bench.py [--num-envs 4096] [--tasks Humanoid,Ant] [--launches 200] [--out FILE.json]

Time: device events around `launches` back-to-back launches of one call (after a warm-up of the
same shape), seven windows; reported are the median window over its launch count, and the fastest
and slowest window — a mean per launch that includes the launch gaps, so a lower bound on the
kernel's own rate; the kernel alone is in a `rocprofv3 --kernel-trace --stats` run of this script
(profiles/dyn_view/). Bytes: algorithmic, from the shapes — 4 (13 + 2 D) read; 4 (nv^2 + 2 nv)
written for all three outputs, 4 nv^2 for M alone; the Jacobian of all bodies writes 4 * 6 nv K.
Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
WINDOWS = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--tasks", default="Humanoid,Ant")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from omniisaacgymenvs_amd import native as N
    from omniisaacgymenvs_amd.utils.task_util import make_env

    assert torch.cuda.is_available(), "dyn_view_bench needs a GPU"
    n = args.num_envs
    out = {"num_envs": n, "launches": args.launches, "windows": WINDOWS,
           "timing": "device events around back-to-back launches; median, min, max of the windows / launches"}
    for task in args.tasks.split(","):
        env = make_env(task, num_envs=n, device="cuda:0", seed=3)
        env.reset()
        view = env.task.get_robot()
        m = view.model
        nv, D = view.num_gen_vel, m.num_dof
        links = np.ascontiguousarray(m.body_link, np.int32)
        offs = np.ascontiguousarray(m.body_offset, np.float32)
        K = len(links)
        f = dict(dtype=torch.float32, device="cuda:0")
        M, c, g = torch.empty((n, nv, nv), **f), torch.empty((n, nv), **f), torch.empty((n, nv), **f)
        jac = torch.empty((n, K, 6, nv), **f)
        lib, h, st = N.lib(), view.handle, view.stream()
        calls = (
            ("k_dynamics_all", lambda: lib.mi_get_dynamics(h, M.data_ptr(), c.data_ptr(), g.data_ptr(), st), 4 * (nv * nv + 2 * nv)),
            ("k_dynamics_M", lambda: lib.mi_get_dynamics(h, M.data_ptr(), None, None, st), 4 * nv * nv),
            ("k_link_jacobian_bodies", lambda: lib.mi_get_link_jacobian(h, N.iptr(links), N.fptr(offs), K, jac.data_ptr(), st),
             4 * 6 * nv * K),
        )
        read = 4 * (13 + 2 * D)
        res = {"nv": nv, "D": D, "K": K}
        for name, fn, wr in calls:
            for _ in range(20):
                assert fn() == 0
            torch.cuda.synchronize()
            ms = []
            for _ in range(WINDOWS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / args.launches)
            t = sorted(ms)[WINDOWS // 2]
            res[name] = {"us_per_launch": round(t * 1e3, 2), "us_min": round(min(ms) * 1e3, 2),
                         "us_max": round(max(ms) * 1e3, 2), "algo_bytes_per_env": {"read": read, "write": wr},
                         "store_GBs": round(wr * n / (t * 1e-3) / 1e9, 1),
                         "frac_of_peak": round((read + wr) * n / (t * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        res["store_rate_vs_jacobian"] = round(res["k_dynamics_all"]["store_GBs"] / res["k_link_jacobian_bodies"]["store_GBs"], 3)
        out[task] = res
        env.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
