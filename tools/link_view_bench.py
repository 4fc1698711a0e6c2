#!/usr/bin/env python
"""Store bandwidth of the link-frame view kernels (mi_get_link_state / mi_get_link_jacobian,
csrc/mi_link.hpp) at a user-sized batch, next to the obs/reward fuse on the same box.

    python tools/link_view_bench.py [--num-envs 4096] [--task Humanoid] [--frames bodies|links]
                                    [--launches 200] [--out FILE.json] [--no-fuse]

Time: device events around `launches` back-to-back launches of one getter (after a warm-up of the
same shape), five windows, the median window over its launch count — a mean per launch that
includes the launch gaps, so a lower bound on the kernel's own rate; the kernel alone is in a
`rocprofv3 --kernel-trace --stats` run of this script (profiles/link_view/). Bytes: algorithmic,
from the shapes — 4 (13 + 2 D) read and 4 * 13 K or 4 * 6 nv K written per env. Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--task", default="Humanoid")
    ap.add_argument("--frames", choices=["bodies", "links"], default="bodies")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-fuse", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    from omniisaacgymenvs_amd import native as N
    from omniisaacgymenvs_amd.utils.task_util import make_env

    assert torch.cuda.is_available(), "link_view_bench needs a GPU"
    n = args.num_envs
    env = make_env(args.task, num_envs=n, device="cuda:0", seed=3)
    env.reset()
    view = env.task.get_robot()
    m = view.model
    if args.frames == "bodies":
        links = np.ascontiguousarray(m.body_link, np.int32)
        offs = np.ascontiguousarray(m.body_offset, np.float32)
    else:
        links, offs = np.arange(m.num_links, dtype=np.int32), None
    K, nv, D = len(links), view.num_gen_vel, m.num_dof
    f = dict(dtype=torch.float32, device="cuda:0")
    pos, quat, vel = torch.empty((n, K, 3), **f), torch.empty((n, K, 4), **f), torch.empty((n, K, 6), **f)
    jac = torch.empty((n, K, 6, nv), **f)
    lib, h, st = N.lib(), view.handle, view.stream()

    def state():
        return lib.mi_get_link_state(h, N.iptr(links), N.fptr(offs), K, pos.data_ptr(), quat.data_ptr(),
                                     vel.data_ptr(), st)

    def jacobian():
        return lib.mi_get_link_jacobian(h, N.iptr(links), N.fptr(offs), K, jac.data_ptr(), st)

    read = 4 * (13 + 2 * D)
    out = {"task": args.task, "num_envs": n, "frames": args.frames, "K": K, "nv": nv, "launches": args.launches,
           "timing": "device events around back-to-back launches, median of 5 windows / launches"}
    for name, fn, wr in (("k_link_state", state, 4 * 13 * K), ("k_link_jacobian", jacobian, 4 * 6 * nv * K)):
        for _ in range(10):
            assert fn() == 0
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.launches)
        t = sorted(ms)[2]
        gbs = (read + wr) * n / (t * 1e-3) / 1e9
        out[name] = {"ms_per_launch": round(t, 5), "windows_ms": [round(x, 5) for x in ms],
                     "algo_bytes_per_env": {"read": read, "write": wr}, "achieved": round(gbs, 1),
                     "store_only": round(wr * n / (t * 1e-3) / 1e9, 1), "unit": "GB/s", "peak": HBM_PEAK_GBS,
                     "frac": round(gbs / HBM_PEAK_GBS, 4)}
    if not args.no_fuse:
        from fuse_roofline import measure
        out["obs_reward_fuse_same_box"] = measure(args.task, n, 30, env=env)
    env.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
