#!/usr/bin/env python
"""Time of the mass-matrix solve view (mi_solve_mass, mi_get_forward_dynamics,
mi_get_link_task_inertia; csrc/mi_msolve.hpp) at a user-sized batch, next to what a user had before
it, in the same process: get_dynamics() + torch.linalg.solve for the solves and forward dynamics,
get_jacobians() + torch.linalg.inv(Mt) + two bmm for the task-space inertia.

    python tools/msolve_bench.py [--num-envs 4096] [--tasks Humanoid,Ant] [--launches 200] [--out FILE.json]

Time: device events around `launches` back-to-back calls (after a warm-up of the same shape),
seven windows; reported are the median window over its call count and the fastest and slowest
window — a mean per call that includes the launch gaps (for the torch paths: of every kernel they
launch). Bytes: algorithmic, from the shapes — 4 (13 + 2 D) + 4 R nv read, 4 R nv written per env
for a solve; the task call writes 4 (6K nv + 36 K^2). Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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

    assert torch.cuda.is_available(), "msolve_bench needs a GPU"
    n = args.num_envs
    out = {"num_envs": n, "launches": args.launches, "windows": WINDOWS,
           "timing": "device events around back-to-back calls; median, min, max of the windows / calls"}

    def timed(fn, launches):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(WINDOWS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / launches)
        return {"us_per_call": round(sorted(ms)[WINDOWS // 2] * 1e3, 2), "us_min": round(min(ms) * 1e3, 2),
                "us_max": round(max(ms) * 1e3, 2)}

    for task in args.tasks.split(","):
        env = make_env(task, num_envs=n, device="cuda:0", seed=3)
        env.reset()
        view = env.task.get_robot()
        m = view.model
        nv, D, nr = view.num_gen_vel, m.num_dof, 6 if m.root_free else 0
        dt = float(view.sim_params.dt)
        links, offs = view._frames(None)
        K = len(links)
        foot = [m.body_names[-1]]
        l1, o1 = view._frames(foot)
        f = dict(dtype=torch.float32, device="cuda:0")
        gen = torch.Generator(device="cuda:0").manual_seed(1)
        rhs = {R: torch.rand((n, R, nv), generator=gen, **f) * 2 - 1 for R in (1, 6)}
        x = {R: torch.empty((n, R, nv), **f) for R in (1, 6)}
        acc = torch.empty((n, nv), **f)
        mj = {k: torch.empty((n, 6 * k, nv), **f) for k in (1, K)}
        lam = {k: torch.empty((n, 6 * k, 6 * k), **f) for k in (1, K)}
        tau = torch.rand((n, D), generator=gen, **f)
        view.set_joint_efforts(tau)
        diag = torch.zeros((n, nv), **f)
        diag[:, nr:] = view.get_armatures() + dt * view.get_joint_dampings()
        lib, h, st = N.lib(), view.handle, view.stream()

        def mt():
            M = view.get_mass_matrices(clone=False)
            return M + torch.diag_embed(diag)

        def torch_solve(R):
            return torch.linalg.solve(mt(), rhs[R].transpose(1, 2)).transpose(1, 2)

        def torch_fd():
            M, c, g = view.get_dynamics(clone=False)
            r = -c - g
            r[:, nr:] += tau - view.get_joint_dampings() * view.get_joint_velocities(clone=False)
            return torch.linalg.solve(M + torch.diag_embed(diag), r.unsqueeze(2)).squeeze(2)

        def torch_task(names):
            J = view.get_jacobians(names)
            J = J.reshape(n, -1, nv)
            X = torch.bmm(J, torch.linalg.inv(mt()))
            return X, torch.bmm(X, J.transpose(1, 2))

        calls = (
            ("forward_dynamics", lambda: lib.mi_get_forward_dynamics(h, 1, None, acc.data_ptr(), st), torch_fd, 1),
            ("solve_R1", lambda: lib.mi_solve_mass(h, 1, rhs[1].data_ptr(), 1, x[1].data_ptr(), st), lambda: torch_solve(1), 1),
            ("solve_R6", lambda: lib.mi_solve_mass(h, 1, rhs[6].data_ptr(), 6, x[6].data_ptr(), st), lambda: torch_solve(6), 6),
            ("task_K1", lambda: lib.mi_get_link_task_inertia(h, 1, N.iptr(l1), N.fptr(o1), 1, mj[1].data_ptr(),
                                                             lam[1].data_ptr(), st), lambda: torch_task(foot), 6),
            (f"task_K{K}", lambda: lib.mi_get_link_task_inertia(h, 1, N.iptr(links), N.fptr(offs), K, mj[K].data_ptr(),
                                                                lam[K].data_ptr(), st), lambda: torch_task(None), 6 * K),
        )
        res = {"nv": nv, "D": D, "K": K}
        for name, fused, base, R in calls:
            assert fused() == 0
            a, b = timed(fused, args.launches), timed(base, max(args.launches // 10, 5))
            res[name] = {"fused": a, "torch": b, "speedup": round(b["us_per_call"] / a["us_per_call"], 2),
                         "algo_bytes_per_env": {"read": 4 * (13 + 2 * D) + (4 * R * nv if name.startswith("solve") else 0),
                                                "write": 4 * R * nv + (4 * R * R if name.startswith("task") else 0)}}
        # the two paths compute the same thing
        torch.cuda.synchronize()
        lib.mi_solve_mass(h, 1, rhs[6].data_ptr(), 6, x[6].data_ptr(), st)
        ref = torch_solve(6)
        res["solve_R6_vs_torch_rel"] = float(((x[6] - ref).abs().amax((1, 2)) / ref.abs().amax((1, 2))).max())
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
