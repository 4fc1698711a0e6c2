#!/usr/bin/env python
"""Time of the contact view (mi_get_contacts, mi_get_contact_jacobian, mi_get_link_contact_summary;
csrc/mi_contact.hpp) at a user-sized batch, next to mi_get_link_state over all links in the same
process (the same forward kinematics without detection, compaction and contact stores) and, for
Ant's ground-only case, next to a torch composition of mi_get_contacts' outputs from
get_link_view poses. Writes profiles/contact_view/README.md.

    python tools/contact_view_bench.py [--num-envs 4096] [--tasks Humanoid,Ant] [--launches 200] [--out FILE.md]

Time: device events around `launches` back-to-back calls (after a warm-up of the same shape), seven
windows; reported are the median window over its call count and the fastest and slowest window.
Needs a GPU."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOWS = 7
DATA, JAC, SUMMARY = 0, 1, 2


def ct_lds(op, E, L, D, nv, C, K):
    """Bytes of LDS per workgroup: CtLds of csrc/mi_contact.hpp, restated."""
    al4 = lambda x: (x + 3) & ~3
    o = al4(4 * E * C) if op == JAC else 0
    o += al4(E * (13 + 2 * D)) + al4(E * (12 * L + 1)) + al4(E) + al4(E * C * 2)
    o += al4(E * C * 3) if op != SUMMARY else 0
    o += al4(E * C * 9) if op == JAC else al4(E * C * 3) if op == DATA else 0
    o += al4(E * C) if op == DATA else 0
    o += al4(E * 6 * nv) + al4(nv) if op == JAC else 0
    o += 2 * al4(E * K) if op == SUMMARY else 0
    return 4 * o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--tasks", default="Humanoid,Ant")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contact_view", "README.md"))
    args = ap.parse_args()

    import numpy as np
    import torch

    from omniisaacgymenvs_amd import native as N
    from omniisaacgymenvs_amd.utils.task_util import make_env

    assert torch.cuda.is_available(), "contact_view_bench needs a GPU"
    n = args.num_envs

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
        return sorted(ms)[WINDOWS // 2] * 1e3, min(ms) * 1e3, max(ms) * 1e3

    rows, notes = [], []
    for task in args.tasks.split(","):
        env = make_env(task, num_envs=n, device="cuda:0", seed=3)
        env.reset()
        view = env.task.get_robot()
        m = view.model
        g = torch.Generator().manual_seed(1)
        for _ in range(30):                                # bodies on the ground: a populated contact set
            env.step((torch.rand((n, env.num_actions), generator=g) * 2 - 1).cuda())
        L, D, nv, C = m.num_links, m.num_dof, view.num_gen_vel, view.max_contacts
        lib, h, st = N.lib(), view.handle, view.stream()
        f32, i32 = dict(dtype=torch.float32, device="cuda:0"), dict(dtype=torch.int32, device="cuda:0")
        cnt, lnk = torch.empty((n,), **i32), torch.empty((n, C, 2), **i32)
        pt, nr, gp = torch.empty((n, C, 3), **f32), torch.empty((n, C, 3), **f32), torch.empty((n, C), **f32)
        J = torch.empty((n, C, 3, nv), **f32)
        feet = [b for b in m.body_names if "foot" in b] or [m.body_names[-1]]
        fl = np.ascontiguousarray([m.body_link[m.get_body_index(b)] for b in feet], dtype=np.int32)
        K = len(fl)
        fc, fr = torch.empty((n, K), **i32), torch.empty((n, K), **f32)
        al = np.arange(L, dtype=np.int32)
        lp, lq, lv = torch.empty((n, L, 3), **f32), torch.empty((n, L, 4), **f32), torch.empty((n, L, 6), **f32)
        calls = [
            ("mi_get_contacts (all five outputs)", lambda: lib.mi_get_contacts(
                h, cnt.data_ptr(), lnk.data_ptr(), pt.data_ptr(), nr.data_ptr(), gp.data_ptr(), st),
             4 * (1 + 9 * C)),
            ("mi_get_contact_jacobian", lambda: lib.mi_get_contact_jacobian(h, J.data_ptr(), st), 4 * 3 * C * nv),
            (f"mi_get_link_contact_summary ({K} feet)", lambda: lib.mi_get_link_contact_summary(
                h, N.iptr(fl), K, fc.data_ptr(), fr.data_ptr(), st), 8 * K),
            (f"mi_get_link_state (all {L} links: the same FK)", lambda: lib.mi_get_link_state(
                h, N.iptr(al), None, L, lp.data_ptr(), lq.data_ptr(), lv.data_ptr(), st), 4 * 13 * L),
        ]
        if not len(m.pairs) or not view.sim_params.enable_self_collisions:
            # ground-only: the same five outputs composed in torch from the bodies' poses
            links = torch.as_tensor(np.asarray(m.body_link), device="cuda:0").long()
            assert set(int(x) for x in m.geom_link) <= set(int(x) for x in m.body_link)
            body_of_link = {int(l): b for b, l in enumerate(m.body_link)}
            pts = [(gi, e) for gi in range(m.num_geoms) for e in ((0, 1) if m.geom_type[gi] == 1 else (0,))]
            pb = torch.as_tensor([body_of_link[int(m.geom_link[gi])] for gi, _ in pts], device="cuda:0").long()
            pl = torch.as_tensor(np.stack([(m.geom_p1 if e else m.geom_p0)[gi] - m.body_offset[body_of_link[int(m.geom_link[gi])]]
                                           for gi, e in pts]), **f32)
            pr = torch.as_tensor(np.asarray([m.geom_radius[gi] for gi, _ in pts]), **f32)
            plink = links[pb].to(torch.int32)
            bodies = view.get_link_view(list(m.body_names))
            off = float(view.sim_params.contact_offset)
            B = m.num_bodies

            def torch_contacts():
                p, q = bodies.get_world_poses(clone=False)
                p, q = p.view(n, B, 3)[:, pb], q.view(n, B, 4)[:, pb]
                w, v = q[..., :1], q[..., 1:]
                t = 2 * torch.cross(v, pl.expand_as(v), dim=-1)
                x = p + pl + w * t + torch.cross(v, t, dim=-1)
                gap = x[..., 2] - pr
                act = gap < off
                count = act.sum(1, dtype=torch.int32)
                order = torch.argsort((~act).to(torch.int8), dim=1, stable=True)[:, :C]
                keep = torch.arange(order.shape[1], device="cuda:0")[None] < count[:, None]
                xo = torch.gather(x, 1, order[..., None].expand(-1, -1, 3))
                xo[..., 2] -= pr[order]
                point = torch.where(keep[..., None], xo, 0.0)
                normal = torch.zeros_like(point)
                normal[..., 2] = keep
                la = torch.where(keep, plink[order], -1)
                return count, torch.stack([la, torch.full_like(la, -1)], -1), point, normal, torch.where(keep, torch.gather(gap, 1, order), 0.0)

            calls.append(("torch composition of mi_get_contacts from get_link_view poses", torch_contacts, 4 * (1 + 9 * C)))
            assert lib.mi_get_contacts(h, cnt.data_ptr(), lnk.data_ptr(), pt.data_ptr(), nr.data_ptr(), gp.data_ptr(), st) == 0
            tc = torch_contacts()
            same = float((tc[0] == cnt).float().mean())
            notes.append(f"{task}: the torch composition's `count` equals the fused call's in {100 * same:.2f} % of the envs "
                         f"(float32 poses rounded through the body frames; candidates at the threshold), "
                         f"largest |gap| difference {float((tc[4] - gp).abs().max()):.2e} m.")
        torch.cuda.synchronize()
        assert lib.mi_get_contacts(h, cnt.data_ptr(), lnk.data_ptr(), pt.data_ptr(), nr.data_ptr(), gp.data_ptr(), st) == 0
        torch.cuda.synchronize()
        notes.append(f"{task}: L = {L}, nv = {nv}, C = {C}; contacts per env at the timed state: mean "
                     f"{float(cnt.float().mean()):.2f}, max {int(cnt.max())}; LDS per workgroup: contacts "
                     f"{ct_lds(DATA, 8, L, D, nv, C, 0)} B (8 envs), Jacobian {ct_lds(JAC, 4, L, D, nv, C, 0)} B (4 envs), "
                     f"summary {ct_lds(SUMMARY, 8, L, D, nv, C, K)} B.")
        for name, fn, wbytes in calls:
            launches = args.launches if name.startswith("mi_") else max(args.launches // 10, 5)
            med, lo, hi = timed(fn, launches)
            rows.append(f"| {task} | {name} | {med:.1f} | {lo:.1f} | {hi:.1f} | {wbytes} | {wbytes * n / med / 1e3:.1f} |")
        env.close()
    big = dict(L=33, D=32, nv=38, C=42)
    text = [
        "# Contact view kernel `k_contacts`: evidence (one MI355X)", "",
        "`mi_get_contacts`, `mi_get_contact_jacobian`, `mi_get_link_contact_summary` (`csrc/mi_contact.hpp`, DESIGN §2",
        "\"Contact view\"). Written by `tools/contact_view_bench.py`.", "",
        f"## Time ({n} envs, after 30 random-action env steps; device events around back-to-back calls, median / min / max of {WINDOWS} windows, µs per call)", "",
        "| task | call | median | min | max | bytes written per env | GB/s of stores |", "|---|---|---|---|---|---|---|", *rows, "",
        *[f"- {x}" for x in notes], "",
        "## Resources", "",
        "VGPRs, scratch (0 B) and static LDS (none) of the three instantiations: `isa_identity.txt` (the compiler's resource lines).",
        f"Largest model `mi_sim_create` accepts (L = 33, nv = 38, C = 42), LDS per workgroup: contacts {ct_lds(DATA, 8, K=0, **big)} B, "
        f"Jacobian {ct_lds(JAC, 4, K=0, **big)} B, summary over all 33 links {ct_lds(SUMMARY, 8, K=33, **big)} B, of the 65 536 B limit; "
        "the host halves the env tile until a workgroup fits.", "",
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(text))
    print("\n".join(text))


if __name__ == "__main__":
    main()
