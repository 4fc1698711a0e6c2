"""Reference of the implicit PD joint drives (include/mi_drive.h, include/mi_sim.h
mi_set_drive_gains / mi_set_drive_targets). Helper module, not a test.

- ``drive_damping`` / ``drive_effort``: the header's two functions restated in float32 numpy, one
  rounding per operation in the header's order (the device and the C build are held to these bits).
- ``implicit_substep``: one contact-free, limit-free substep under a drive in float64, stated as the
  IMPLICIT equation itself (the spring and damper evaluated at the end state q+ = q + dt u+), on
  tests/dyn_ref.py's M, c, g and tests/msolve_ref.py's tree solve of that one matrix:
      (M + arm + dt B + dt kd + dt^2 kp) (u+ - u) = dt (tau + kp (q* - q - dt u) + kd (qd* - u) - c - g - B u)
- ``reduced_substep``: the same substep the way the stepper takes it, a drive-free substep of
  tests/msolve_ref.py (tree LTDL) with damping B_E and effort tau + F_d.
- ``hold_pose``: implicit substeps in a row (float64), for the pose-holding test."""
from __future__ import annotations

import numpy as np

from tests.msolve_ref import MassSolve

F32 = np.float32


def drive_damping(damp, kp, kd, dt):
    """(damp + kd) + dt*kp in float32."""
    damp, kp, kd, dt = (np.asarray(x, F32) for x in (damp, kp, kd, dt))
    a = (damp + kd).astype(F32)
    b = (dt * kp).astype(F32)
    return (a + b).astype(F32)


def drive_effort(eff, kp, kd, q, qt, qdt):
    """(eff + kp*(qt - q)) + kd*qdt in float32."""
    eff, kp, kd, q, qt, qdt = (np.asarray(x, F32) for x in (eff, kp, kd, q, qt, qdt))
    e = (qt - q).astype(F32)
    s = (kp * e).astype(F32)
    a = (eff + s).astype(F32)
    d = (kd * qdt).astype(F32)
    return (a + d).astype(F32)


def _joint(model, values, n, dtype=np.float64):
    return np.broadcast_to(np.asarray(values).astype(dtype), (n, model.num_dof))


def implicit_substep(model, st, dt, tau, kp, kd, qt, qdt, gravity=(0.0, 0.0, -9.81), armature=None, damping=None):
    """u+ [n,nv] (float64) of one contact-free, limit-free substep with the drive solved implicitly."""
    f = np.float64
    n = st["q"].shape[0]
    arm = _joint(model, model.armature[1:] if armature is None else armature, n)
    B = _joint(model, model.damping[1:] if damping is None else damping, n)
    kp, kd, qt, qdt, tau = (_joint(model, x, n) for x in (kp, kd, qt, qdt, tau))
    # the implicit matrix as ONE diagonal on M (mode "armature" adds its armature argument and nothing else)
    ms = MassSolve(model, st, dt, "armature", gravity=gravity, armature=arm + dt * B + dt * kd + dt * dt * kp, dtype=f)
    nr, u = ms.nr, ms.u
    q, uj = st["q"].astype(f), u[:, nr:]
    rhs = -ms.dyn.c - ms.dyn.g
    rhs[:, nr:] += tau + kp * (qt - q - dt * uj) + kd * (qdt - uj) - B * uj
    du = ms.solve(dt * rhs)
    return u + du


def reduced_substep(model, st, dt, tau, kp, kd, qt, qdt, gravity=(0.0, 0.0, -9.81), armature=None, damping=None,
                    dtype=np.float64):
    """The same u+ as a DRIVE-FREE substep with damping B_E = B + kd + dt kp and efforts tau + F_d."""
    n = st["q"].shape[0]
    B = _joint(model, model.damping[1:] if damping is None else damping, n, dtype)
    kp, kd, qt, qdt, tau = (_joint(model, x, n, dtype) for x in (kp, kd, qt, qdt, tau))
    BE = B + kd + dtype(dt) * kp
    eff = tau + kp * (qt - st["q"].astype(dtype)) + kd * qdt
    ms = MassSolve(model, st, dt, "stepper", gravity=gravity, armature=armature, damping=BE, dtype=dtype)
    return ms.u + dtype(dt) * ms.forward_dynamics(eff)


def _quat_mul(a, b):
    w1, x1, y1, z1 = a.T
    w2, x2, y2, z2 = b.T
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=1)


def advance(model, st, dt, u1):
    """The state after the substep's position update with the new velocity u1 (float64): joints and
    root position by dt u+, the root orientation by the exact rotation of its world angular velocity."""
    nr = 6 if model.root_free else 0
    out = {k: np.array(v, np.float64) for k, v in st.items()}
    out["qd"] = u1[:, nr:].copy()
    out["q"] = out["q"] + dt * out["qd"]
    if nr:
        out["vel"] = u1[:, :6].copy()
        out["pos"] = out["pos"] + dt * u1[:, :3]
        w = u1[:, 3:6]
        ang = np.linalg.norm(w, axis=1) * dt
        axis = w / np.maximum(np.linalg.norm(w, axis=1), 1e-300)[:, None]
        dq = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], axis=1)
        r = _quat_mul(dq, out["rot"])
        out["rot"] = r / np.linalg.norm(r, axis=1)[:, None]
    return out


def hold_pose(model, st, dt, kp, kd, qt, steps, gravity=(0.0, 0.0, 0.0), tol=None):
    """max |q - q*| after each of ``steps`` implicit substeps from ``st`` (float64, no efforts, no
    velocity target); stops early once it is below ``tol``."""
    errs = []
    cur = {k: np.array(v, np.float64) for k, v in st.items()}
    for _ in range(steps):
        u1 = implicit_substep(model, cur, dt, 0.0, kp, kd, qt, 0.0, gravity=gravity)
        cur = advance(model, cur, dt, u1)
        errs.append(float(np.abs(cur["q"] - np.asarray(qt, np.float64)).max()))
        if tol is not None and errs[-1] < tol:
            break
    return errs
