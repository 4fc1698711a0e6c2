"""Inverse-dynamics view on the GPU (include/mi_sim.h mi_get_inverse_dynamics /
mi_get_link_acceleration / mi_get_momentum and the view methods on top) against the numpy
reference of tests/idyn_ref.py.

Tolerance: the rule of tests/test_gpu_link_view.py / test_gpu_dyn_view.py. The reference runs twice
on the float32 state read back from the device, in float64 and in float32; the device may be off
the float64 run by 4x the float32 run's worst deviation per output, floored at 2 ulp of the
output's magnitude. Measured (MI355X, N = 257, device error / bound): Humanoid tau 1.6e-4 / 6.0e-4,
joint_wrench 1.6e-4 / 5.4e-4, accelerations of all links with offsets 2.6e-5 / 1.0e-4, com 1.8e-6 /
4.6e-5, mom 2.4e-5 / 4.9e-3, cmm 4.2e-6 / 1.9e-3, kinetic energy 8.8e-5 / 2.3e-3, potential 2.4e-4 /
9.6e-4; Ant tau 2.8e-6 / 1.0e-5 (acc = NULL: 2.3e-6 / 3.1e-6, the largest ratio, 0.73), accelerations
4.9e-6 / 1.8e-5; Cartpole tau 3.6e-6 / 1.7e-5, joint_wrench 7.8e-6 / 3.9e-5, accelerations 1.3e-6 /
6.8e-6. The root frame of a floating base is acc[:, 0:6] itself (error 0). Every case prints device
error, bound and ratio (pytest -s); profiles/idyn_view/README.md has the measured table.

Stepper consistency: with a = (u1 - u0) / dt over one mi_sim_step(1) in free flight (the set-up of
the dyn-view test), mi_get_inverse_dynamics(a, MI_MASS_STEPPER) at state 0 returns the efforts that
were set on the joint DOFs and 0 on the root's. The same limits as there: the residual of the
float64 terms below 1e-3 of |tau - c - g|, the device's within 2x that plus bound(M) |a|.
Measured (N = 16, float64 terms / device / limit): Ant 5.6e-6 / 5.2e-6 / 8.6e-5 at |tau - c - g| =
9.1; Humanoid 2.1e-4 / 2.5e-4 / 5.4e-3 at 430."""
import numpy as np
import pytest
import torch

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.utils.task_util import make_env
from tests.idyn_ref import MODES, InverseDynamics
from tests.link_ref import Kinematics, integrate, random_state
from tests.msolve_ref import MassSolve
from tests.test_gpu_dyn_view import _free_flight, _u, dynamics, refs_and_bounds, sim_gravity
from tests.test_gpu_link_view import link_jac, read_state, write_state
from tests.test_gpu_msolve import bound_of, forward

pytestmark = pytest.mark.gpu
CASES = [("Humanoid", 257), ("Ant", 257), ("Cartpole", 257), ("Ant", 1)]
EPS = float(np.finfo(np.float32).eps)
E_NULL, E_SHAPE, E_ARG = -1, -2, -5
NAN = float("nan")


# ---- device calls: fresh NaN-filled buffers, skipped outputs pass NULL ----
def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def inverse_dynamics(view, which, acc=None, tau=True, wrench=True):
    n, nv, L = view.count, view.num_gen_vel, view.model.num_links
    t = {"tau": torch.full((n, nv), NAN, device="cuda:0") if tau else None,
         "wrench": torch.full((n, L, 6), NAN, device="cuda:0") if wrench else None}
    a = _dev(acc)
    rc = N.lib().mi_get_inverse_dynamics(view.handle, which, N.ptr(a), N.ptr(t["tau"]), N.ptr(t["wrench"]), view.stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in t.items() if v is not None}


def link_acc(view, links, offs, acc=None, K=None, out=True):
    ids = np.ascontiguousarray(links, dtype=np.int32)
    o = None if offs is None else np.ascontiguousarray(offs, dtype=np.float32)
    K = len(ids) if K is None else K
    t = torch.full((view.count, max(K, 1), 6), NAN, device="cuda:0") if out else None
    a = _dev(acc)
    rc = N.lib().mi_get_link_acceleration(view.handle, N.iptr(ids), N.fptr(o), K, N.ptr(a), N.ptr(t), view.stream())
    torch.cuda.synchronize()
    return rc, None if t is None else t.cpu().numpy()


MOM_KINDS = ("com", "mom", "cmm", "energy")


def momentum(view, **on):
    n, nv = view.count, view.num_gen_vel
    shape = {"com": (n, 3), "mom": (n, 6), "cmm": (n, 6, nv), "energy": (n, 2)}
    t = {k: torch.full(shape[k], NAN, device="cuda:0") if on.get(k, True) else None for k in MOM_KINDS}
    rc = N.lib().mi_get_momentum(view.handle, *(N.ptr(t[k]) for k in MOM_KINDS), view.stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in t.items() if v is not None}


# ---- the bound ----
def bound(x32, x64):
    return max(4.0 * float(np.abs(x32 - x64).max()), 2.0 * EPS * float(np.abs(x64).max()))


def check(tag, dev, x32, x64):
    b = bound(x32, x64)
    err = float(np.abs(dev.astype(np.float64) - x64).max())
    print(f"{tag}: device error {err:.3e} bound {b:.3e} ratio {err / b if b else float(err > 0):.2f}")
    assert np.isfinite(dev).all(), tag
    assert err <= b, (tag, err, b)
    return b


def refs(view, st, **kw):
    kw.setdefault("gravity", sim_gravity(view))
    args = (view.model, st, float(view.sim_params.dt))
    return InverseDynamics(*args, **kw), InverseDynamics(*args, dtype=np.float32, **kw)


def offsets_of(L):
    return np.random.default_rng(8).uniform(-0.3, 0.3, size=(L, 3)).astype(np.float32)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def case(request, gpu):
    name, n = request.param
    env = make_env(name, num_envs=n, device="cuda:0", seed=11)
    env.reset()
    view = env.task.get_robot()
    m = view.model
    write_state(view, random_state(m, n, view.env_origins, seed=17))
    st = read_state(view)
    acc = np.random.default_rng(21).uniform(-10, 10, size=(n, view.num_gen_vel)).astype(np.float32)
    c = dict(name=name, n=n, env=env, view=view, model=m, st=st, acc=acc, tag=f"{name}-{n}",
             links=list(range(m.num_links)), offs=offsets_of(m.num_links))
    c["r64"], c["r32"] = refs(view, st)
    yield c
    env.close()


# ---- 1. parity ----
@pytest.mark.parametrize("with_acc", [True, False], ids=["acc", "null"])
@pytest.mark.parametrize("mode", list(MODES))
def test_parity_inverse_dynamics(case, mode, with_acc):
    view, r64, r32 = case["view"], case["r64"], case["r32"]
    acc = case["acc"] if with_acc else None
    rc, got = inverse_dynamics(view, MODES[mode], acc)
    assert rc == 0 and got["tau"].shape == (case["n"], view.num_gen_vel)
    tag = f"{case['tag']} {mode} {'acc' if with_acc else 'null'}"
    check(tag + " tau", got["tau"], r32.tau(acc, mode), r64.tau(acc, mode))
    check(tag + " joint_wrench", got["wrench"], r32.joint_wrenches(acc), r64.joint_wrenches(acc))


@pytest.mark.parametrize("with_acc", [True, False], ids=["acc", "null"])
@pytest.mark.parametrize("frames", ["root", "all_offset"])
def test_parity_link_acceleration(case, frames, with_acc):
    view, r64, r32 = case["view"], case["r64"], case["r32"]
    links, offs = ([0], None) if frames == "root" else (case["links"], case["offs"])
    acc = case["acc"] if with_acc else None
    rc, got = link_acc(view, links, offs, acc)
    assert rc == 0 and got.shape == (case["n"], len(links), 6)
    check(f"{case['tag']} acceleration {frames} {'acc' if with_acc else 'null'}", got,
          r32.frame_accelerations(links, offs, acc), r64.frame_accelerations(links, offs, acc))


def test_parity_momentum(case):
    rc, got = momentum(case["view"])
    assert rc == 0
    m64, m32 = case["r64"].momentum(), case["r32"].momentum()
    for k in MOM_KINDS:
        if k == "energy":       # two quantities of different magnitudes: each against its own bound
            for i, part in enumerate(("kinetic", "potential")):
                check(f"{case['tag']} energy {part}", got[k][:, i], m32[k][:, i], m64[k][:, i])
        else:
            check(f"{case['tag']} {k}", got[k], m32[k], m64[k])


# ---- 2. bit-exact structure ----
def _all_outputs(view, c, acc):
    out = {}
    for mode, which in MODES.items():
        rc, got = inverse_dynamics(view, which, acc)
        assert rc == 0
        out.update({f"{k}_{mode}": v for k, v in got.items()})
    rc, out["lacc"] = link_acc(view, c["links"], c["offs"], acc)
    assert rc == 0
    rc, mo = momentum(view)
    assert rc == 0
    out.update(mo)
    return out


def test_null_acc_is_zero_acc_and_output_selection(case):
    view, acc = case["view"], case["acc"]
    null, zero = _all_outputs(view, case, None), _all_outputs(view, case, np.zeros_like(acc))
    for k in null:
        assert np.array_equal(null[k], zero[k]), k
    full = _all_outputs(view, case, acc)
    again = _all_outputs(view, case, acc)                        # a rerun: the same bits
    for k in full:
        assert np.array_equal(full[k], again[k]), k
    for mode, which in MODES.items():
        rc, one = inverse_dynamics(view, which, acc, wrench=False)
        assert rc == 0 and list(one) == ["tau"] and np.array_equal(one["tau"], full[f"tau_{mode}"])
        rc, one = inverse_dynamics(view, which, acc, tau=False)
        assert rc == 0 and list(one) == ["wrench"] and np.array_equal(one["wrench"], full[f"wrench_{mode}"])
        assert np.array_equal(full[f"wrench_{mode}"], full["wrench_rigid"])      # the wrench knows no mode
    for k in MOM_KINDS:
        rc, one = momentum(view, **{x: x == k for x in MOM_KINDS})
        assert rc == 0 and list(one) == [k] and np.array_equal(one[k], full[k]), k
    # cmm columns are all zero exactly where the reference's are
    ref_zero = np.all(case["r64"].momentum()["cmm"] == 0.0, axis=1)
    assert np.array_equal(np.all(full["cmm"] == 0.0, axis=1), ref_zero)


def test_translation_invariance(case):
    view, n, acc = case["view"], case["n"], case["acc"].copy()
    if n < 2:
        return
    st = {k: v.copy() for k, v in case["st"].items()}
    for k in ("rot", "vel", "q", "qd"):
        st[k][n - 1] = st[k][0]
    acc[n - 1] = acc[0]
    assert np.abs(st["pos"][n - 1] - st["pos"][0]).max() > 0.5
    try:
        write_state(view, st)
        two = _all_outputs(view, case, acc)
        for k in two:
            if k == "com":                  # the one output that is a world position
                continue
            a, b = (two[k][0], two[k][n - 1]) if k != "energy" else (two[k][0, 0], two[k][n - 1, 0])
            assert np.array_equal(a, b), k
    finally:
        write_state(view, case["st"])
        torch.cuda.synchronize()


def test_capture(case):
    """The three calls inside torch.cuda.graph on one stream, replayed after the state changed, equal
    the eager results bit for bit; the view's getters allocate nothing after their first call."""
    view, m, n = case["view"], case["model"], case["n"]
    nv, L = view.num_gen_vel, m.num_links
    acc = _dev(case["acc"])
    links, offs = np.ascontiguousarray(case["links"], np.int32), np.ascontiguousarray(case["offs"], np.float32)
    shapes = dict(tau=(n, nv), wrench=(n, L, 6), lacc=(n, L, 6), com=(n, 3), mom=(n, 6), cmm=(n, 6, nv), energy=(n, 2))
    t = {k: torch.zeros(s, device="cuda:0") for k, s in shapes.items()}
    lib = N.lib()

    def call():
        s = view.stream()
        assert lib.mi_get_inverse_dynamics(view.handle, 1, acc.data_ptr(), t["tau"].data_ptr(), t["wrench"].data_ptr(), s) == 0
        assert lib.mi_get_link_acceleration(view.handle, N.iptr(links), N.fptr(offs), L, acc.data_ptr(), t["lacc"].data_ptr(), s) == 0
        assert lib.mi_get_momentum(view.handle, *(t[k].data_ptr() for k in MOM_KINDS), s) == 0

    def getters(rv):
        view.get_inverse_dynamics(acc, mode="stepper", clone=False)
        view.get_joint_reaction_wrenches(acc)
        view.get_coms(clone=False), view.get_momenta(clone=False), view.get_energies(clone=False)
        view.get_centroidal_momentum_matrices(clone=False)
        rv.get_accelerations(acc, clone=False)

    call()
    rv = view.get_link_view(list(m.body_names))
    getters(rv)
    torch.cuda.synchronize()
    keep = view.get_inverse_dynamics(acc, mode="stepper", clone=False)
    mem = torch.cuda.memory_allocated()
    view.get_inverse_dynamics(acc, mode="stepper", clone=False), view.get_momenta(clone=False)
    rv.get_accelerations(acc, clone=False)
    assert torch.cuda.memory_allocated() == mem
    assert torch.equal(keep, t["tau"])
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            call()
    torch.cuda.current_stream().wait_stream(s)
    first = {k: v.cpu().numpy().copy() for k, v in t.items()}
    try:
        write_state(view, random_state(m, n, view.env_origins, seed=29))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: v.cpu().numpy().copy() for k, v in t.items()}
        for v in t.values():
            v.zero_()
        call()
        torch.cuda.synchronize()
        for k, v in t.items():
            assert np.array_equal(replayed[k], v.cpu().numpy()), k
        assert not np.array_equal(replayed["tau"], first["tau"])         # the state did change
    finally:
        write_state(view, case["st"])
        torch.cuda.synchronize()


def test_python_surface(case):
    view, m, n, acc = case["view"], case["model"], case["n"], _dev(case["acc"])
    full = _all_outputs(view, case, case["acc"])
    for mode in MODES:
        assert np.array_equal(view.get_inverse_dynamics(acc, mode=mode).cpu().numpy(), full[f"tau_{mode}"])
    assert np.array_equal(view.get_inverse_dynamics().cpu().numpy(), inverse_dynamics(view, 2)[1]["tau"])
    w = view.get_joint_reaction_wrenches(acc)
    assert tuple(w.shape) == (n, m.num_bodies, 6)
    assert np.array_equal(w.cpu().numpy(), full["wrench_rigid"][:, np.asarray(m.body_link)])
    for fn, k in ((view.get_coms, "com"), (view.get_momenta, "mom"), (view.get_centroidal_momentum_matrices, "cmm"),
                  (view.get_energies, "energy")):
        a, b, cl = fn(clone=False), fn(clone=False), fn()
        assert a.data_ptr() == b.data_ptr() != cl.data_ptr() and np.array_equal(cl.cpu().numpy(), full[k]), k
    idx = torch.tensor([n - 1, 0, n // 2], device="cuda:0")
    assert torch.equal(view.get_momenta(indices=idx), view.get_momenta()[idx])
    assert torch.equal(view.get_inverse_dynamics(acc, indices=idx), view.get_inverse_dynamics(acc)[idx])
    rv = view.get_link_view(list(m.body_names))
    got = rv.get_accelerations(acc)
    links, offs = view._frames(None)
    assert tuple(got.shape) == (n, m.num_bodies, 6)
    assert np.array_equal(got.cpu().numpy(), link_acc(view, links, offs, case["acc"])[1])
    assert torch.equal(rv.get_accelerations(acc, indices=idx), got[idx])
    for bad in (view.solve_mass_matrices, ):
        with pytest.raises(ValueError):
            bad(torch.zeros((n, view.num_gen_vel), device="cuda:0"), mode="rigid")
    with pytest.raises(ValueError):
        view.get_forward_dynamics(mode="rigid")
    with pytest.raises(ValueError):
        view.get_inverse_dynamics(torch.zeros((n, 1), device="cuda:0"))


# ---- 3. consistency with the existing views, device against device ----
def test_consistency_with_the_dynamics_view(case):
    """tau_rigid == M acc + cor + grav with the device's own M, cor, grav: every term is within its
    own bound of the float64 value, for which the identity is exact."""
    view, acc, nv = case["view"], case["acc"].astype(np.float64), case["view"].num_gen_vel
    rc, dyn = dynamics(view)
    assert rc == 0
    _, _, bd = refs_and_bounds(case["model"], case["st"], sim_gravity(view))
    rc, got = inverse_dynamics(view, 2, case["acc"], wrench=False)
    assert rc == 0
    want = np.einsum("nij,nj->ni", dyn["M"].astype(np.float64), acc) + dyn["cor"] + dyn["grav"]
    b = bound(case["r32"].tau(case["acc"], "rigid"), case["r64"].tau(case["acc"], "rigid"))
    limit = b + nv * bd["M"] * float(np.abs(acc).max()) + bd["cor"] + bd["grav"]
    err = float(np.abs(got["tau"] - want).max())
    print(f"{case['tag']} tau_rigid - (M acc + cor + grav): {err:.3e} limit {limit:.3e}")
    assert err <= limit


@pytest.mark.parametrize("mode", ["armature", "stepper"])
def test_round_trip_through_forward_dynamics(case, mode):
    """acc0 = forward dynamics of random efforts; tau = inverse dynamics of acc0; forward dynamics
    of tau's joint entries gives acc0 back. With e the error of acc0 (at most the solve view's own
    bound b_fd |acc|), tau's root entries are (Mt e)_root instead of 0 and are dropped by the second
    call, which moves its result by the Mt-orthogonal projection of e (2-norm at most
    sqrt(cond Mt) |e|_2); tau's own error d (at most its bound b_tau per entry) moves it by
    Mt^-1 d, at most sqrt(nv) b_tau / lambda_min; the second solve adds its own b_fd |acc|."""
    view, m, n, st = case["view"], case["model"], case["n"], case["st"]
    nr, nv = case["r64"].nr, view.num_gen_vel
    eff = np.random.default_rng(3).uniform(-5, 5, size=(n, m.num_dof)).astype(np.float32)
    rc, acc0 = forward(view, MODES[mode], eff)
    assert rc == 0
    rc, got = inverse_dynamics(view, MODES[mode], acc0, wrench=False)
    assert rc == 0
    rc, acc1 = forward(view, MODES[mode], got["tau"][:, nr:])
    assert rc == 0
    args = (m, st, float(view.sim_params.dt), mode)
    ms64 = MassSolve(*args, gravity=sim_gravity(view))
    ms32 = MassSolve(*args, gravity=sim_gravity(view), dtype=np.float32)
    b_fd = bound_of(ms32.forward_dynamics(eff), ms64.forward_dynamics(eff)) * float(np.abs(acc0).max())
    b_tau = check(f"{case['tag']} {mode} tau of the device's acc", got["tau"], case["r32"].tau(acc0, mode),
                  case["r64"].tau(acc0, mode))
    lam = np.linalg.eigvalsh(ms64.Mt)
    cond, lmin = float((lam[:, -1] / lam[:, 0]).max()), float(lam[:, 0].min())
    limit = b_fd * (1.0 + np.sqrt(nv * cond)) + np.sqrt(nv) * b_tau / lmin
    err = float(np.abs(acc1.astype(np.float64) - acc0).max())
    err_tau = float(np.abs(got["tau"][:, nr:].astype(np.float64) - eff).max())
    print(f"{case['tag']} {mode} round trip: |acc1 - acc0| {err:.3e} limit {limit:.3e}; |tau_joint - efforts| {err_tau:.3e}, "
          f"|tau_root| {float(np.abs(got['tau'][:, :nr]).max()) if nr else 0.0:.3e}")
    assert err <= limit


def test_bias_acceleration_is_the_jacobian_rate(case):
    """Loose sanity only (the float64 reference is the check): (J(state moved by h) u - J u) / h with
    float32 Jacobians from the device, h = 1e-3: truncation ~ h |a'|, held to 5 % of the largest
    acceleration, plus the rounding of the two Jacobians, 1 ulp of |J u| each over h, twice over
    (the cart-pole's link origins ride on the cart: its bias is 0 and only this term is left)."""
    view, m, st, n = case["view"], case["model"], case["st"], case["n"]
    links, h = case["links"], 1e-3
    u = Kinematics(m, st["pos"], st["rot"], st["vel"], st["q"], st["qd"]).u(st["vel"], st["qd"])
    rc, bias = link_acc(view, links, None)
    rc0, J0 = link_jac(view, links, None)
    p, r, q = integrate(m, st["pos"], st["rot"], st["vel"], st["q"], st["qd"], h)
    try:
        write_state(view, dict(st, pos=p.astype(np.float32), rot=r.astype(np.float32), q=q.astype(np.float32)))
        rc1, J1 = link_jac(view, links, None)
    finally:
        write_state(view, st)
        torch.cuda.synchronize()
    assert rc == rc0 == rc1 == 0
    fd = np.einsum("nkrc,nc->nkr", J1.astype(np.float64) - J0.astype(np.float64), u) / h
    err, scale = float(np.abs(bias - fd).max()), float(np.abs(fd).max())
    vel = float(np.abs(np.einsum("nkrc,nc->nkr", J0.astype(np.float64), u)).max())
    limit = 0.05 * scale + 4.0 * EPS * vel / h
    print(f"{case['tag']} Jdot u against differenced Jacobians: {err:.3e} of {scale:.3e} (limit {limit:.3e})")
    assert err <= limit


def test_momentum_is_cmm_times_u(case):
    view, st = case["view"], case["st"]
    rc, got = momentum(view)
    assert rc == 0
    u = case["r64"].u
    m64, m32 = case["r64"].momentum(), case["r32"].momentum()
    limit = bound(m32["mom"], m64["mom"]) + view.num_gen_vel * bound(m32["cmm"], m64["cmm"]) * float(np.abs(u).max())
    err = float(np.abs(np.einsum("nrk,nk->nr", got["cmm"].astype(np.float64), u) - got["mom"]).max())
    print(f"{case['tag']} mom - cmm u: {err:.3e} limit {limit:.3e}")
    assert err <= limit


# ---- 4. the stepper ----
@pytest.mark.parametrize("name", ["Ant", "Humanoid"])
def test_consistency_with_the_stepper(gpu, name):
    n = 16
    env, view, g = _free_flight(name, n, seed=5, moving=True)
    m, dt, nr = view.model, float(view.sim_params.dt), 6
    eff = g.uniform(-5, 5, size=(n, m.num_dof)).astype(np.float32)
    view.set_joint_efforts(torch.from_numpy(eff).cuda())
    st0 = read_state(view)
    view.sim_step(1)
    st1 = read_state(view)
    write_state(view, st0)
    assert all(np.array_equal(v, st0[k]) for k, v in read_state(view).items())
    a = (_u(st1) - _u(st0)) / dt
    rc, got = inverse_dynamics(view, MODES["stepper"], a.astype(np.float32), wrench=False)
    assert rc == 0
    kw = dict(gravity=sim_gravity(view), damping=view.get_joint_dampings().cpu().numpy(),
              armature=view.get_armatures().cpu().numpy())
    r64 = InverseDynamics(m, st0, dt, **kw)
    _, _, bd = refs_and_bounds(m, st0, sim_gravity(view))
    want = np.concatenate([np.zeros((n, nr)), eff.astype(np.float64)], axis=1)
    rest = want - r64.dyn.c - r64.dyn.g
    rest[:, nr:] -= r64.damp * r64.u[:, nr:]
    scale, ud = float(np.abs(rest).max()), float(np.abs(a).max())
    r_ref = float(np.abs(r64.tau(a, "stepper") - want).max())
    r_dev = float(np.abs(got["tau"].astype(np.float64) - want).max())
    limit = 2.0 * r_ref + bd["M"] * ud
    print(f"{name} stepper: inverse-dynamics residual float64 terms {r_ref:.3e}, device {r_dev:.3e} (limit {limit:.3e}); "
          f"|tau - c - g| {scale:.3e}, |du/dt| {ud:.3e}")
    assert r_ref < 1e-3 * scale, "a limit or contact row fired: choose another state"
    assert r_dev <= limit
    env.close()


# ---- 5. per-env parameters ----
@pytest.mark.parametrize("name", ["Cartpole", "Ant", "Humanoid"])
def test_per_env_parameters(gpu, name):
    n = 66
    env = make_env(name, num_envs=n, device="cuda:0", seed=11)
    env.reset()
    view = env.task.get_robot()
    m = view.model
    write_state(view, random_state(m, n, view.env_origins, seed=17))
    st = read_state(view)
    acc = np.random.default_rng(21).uniform(-10, 10, size=(n, view.num_gen_vel)).astype(np.float32)
    c = dict(links=list(range(m.num_links)), offs=offsets_of(m.num_links))
    first = _all_outputs(view, c, acc)
    idx = np.arange(0, n, 3)
    g = np.random.default_rng(9)
    ti = torch.from_numpy(idx).cuda()
    view.set_env_gravity(torch.from_numpy(g.uniform(-12, 12, size=(len(idx), 3)).astype(np.float32)).cuda(), indices=ti)
    damp = (view.get_joint_dampings().cpu().numpy()[idx] * g.uniform(0.5, 2, size=(len(idx), m.num_dof))
            + g.uniform(0.1, 1, size=(len(idx), m.num_dof))).astype(np.float32)
    view.set_joint_dampings(torch.from_numpy(damp).cuda(), indices=ti)
    if name != "Cartpole":         # the analytic cart-pole has no armature
        arm = (view.get_armatures().cpu().numpy()[idx] * g.uniform(0.5, 2, size=(len(idx), m.num_dof))
               + g.uniform(0.01, 0.05, size=(len(idx), m.num_dof))).astype(np.float32)
        view.set_armatures(torch.from_numpy(arm).cuda(), indices=ti)
    got = _all_outputs(view, c, acc)
    changed = np.zeros(n, bool)
    changed[idx] = True
    for k in first:
        moved = np.array([not np.array_equal(got[k][e], first[k][e]) for e in range(n)])
        if k in ("com", "mom", "cmm", "lacc"):
            assert not moved.any(), k
        elif k == "energy":
            assert np.array_equal(got[k][:, 0], first[k][:, 0])
            assert np.array_equal(got[k][:, 1] != first[k][:, 1], changed)
        else:                       # tau of every mode and the wrench follow gravity
            assert np.array_equal(moved, changed), (k, np.flatnonzero(moved != changed))
    kw = dict(gravity=view.get_env_gravity().cpu().numpy(), damping=view.get_joint_dampings().cpu().numpy(),
              armature=None if name == "Cartpole" else view.get_armatures().cpu().numpy())
    r64, r32 = refs(view, st, **kw)
    for mode in MODES:
        check(f"{name} per-env table tau {mode}", got[f"tau_{mode}"], r32.tau(acc, mode), r64.tau(acc, mode))
    check(f"{name} per-env table potential energy", got["energy"][:, 1], r32.momentum()["energy"][:, 1],
          r64.momentum()["energy"][:, 1])
    torch.cuda.synchronize()
    view.clear_env_params()
    back = _all_outputs(view, c, acc)
    for k in first:
        assert np.array_equal(back[k], first[k]), k
    env.close()


# ---- 6. errors ----
def test_errors(case):
    view, L, lib = case["view"], case["model"].num_links, N.lib()
    n, nv = case["n"], view.num_gen_vel
    rc, none = inverse_dynamics(view, 2, None, tau=False, wrench=False)
    assert rc == E_NULL and none == {} and b"both null" in lib.mi_last_error()
    rc, none = momentum(view, com=False, mom=False, cmm=False, energy=False)
    assert rc == E_NULL and none == {} and b"all null" in lib.mi_last_error()
    assert link_acc(view, [0], None, out=False)[0] == E_NULL
    for which in (3, -1):
        assert inverse_dynamics(view, which)[0] == E_ARG
    buf = torch.zeros((n, nv), device="cuda:0")
    assert lib.mi_solve_mass(view.handle, N.MI_MASS_RIGID, buf.data_ptr(), 1, buf.data_ptr(), view.stream()) == E_ARG
    assert lib.mi_get_forward_dynamics(view.handle, N.MI_MASS_RIGID, None, buf.data_ptr(), view.stream()) == E_ARG
    assert link_acc(view, [0], None, K=0)[0] == E_SHAPE
    assert link_acc(view, [0] * (L + 1), None)[0] == E_SHAPE
    assert link_acc(view, [L], None)[0] == E_ARG
    assert link_acc(view, [-1], None)[0] == E_ARG
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        view._momentum(False, False, False, False)
    torch.cuda.synchronize()
