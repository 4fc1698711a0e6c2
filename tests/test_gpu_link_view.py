"""Link-frame view on the GPU (include/mi_sim.h mi_get_link_state / mi_get_link_jacobian,
robots/articulations.py RigidPrimView) against the numpy reference of tests/link_ref.py.

Tolerance: nothing here is a tuned number. The reference runs twice on the float32 state read
back from the device, in float64 and in float32; the device may be off the float64 run by 4x the
float32 run's worst deviation per output kind (it orders its float32 operations differently from
numpy), floored at 2 ulp of the output's magnitude. Measured (MI355X, N = 257, device error / bound):
Humanoid bodies pos 1.9e-6 / 1.1e-5, quat 3.2e-7 / 1.3e-6, vel 1.7e-6 / 6.7e-6, jac 2.9e-7 / 1.1e-6,
jac @ u - vel 1.1e-6 / 2.9e-5; every case prints its own figures (pytest -s), DESIGN §4 has the table."""
import numpy as np
import pytest
import torch

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.robots.articulations import RigidPrimView
from omniisaacgymenvs_amd.utils.task_util import make_env
from tests.link_ref import Kinematics, random_state

pytestmark = pytest.mark.gpu
CASES = [("Humanoid", 257), ("Ant", 257), ("Cartpole", 257), ("Ant", 1)]
EPS = float(np.finfo(np.float32).eps)


# ---- device calls ----
def link_state(view, links, offs, pos=True, quat=True, vel=True, K=None):
    """mi_get_link_state into fresh buffers -> (rc, dict of numpy arrays); skipped outputs pass NULL."""
    ids = np.ascontiguousarray(links, dtype=np.int32)
    o = None if offs is None else np.ascontiguousarray(offs, dtype=np.float32)
    K = len(ids) if K is None else K
    n = view.count
    t = {k: torch.full((n, max(K, 1), w), np.nan, device="cuda:0") if on else None
         for k, w, on in (("pos", 3, pos), ("quat", 4, quat), ("vel", 6, vel))}
    rc = N.lib().mi_get_link_state(view.handle, N.iptr(ids), N.fptr(o), K, N.ptr(t["pos"]), N.ptr(t["quat"]),
                                   N.ptr(t["vel"]), view.stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in t.items() if v is not None}


def link_jac(view, links, offs, K=None):
    ids = np.ascontiguousarray(links, dtype=np.int32)
    o = None if offs is None else np.ascontiguousarray(offs, dtype=np.float32)
    K = len(ids) if K is None else K
    out = torch.full((view.count, max(K, 1), 6, view.num_gen_vel), np.nan, device="cuda:0")
    rc = N.lib().mi_get_link_jacobian(view.handle, N.iptr(ids), N.fptr(o), K, out.data_ptr(), view.stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def read_state(view):
    """The float32 state through the per-call gathers."""
    lib, n, D = N.lib(), view.count, view.num_dof
    t = {k: torch.empty(s, device="cuda:0") for k, s in
         (("pos", (n, 3)), ("rot", (n, 4)), ("vel", (n, 6)), ("q", (n, D)), ("qd", (n, D)))}
    st = view.stream()
    assert lib.mi_get_root_state(view.handle, t["pos"].data_ptr(), t["rot"].data_ptr(), t["vel"].data_ptr(), st) == 0
    assert lib.mi_get_dof_state(view.handle, t["q"].data_ptr(), t["qd"].data_ptr(), st) == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def write_state(view, st):
    dev = lambda a: torch.from_numpy(a).cuda()
    view.set_world_poses(dev(st["pos"]), dev(st["rot"]))
    if view.model.root_free:            # a fixed base has no root velocity
        view.set_velocities(dev(st["vel"]))
    view.set_joint_positions(dev(st["q"]))
    view.set_joint_velocities(dev(st["qd"]))


# ---- the bound ----
def _align(q, ref):
    """Quaternions up to sign: q with the sign of ref."""
    return q * np.where((q * ref).sum(-1, keepdims=True) < 0, -1.0, 1.0)


def bounds_and_refs(model, st, links, offs):
    """Float64 reference outputs and the bound per output kind: 4 x the float32 run's worst
    deviation from the float64 run, at least 2 ulp of the largest value."""
    k64 = Kinematics(model, st["pos"], st["rot"], st["vel"], st["q"], st["qd"])
    k32 = Kinematics(model, st["pos"], st["rot"], st["vel"], st["q"], st["qd"], dtype=np.float32)
    r64 = dict(zip(("pos", "quat", "vel"), k64.frames(links, offs)), jac=k64.jacobians(links, offs))
    r32 = dict(zip(("pos", "quat", "vel"), k32.frames(links, offs)), jac=k32.jacobians(links, offs))
    r32["quat"] = _align(r32["quat"].astype(np.float64), r64["quat"])
    bound = {k: max(4.0 * float(np.abs(r32[k] - r64[k]).max()), 2.0 * EPS * float(np.abs(r64[k]).max())) for k in r64}
    return k64, r64, bound


def check(tag, got, r64, bound, kinds):
    for k in kinds:
        g = got[k].astype(np.float64)
        if k == "quat":
            g = _align(g, r64[k])
        err = float(np.abs(g - r64[k]).max())
        print(f"{tag} {k}: device error {err:.3e} bound {bound[k]:.3e}")
        assert np.isfinite(g).all(), (tag, k)
        assert err <= bound[k], (tag, k, err, bound[k])


# ---- one env + random state + references per case, shared by the tests below ----
@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def case(request, gpu):
    name, n = request.param
    env = make_env(name, num_envs=n, device="cuda:0", seed=11)
    env.reset()
    view = env.task.get_robot()
    m = view.model
    write_state(view, random_state(m, n, view.env_origins, seed=17))
    st = read_state(view)
    L = m.num_links
    c = dict(name=name, n=n, env=env, view=view, model=m, st=st, links=list(range(L)),
             offs=np.random.default_rng(5).uniform(-0.3, 0.3, size=(L, 3)).astype(np.float32))
    c["bodies"] = bounds_and_refs(m, st, list(m.body_link), m.body_offset.astype(np.float32))
    c["raw"] = bounds_and_refs(m, st, c["links"], c["offs"])
    yield c
    env.close()


def test_parity(case):
    m, view = case["model"], case["view"]
    rc, got = link_state(view, m.body_link, m.body_offset)
    assert rc == 0
    _, r64, bound = case["bodies"]
    check(f"{case['name']}-{case['n']} bodies", got, r64, bound, ("pos", "quat", "vel"))
    rc, got = link_state(view, case["links"], case["offs"])
    assert rc == 0
    _, r64, bound = case["raw"]
    check(f"{case['name']}-{case['n']} links+offsets", got, r64, bound, ("pos", "quat", "vel"))


def test_root_frame_is_the_root_state(case):
    view = case["view"]
    rc, got = link_state(view, [0], None)
    assert rc == 0
    p, r = view.get_world_poses()
    v = view.get_velocities()
    assert np.array_equal(got["pos"][:, 0], p.cpu().numpy())
    assert np.array_equal(got["quat"][:, 0], r.cpu().numpy())
    assert np.array_equal(got["vel"][:, 0], v.cpu().numpy())


def test_selection_and_errors(case):
    view, L = case["view"], case["model"].num_links
    lib = N.lib()
    rc, full = link_state(view, case["links"], case["offs"])
    assert rc == 0
    sel = list(np.random.default_rng(9).permutation(L)[:max(1, L // 2)])
    sel = sel + [sel[0]]                                   # scrambled, one id twice
    if len(sel) > L:
        sel = sel[:L]
    rc, sub = link_state(view, sel, case["offs"][sel])
    assert rc == 0
    for k in full:
        assert np.array_equal(sub[k], full[k][:, sel]), k
    rcj, jfull = link_jac(view, case["links"], case["offs"])
    rcs, jsub = link_jac(view, sel, case["offs"][sel])
    assert rcj == 0 and rcs == 0 and np.array_equal(jsub, jfull[:, sel])
    # NULL outputs are skipped
    rc, only = link_state(view, sel, case["offs"][sel], pos=False, vel=False)
    assert rc == 0 and list(only) == ["quat"] and np.array_equal(only["quat"], sub["quat"])
    rc, none = link_state(view, sel, None, pos=False, quat=False, vel=False)
    assert rc == 0 and none == {}
    # shapes and ids
    MI_E_SHAPE, MI_E_ARG = -2, -5
    for fn in (link_state, link_jac):
        assert fn(view, [0], None, K=0)[0] == MI_E_SHAPE and b"K=0" in lib.mi_last_error()
        assert fn(view, [0] * (L + 1), None)[0] == MI_E_SHAPE and f"K={L + 1}".encode() in lib.mi_last_error()
        assert fn(view, [0, L], None)[0] == MI_E_ARG and f"link_ids[1]={L}".encode() in lib.mi_last_error()
        assert fn(view, [-1], None)[0] == MI_E_ARG and b"link_ids[0]=-1" in lib.mi_last_error()


def test_jacobian(case):
    m, view, st = case["model"], case["view"], case["st"]
    nv = m.num_dof + (6 if m.root_free else 0)
    assert view.num_gen_vel == nv
    for tag, links, offs in (("bodies", list(m.body_link), m.body_offset.astype(np.float32)),
                             ("raw", case["links"], case["offs"])):
        kin, r64, bound = case[tag]
        rc, jac = link_jac(view, links, offs)
        assert rc == 0 and jac.shape == (case["n"], len(links), 6, nv)
        check(f"{case['name']}-{case['n']} {tag}", {"jac": jac}, r64, bound, ("jac",))
        for k, l in enumerate(links):
            dead = ~kin.ancestor_columns(l)
            assert np.all(jac[:, k][:, :, dead] == 0.0) and not np.signbit(jac[:, k][:, :, dead]).any()
        rc, got = link_state(view, links, offs, pos=False, quat=False)
        u = kin.u(st["vel"], st["qd"])
        err = float(np.abs(np.einsum("nkrc,nc->nkr", jac.astype(np.float64), u) - got["vel"]).max())
        print(f"{case['name']}-{case['n']} {tag} jac @ u - vel: {err:.3e} bound {nv * bound['jac']:.3e}")
        assert err <= nv * bound["jac"]
    # the Python surface: all bodies by default, names select
    J = view.get_jacobians()
    assert tuple(J.shape) == (case["n"], m.num_bodies, 6, nv)
    names = [m.body_names[-1], m.body_names[0]]
    assert torch.equal(view.get_jacobians(names), J[:, [m.num_bodies - 1, 0]])


@pytest.mark.parametrize("name", ["Humanoid", "Ant", "Cartpole"])
def test_after_stepping(gpu, name):
    """Three env steps, then two direct substeps left deferred: the link getter issues them
    itself, and its frames are the reference's on the state read back afterwards."""
    n = 257
    env = make_env(name, num_envs=n, device="cuda:0", seed=23)
    env.reset()
    view = env.task.get_robot()
    m = view.model
    g = torch.Generator().manual_seed(4)
    for _ in range(3):
        env.step((torch.rand((n, env.num_actions), generator=g) * 2 - 1).cuda())
    before = read_state(view)
    view.sim_step(2)                                       # deferred
    links, offs = list(m.body_link), m.body_offset.astype(np.float32)
    rc, got = link_state(view, links, offs)                # must flush
    assert rc == 0
    st = read_state(view)
    assert not np.array_equal(st["q"], before["q"])        # the substeps ran
    _, r64, bound = bounds_and_refs(m, st, links, offs)
    check(f"{name} after stepping", got, r64, bound, ("pos", "quat", "vel"))
    # contact geoms never sink deeper than the solver lets them: each ground geom's end points
    # (frames of their own: link + offset) stay above -(contact_offset + radius)
    if m.num_geoms:
        gl = np.concatenate([m.geom_link, m.geom_link])
        gp = np.concatenate([m.geom_p0, m.geom_p1]).astype(np.float32)
        gr = np.concatenate([m.geom_radius, m.geom_radius])
        low = []
        for i in range(0, len(gl), m.num_links):           # at most L frames per call
            rc, pts = link_state(view, gl[i:i + m.num_links], gp[i:i + m.num_links], quat=False, vel=False)
            assert rc == 0
            low.append(pts["pos"][:, :, 2])
        z = np.concatenate(low, axis=1)
        floor = -(float(view.sim_params.contact_offset) + gr)
        print(f"{name}: lowest geom centre {z.min():.4f} m")
        assert np.all(z >= floor[None, :])
        feet = [b for b in m.body_names if b.endswith("foot")]
        assert feet
        fz = view.get_link_view(feet).get_world_poses()[0].view(n, len(feet), 3)[:, :, 2]
        assert float(fz.min()) >= -(float(view.sim_params.contact_offset) + float(m.geom_radius.max()))
    env.close()


def test_capture(case):
    """Both getters captured in one graph (a single stream, no branches); after a state change
    the replay equals an eager call bit for bit."""
    view, m, n = case["view"], case["model"], case["n"]
    links = np.ascontiguousarray(m.body_link, dtype=np.int32)
    offs = np.ascontiguousarray(m.body_offset, dtype=np.float32)
    K, nv = len(links), view.num_gen_vel
    lib = N.lib()
    buf = lambda *s: torch.zeros(s, device="cuda:0")
    pos, quat, vel, jac = buf(n, K, 3), buf(n, K, 4), buf(n, K, 6), buf(n, K, 6, nv)

    def call():
        assert lib.mi_get_link_state(view.handle, N.iptr(links), N.fptr(offs), K, pos.data_ptr(), quat.data_ptr(),
                                     vel.data_ptr(), view.stream()) == 0
        assert lib.mi_get_link_jacobian(view.handle, N.iptr(links), N.fptr(offs), K, jac.data_ptr(),
                                        view.stream()) == 0

    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.current_stream().wait_stream(s)
    try:
        write_state(view, random_state(m, n, view.env_origins, seed=29))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        replayed = [t.cpu().numpy().copy() for t in (pos, quat, vel, jac)]
        for t in (pos, quat, vel, jac):
            t.zero_()
        call()
        torch.cuda.synchronize()
        for a, t in zip(replayed, (pos, quat, vel, jac)):
            assert np.array_equal(a, t.cpu().numpy())
        assert not np.array_equal(replayed[0], case["bodies"][1]["pos"].astype(np.float32))   # the state did change
    finally:
        write_state(view, case["st"])                      # the shared state, for the other tests
        torch.cuda.synchronize()


def test_rigid_prim_view(case):
    view, m, n = case["view"], case["model"], case["n"]
    names = [m.body_names[-1], m.body_names[0], m.body_names[m.num_bodies // 2]]
    K = len(names)
    ids = [m.get_body_index(b) for b in names]
    rc, want = link_state(view, m.body_link[ids], m.body_offset[ids])
    assert rc == 0
    lv = view.get_link_view(names, name="some_bodies")
    assert isinstance(lv, RigidPrimView) and lv.count == n * K and lv.name == "some_bodies"
    p, r = lv.get_world_poses()
    v = lv.get_velocities()
    assert tuple(p.shape) == (n * K, 3) and tuple(r.shape) == (n * K, 4) and tuple(v.shape) == (n * K, 6)
    # env-major prims: .view(N, K, ...) is [env, body]
    assert np.array_equal(p.view(n, K, 3).cpu().numpy(), want["pos"])
    assert np.array_equal(r.view(n, K, 4).cpu().numpy(), want["quat"])
    assert np.array_equal(v.view(n, K, 6).cpu().numpy(), want["vel"])
    idx = torch.tensor([n * K - 1, 0, min(K, n * K - 1), min(K + 1, n * K - 1)], device="cuda:0")
    pi, ri = lv.get_world_poses(indices=idx)
    assert torch.equal(pi, p[idx]) and torch.equal(ri, r[idx]) and torch.equal(lv.get_velocities(indices=idx), v[idx])
    # clone=False hands out the view's own buffer, clone=True a copy
    a, _ = lv.get_world_poses(clone=False)
    b, _ = lv.get_world_poses(clone=False)
    c, _ = lv.get_world_poses()
    assert a.data_ptr() == b.data_ptr() != c.data_ptr() and torch.equal(a, c)
    assert lv.get_velocities(clone=False).data_ptr() == lv.get_velocities(clone=False).data_ptr()
    # the reference's construction: a prim path expression, bound by the articulation
    one = view.get_link_view(RigidPrimView(prim_paths_expr=f"/World/envs/.*/{case['name']}/{names[0]}", name="one"))
    assert one.count == n and one.body_names == [names[0]]
    assert np.array_equal(one.get_world_poses()[0].cpu().numpy(), want["pos"][:, 0])
    with pytest.raises(KeyError):
        view.get_link_view(["no_such_body"])
    assert view.num_bodies == m.num_bodies and view.body_names == m.body_names
    assert view.get_body_index(names[0]) == ids[0]
