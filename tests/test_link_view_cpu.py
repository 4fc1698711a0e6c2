"""Link-frame view, the parts that need no GPU: the model's body tables, the numpy reference's
own consistency (tests/link_ref.py) and the binding of the two entry points."""
import ctypes as C
import re
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.robots.model import asset_path, load_robot, quat_to_mat
from tests.link_ref import Kinematics, integrate, random_state

ROBOTS = {"Humanoid": "humanoid.xml", "Ant": "ant.xml", "Cartpole": "cartpole.xml"}


def _mjcf_body_origins(path):
    """name -> origin of every <body> at q = 0 with the root at the identity: pos / quat composed
    down the tree straight from the file (the root body's own pos is the spawn pose, not kinematics)."""
    root = ET.parse(path).getroot().find("worldbody").find("body")
    out = {}

    def walk(el, R, p, top):
        if not top:
            pos = np.array([float(t) for t in el.get("pos", "0 0 0").split()])
            q = np.array([float(t) for t in el.get("quat", "1 0 0 0").split()])
            p, R = p + R @ pos, R @ quat_to_mat(q / np.linalg.norm(q))
        out[el.get("name")] = p
        for ch in el.findall("body"):
            walk(ch, R, p, False)

    walk(root, np.eye(3), np.zeros(3), True)
    return out


@pytest.mark.parametrize("name", list(ROBOTS))
def test_body_tables(name):
    m = load_robot(name)
    B = m.num_bodies
    assert B == len(m.body_names) == m.body_link.shape[0] == m.body_offset.shape[0]
    assert m.body_offset.shape == (B, 3)
    assert len(set(m.body_names)) == B and m.body_names[0] == m.body_of_link[0] and m.body_link[0] == 0
    # body b rides on the LAST link of its chain
    for b, (bn, l) in enumerate(zip(m.body_names, m.body_link)):
        assert m.body_of_link[l] == bn
        assert l == max(i for i, x in enumerate(m.body_of_link) if x == bn)
        assert m.get_body_index(bn) == b
    for sl in m.sensor_link:
        assert sl in m.body_link
    # q = 0, identity root: every body origin is the file's pos / quat composition
    n = 1
    z = np.zeros((n, m.num_dof))
    kin = Kinematics(m, np.zeros((n, 3)), np.array([[1.0, 0, 0, 0]]), np.zeros((n, 6)), z, z)
    pos, _, _ = kin.frames(list(m.body_link), m.body_offset)
    want = _mjcf_body_origins(asset_path(ROBOTS[name]))
    for b, bn in enumerate(m.body_names):
        np.testing.assert_allclose(pos[0, b], want[bn], rtol=0, atol=1e-12, err_msg=bn)
    gone = sorted(set(want) - set(m.body_names))
    for bn in gone + ["no_such_body"]:
        with pytest.raises(KeyError) as ei:
            m.get_body_index(bn)
        assert m.body_names[-1] in str(ei.value)       # names the bodies that remain
    if name == "Humanoid":
        assert gone == ["head", "left_hand", "right_hand"]


@pytest.mark.parametrize("name", list(ROBOTS))
def test_reference_is_self_consistent(name):
    """The reference's velocity is the central finite difference of its pose along u, and its
    Jacobian times u is its velocity (float64)."""
    m = load_robot(name)
    n, L = 5, m.num_links
    st = {k: v.astype(np.float64) for k, v in random_state(m, n, np.zeros((n, 3)), seed=3).items()}
    st["rot"] /= np.linalg.norm(st["rot"], axis=1, keepdims=True)   # unit in float64, not just in float32
    g = np.random.default_rng(4)
    links = list(range(L))
    offs = g.uniform(-0.3, 0.3, size=(L, 3))
    kin = Kinematics(m, st["pos"], st["rot"], st["vel"], st["q"], st["qd"])
    pos, quat, vel = kin.frames(links, offs)
    J = kin.jacobians(links, offs)
    assert J.shape == (n, L, 6, kin.nv) and kin.nv == m.num_dof + (6 if m.root_free else 0)
    np.testing.assert_allclose(np.einsum("nkrc,nc->nkr", J, kin.u(st["vel"], st["qd"])), vel, rtol=0, atol=1e-12)
    for k, l in enumerate(links):
        assert np.all(J[:, k][:, :, ~kin.ancestor_columns(l)] == 0.0)
    h = 1e-6
    side = []
    for sgn in (+1, -1):
        p, r, q = integrate(m, st["pos"], st["rot"], st["vel"], st["q"], st["qd"], sgn * h)
        side.append(Kinematics(m, p, r, st["vel"], q, st["qd"]))
    pp, _, _ = side[0].frames(links, offs)
    pm, _, _ = side[1].frames(links, offs)
    np.testing.assert_allclose((pp - pm) / (2 * h), vel[..., :3], rtol=0, atol=2e-8)
    for k, l in enumerate(links):
        S = side[0].R[l] @ np.swapaxes(side[1].R[l], 1, 2)       # ~ I + 2 h [w]x
        W = (S - np.swapaxes(S, 1, 2)) / (4 * h)
        w = np.stack([W[:, 2, 1], W[:, 0, 2], W[:, 1, 0]], axis=1)
        np.testing.assert_allclose(w, vel[:, k, 3:], rtol=0, atol=2e-8)
        # the quaternion and the rotation matrix describe one orientation
        np.testing.assert_allclose(np.stack([quat_to_mat(x) for x in quat[:, k]]), kin.R[l], rtol=0, atol=1e-12)


def test_reference_runs_in_float32():
    m = load_robot("Ant")
    st = random_state(m, 4, np.zeros((4, 3)), seed=1)
    k32 = Kinematics(m, st["pos"], st["rot"], st["vel"], st["q"], st["qd"], dtype=np.float32)
    k64 = Kinematics(m, st["pos"], st["rot"], st["vel"], st["q"], st["qd"])
    links = list(range(m.num_links))
    for a, b in zip(k32.frames(links) + (k32.jacobians(links),), k64.frames(links) + (k64.jacobians(links),)):
        assert a.dtype == np.float32 and b.dtype == np.float64
        assert 0 < np.abs(a - b).max() < 1e-4


def test_native_binds_the_link_entry_points():
    """native.py declares mi_get_link_state / mi_get_link_jacobian with the header's signatures."""
    p, i32p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    want = {"mi_get_link_state": [p, i32p, f32p, C.c_int32, p, p, p, p],
            "mi_get_link_jacobian": [p, i32p, f32p, C.c_int32, p, p]}
    hdr = open(asset_path("../../../include/mi_sim.h")).read()
    for name, args in want.items():
        assert name in N.EXPORTED_SYMBOLS
        res, got = N._SIGS[name]
        assert res is C.c_int and got == args
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr)
        assert decl, name
        # one parameter per comma of the declaration (comments hold none)
        params = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")
        assert len(params) == len(args), (name, params)
    assert re.search(r"#define MI_ABI_VERSION 4\b", hdr)
