"""A robot whose joint tables hold what the packaged robots' do not, and float64 restatements of the kinematics and dynamics
kernels on it (TEST INFRASTRUCTURE ONLY: no GPU, no reference; plain numpy built from the MODEL'S TABLES, not from the URDF).

The packaged robots have multipliers of +-1 only, no bias, no mimic joint and no prismatic joint behind a revolute one, so the
lines of the kernels that read those never ran in the suite.  The zoo (10 links, 6 dofs, 4 tool frames, 18 spheres):

    link  joint  type / axis                  what it contributes
    base  -      fixed                        mass 2.0, the root
    l1    j1     revolute   0  0  1           Z_ROT; every joint origin (this one too) has a non-zero rpy
    l2    j2     prismatic  1  0  0           X_PRISM behind a rotation, in the middle of the chain: a rotated parent frame
    l3    j3     revolute   0 -1  0           Y_ROT, negative axis: multiplier -1
    l3f   jf     fixed, rotated               no <inertial>: the loader's default mass
    l4    j4     prismatic  0  0 -1           Z_PRISM, negative axis; revolute links before (l1, l3) and after (l5, l6) it
    l5    j5     revolute   1  0  0           X_ROT; tool frame
    l6    j6     revolute   0  0  1           mimic of j1, multiplier 0.5, offset 0.3: a second link on dof 0, a multiplier
                                              outside {+-1}, a bias; tool frame
    fa    ja     prismatic  0  1  0           Y_PRISM; tool frame, child of l6
    fb    jb     prismatic  0  1  0           mimic of ja, multiplier -1.5, offset 0.01; tool frame, sibling of fa: the tree
                                              branches and a second prismatic link adds into dof 5

The kernel contract restated here is ``angle = multiplier * q + bias`` about the POSITIVE axis (include/curobo_hip.h); what a
negative axis means for a mimic offset in URDF terms is the loader's business.  ``model()`` asserts the properties of the
table above on the loaded tables, so that a later edit cannot quietly remove them, and replaces the loader's isotropic default
inertias by anisotropic ones with off-diagonal terms (layout ``[ixx iyy izz ixy ixz iyz]`` at the centre of mass).
"""

import dataclasses
import functools
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ZOO_URDF = """<?xml version="1.0"?>
<robot name="joint_zoo">
  <link name="base"><inertial><origin xyz="0.01 -0.02 0.03" rpy="0 0 0"/><mass value="2.0"/></inertial></link>
  <link name="l1"><inertial><origin xyz="0.02 0.01 0.05" rpy="0 0 0"/><mass value="1.4"/></inertial></link>
  <link name="l2"><inertial><origin xyz="0.06 -0.01 0.02" rpy="0 0 0"/><mass value="1.1"/></inertial></link>
  <link name="l3"><inertial><origin xyz="-0.01 0.03 0.07" rpy="0 0 0"/><mass value="0.9"/></inertial></link>
  <link name="l3f"/>
  <link name="l4"><inertial><origin xyz="0.02 0.02 -0.04" rpy="0 0 0"/><mass value="0.7"/></inertial></link>
  <link name="l5"><inertial><origin xyz="0.04 -0.02 0.01" rpy="0 0 0"/><mass value="0.6"/></inertial></link>
  <link name="l6"><inertial><origin xyz="-0.02 0.01 0.03" rpy="0 0 0"/><mass value="0.5"/></inertial></link>
  <link name="fa"><inertial><origin xyz="0.01 0.02 0.01" rpy="0 0 0"/><mass value="0.2"/></inertial></link>
  <link name="fb"><inertial><origin xyz="-0.01 -0.02 0.01" rpy="0 0 0"/><mass value="0.25"/></inertial></link>
  <joint name="j1" type="revolute"><parent link="base"/><child link="l1"/><origin xyz="0.0 0.0 0.12" rpy="0.1 -0.05 0.2"/>
    <axis xyz="0 0 1"/><limit lower="-2.2" upper="2.0" velocity="2.0" effort="80.0"/></joint>
  <joint name="j2" type="prismatic"><parent link="l1"/><child link="l2"/><origin xyz="0.05 0.02 0.15" rpy="-0.3 0.4 0.15"/>
    <axis xyz="1 0 0"/><limit lower="-0.1" upper="0.35" velocity="0.5" effort="60.0"/></joint>
  <joint name="j3" type="revolute"><parent link="l2"/><child link="l3"/><origin xyz="0.2 -0.03 0.04" rpy="0.25 0.1 -0.35"/>
    <axis xyz="0 -1 0"/><limit lower="-1.8" upper="1.9" velocity="2.0" effort="60.0"/></joint>
  <joint name="jf" type="fixed"><parent link="l3"/><child link="l3f"/><origin xyz="0.03 0.04 0.18" rpy="0.5 -0.2 0.7"/></joint>
  <joint name="j4" type="prismatic"><parent link="l3f"/><child link="l4"/><origin xyz="-0.02 0.05 0.06" rpy="-0.15 0.3 0.1"/>
    <axis xyz="0 0 -1"/><limit lower="-0.2" upper="0.15" velocity="0.5" effort="40.0"/></joint>
  <joint name="j5" type="revolute"><parent link="l4"/><child link="l5"/><origin xyz="0.04 0.0 -0.1" rpy="0.2 0.35 -0.25"/>
    <axis xyz="1 0 0"/><limit lower="-2.4" upper="2.1" velocity="2.5" effort="30.0"/></joint>
  <joint name="j6" type="revolute"><parent link="l5"/><child link="l6"/><origin xyz="0.12 0.02 0.03" rpy="-0.4 0.15 0.3"/>
    <axis xyz="0 0 1"/><limit lower="-3.0" upper="3.0" velocity="2.5" effort="20.0"/><mimic joint="j1" multiplier="0.5" offset="0.3"/></joint>
  <joint name="ja" type="prismatic"><parent link="l6"/><child link="fa"/><origin xyz="0.02 0.03 0.08" rpy="0.1 0.2 -0.1"/>
    <axis xyz="0 1 0"/><limit lower="0.0" upper="0.06" velocity="0.2" effort="20.0"/></joint>
  <joint name="jb" type="prismatic"><parent link="l6"/><child link="fb"/><origin xyz="0.02 -0.03 0.08" rpy="-0.1 0.25 0.05"/>
    <axis xyz="0 1 0"/><limit lower="-0.1" upper="0.1" velocity="0.2" effort="20.0"/><mimic joint="ja" multiplier="-1.5" offset="0.01"/></joint>
</robot>
"""
#: two spheres on every link that carries a mass of its own; one of l5's is disabled
ZOO_SPHERES = {
    "base": [{"center": [0.0, 0.0, 0.05], "radius": 0.07}, {"center": [0.03, -0.02, 0.0], "radius": 0.05}],
    "l1": [{"center": [0.0, 0.01, 0.06], "radius": 0.05}, {"center": [0.04, 0.0, 0.12], "radius": 0.04}],
    "l2": [{"center": [0.05, 0.0, 0.01], "radius": 0.045}, {"center": [0.14, -0.02, 0.03], "radius": 0.04}],
    "l3": [{"center": [0.0, 0.02, 0.05], "radius": 0.04}, {"center": [0.02, 0.03, 0.13], "radius": 0.035}],
    "l4": [{"center": [0.0, 0.0, -0.03], "radius": 0.035}, {"center": [0.03, 0.01, -0.08], "radius": 0.03}],
    "l5": [{"center": [0.04, 0.0, 0.0], "radius": 0.035}, {"center": [0.09, 0.01, 0.02], "radius": -100.0}],
    "l6": [{"center": [0.0, 0.0, 0.03], "radius": 0.03}, {"center": [0.01, 0.0, 0.07], "radius": 0.025}],
    "fa": [{"center": [0.0, 0.01, 0.02], "radius": 0.015}, {"center": [0.0, 0.01, 0.05], "radius": 0.012}],
    "fb": [{"center": [0.0, -0.01, 0.02], "radius": 0.015}, {"center": [0.0, -0.01, 0.05], "radius": 0.012}],
}
TOOL_FRAMES = ["fa", "l5", "l6", "fb"]  # the first names the main chain; the loader orders them l5, l6, fa, fb
GRAVITY = 9.81


def _inertias(masses):
    """[L, 8] float32: per link a positive-definite, anisotropic inertia with off-diagonal terms, scaled by the link's mass"""
    rng = np.random.default_rng(21)
    out = np.zeros((len(masses), 8), np.float32)
    for i, m in enumerate(masses):
        a = rng.normal(size=(3, 3))
        inertia = 0.02 * m * (a @ a.T + 0.5 * np.eye(3))
        out[i, :6] = [inertia[0, 0], inertia[1, 1], inertia[2, 2], inertia[0, 1], inertia[0, 2], inertia[1, 2]]
    return out


@functools.lru_cache(maxsize=None)
def model():
    from curobo_amd.robot import build_robot_model
    from curobo_amd.robot.builder import RobotBuilder
    from curobo_amd.robot.loader import FIXED, X_PRISM, X_ROT, Z_PRISM
    from curobo_amd.robot.urdf import load_urdf

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "joint_zoo.urdf")
        with open(path, "w") as fh:
            fh.write(ZOO_URDF)
        b = RobotBuilder(path, tool_frames=TOOL_FRAMES, device="cpu")
        b.set_collision_spheres(ZOO_SPHERES)
        cfg = b.build()
        m = build_robot_model(cfg, load_urdf(path))
    m = dataclasses.replace(m, link_inertias=_inertias(m.link_masses_com[:, 3]))
    # ---- the properties this robot exists for
    jt, jm = m.joint_map_type.astype(int), m.joint_map.astype(int)
    off = m.joint_offset_map.reshape(-1, 2)
    moving = jt != FIXED
    assert m.num_dof <= 16 and len(m.tool_frame_map) >= 2
    assert set(jt[moving]) == set(range(X_PRISM, X_ROT + 3)), "all six joint types"
    assert (off[moving, 1] != 0).any(), "a bias"
    assert (~np.isin(off[moving, 0], (-1.0, 1.0))).any(), "a multiplier outside {+-1}"
    assert (np.diff(m.joint_links_offsets) == 2).any(), "a dof with two links"
    sandwiched = False
    for t in m.tool_frame_map:
        chain = [int(k) for k in m.link_chain_data[m.link_chain_offsets[t]:m.link_chain_offsets[t + 1]]]
        kinds = [jt[k] for k in chain if jt[k] != FIXED]
        for i, k in enumerate(kinds):
            if k <= Z_PRISM and any(x >= X_ROT for x in kinds[:i]) and any(x >= X_ROT for x in kinds[i + 1:]):
                sandwiched = True
    assert sandwiched, "a prismatic link with a revolute link before and after it on a tool chain"
    assert (m.link_spheres[0, :, 3] < 0).sum() == 1 and m.num_spheres == 18
    iner = m.link_inertias
    for i in range(m.num_links):
        full = np.array([[iner[i, 0], iner[i, 3], iner[i, 4]], [iner[i, 3], iner[i, 1], iner[i, 5]], [iner[i, 4], iner[i, 5], iner[i, 2]]])
        assert np.linalg.eigvalsh(full).min() > 0 and np.abs(iner[i, 3:6]).min() > 0
    return m


def mimic_free_frames(m):
    """indices t of the tool frames whose chain holds no mimic link (a link that is not the first of its dof)"""
    off = m.joint_links_offsets.astype(int)
    followers = {int(k) for j in range(m.num_dof) for k in m.joint_links_data[off[j] + 1:off[j + 1]]}
    return [t for t, link in enumerate(m.tool_frame_map.astype(int)) if not (set(_chain(m, link)) & followers)]


def revolute_dofs(m):
    """[D] float32: 1 for a dof whose links are all revolute, 0 for a prismatic one"""
    return np.array([float(all(m.joint_map_type[k] >= 3 for k in np.nonzero(m.joint_map == j)[0])) for j in range(m.num_dof)], np.float32)


# ------------------------------------------------------------------------------------------------ forward, float64
def _chain(m, link):
    return [int(k) for k in m.link_chain_data[m.link_chain_offsets[link]:m.link_chain_offsets[link + 1]]]


def _joint_matrix(jt, angle):
    """[n, 4, 4]: translation along / rotation about the positive axis"""
    J = np.broadcast_to(np.eye(4), (len(angle), 4, 4)).copy()
    if jt < 0:
        return J
    if jt <= 2:
        J[:, jt, 3] = angle
        return J
    a = jt - 3
    i, k = (a + 1) % 3, (a + 2) % 3
    c, s = np.cos(angle), np.sin(angle)
    J[:, i, i], J[:, i, k], J[:, k, i], J[:, k, k] = c, -s, s, c
    return J


def fk64(m, q):
    """link transforms [n, L, 4, 4]: cumulative products of ``fixed_transform @ joint(multiplier * q + bias)``"""
    q = np.atleast_2d(np.asarray(q, np.float64))
    n, L = q.shape[0], m.num_links
    off = m.joint_offset_map.reshape(-1, 2).astype(np.float64)
    T = np.zeros((n, L, 4, 4))
    for l in range(L):
        F = np.eye(4)
        F[:3] = m.fixed_transforms[l].astype(np.float64)
        jt, j = int(m.joint_map_type[l]), int(m.joint_map[l])
        angle = off[l, 0] * q[:, j] + off[l, 1] if jt >= 0 else np.zeros(n)
        local = F[None] @ _joint_matrix(jt, angle)
        T[:, l] = local if l == 0 else T[:, int(m.link_map[l])] @ local
    return T


def spheres64(m, T):
    """world spheres [n, S, 4]; the radius (a disabled one too) is the table's"""
    s = m.link_spheres[0].astype(np.float64)
    Tl = T[:, m.link_sphere_idx_map.astype(int)]
    out = np.empty((T.shape[0], s.shape[0], 4))
    out[..., :3] = np.einsum("nsij,sj->nsi", Tl[..., :3, :3], s[:, :3]) + Tl[..., :3, 3]
    out[..., 3] = s[:, 3]
    return out


def link_com64(m, T):
    """world centres of mass of the links [n, L, 3]"""
    mc = m.link_masses_com.astype(np.float64)
    return np.einsum("nlij,lj->nli", T[..., :3, :3], mc[:, :3]) + T[..., :3, 3]


def com64(m, T):
    """[n, 4]: centre of mass and total mass"""
    mass = m.link_masses_com[:, 3].astype(np.float64)
    c = np.einsum("nli,l->ni", link_com64(m, T), mass) / mass.sum()
    return np.concatenate([c, np.full((T.shape[0], 1), mass.sum())], 1)


def tool_pose64(m, T):
    """(positions [n, T, 3], rotations [n, T, 3, 3]) of the tool frames"""
    Tt = T[:, m.tool_frame_map.astype(int)]
    return Tt[..., :3, 3], Tt[..., :3, :3]


def quat_to_matrix(quat):
    """[..., 4] (w, x, y, z), normalised here -> [..., 3, 3]; R(q) = R(-q): no sign question"""
    q = np.asarray(quat, np.float64)
    w, x, y, z = np.moveaxis(q / np.linalg.norm(q, axis=-1, keepdims=True), -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def matrix_to_quat(R):
    """[..., 3, 3] -> [..., 4] (w, x, y, z) with w >= 0, through the largest of the four squared components"""
    R = np.asarray(R, np.float64)
    m00, m11, m22 = R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]
    sq = np.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1)
    big = np.argmax(sq, -1)
    cand = np.stack([
        np.stack([sq[..., 0], R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1),
        np.stack([R[..., 2, 1] - R[..., 1, 2], sq[..., 1], R[..., 0, 1] + R[..., 1, 0], R[..., 0, 2] + R[..., 2, 0]], -1),
        np.stack([R[..., 0, 2] - R[..., 2, 0], R[..., 0, 1] + R[..., 1, 0], sq[..., 2], R[..., 1, 2] + R[..., 2, 1]], -1),
        np.stack([R[..., 1, 0] - R[..., 0, 1], R[..., 0, 2] + R[..., 2, 0], R[..., 1, 2] + R[..., 2, 1], sq[..., 3]], -1)], -2)
    q = np.take_along_axis(cand, big[..., None, None], -2)[..., 0, :]
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return np.where(q[..., :1] < 0, -q, q)


# ------------------------------------------------------------------------------------------------ Jacobians, float64
def point_jacobian64(m, T, link, point):
    """(Jv [n, 3, D], Jw [n, 3, D]) of the world point ``point`` [n, 3] that rides on ``link``: every moving link k of the
    chain adds ``mul_k * axis_k x (point - p_k)`` / ``mul_k * axis_k`` (revolute) or ``mul_k * axis_k`` linear only
    (prismatic) into column ``joint_map[k]``"""
    n, D = T.shape[0], m.num_dof
    off = m.joint_offset_map.reshape(-1, 2).astype(np.float64)
    Jv, Jw = np.zeros((n, 3, D)), np.zeros((n, 3, D))
    for k in _chain(m, link):
        jt, j = int(m.joint_map_type[k]), int(m.joint_map[k])
        if jt < 0:
            continue
        axis = off[k, 0] * T[:, k, :3, jt % 3]
        if jt >= 3:
            Jv[:, :, j] += np.cross(axis, point - T[:, k, :3, 3])
            Jw[:, :, j] += axis
        else:
            Jv[:, :, j] += axis
    return Jv, Jw


def jacobian64(m, q, T=None):
    """tool-frame Jacobians [n, T, 6, D], rows (linear, angular), the columns of a dof's links summed"""
    T = fk64(m, q) if T is None else T
    out = np.zeros((T.shape[0], len(m.tool_frame_map), 6, m.num_dof))
    for t, link in enumerate(m.tool_frame_map.astype(int)):
        out[:, t, :3], out[:, t, 3:] = point_jacobian64(m, T, link, T[:, link, :3, 3])
    return out


def _central(f, q, h):
    """[n, D]: central differences of the per-row scalar ``f(q) -> [n]``"""
    q = np.asarray(q, np.float64)
    out = np.zeros_like(q)
    for j in range(q.shape[1]):
        dq = np.zeros_like(q)
        dq[:, j] = h
        out[:, j] = (f(q + dq) - f(q - dq)) / (2 * h)
    return out


def quat_omega64(quat, g_quat):
    """omega = 1/2 E(q)^T g_quat [n, T, 3], as tests/test_oracle_kinematics.py::test_backward_orientation_term writes it"""
    qw, qx, qy, qz = np.moveaxis(np.asarray(quat, np.float64), -1, 0)
    gw, gx, gy, gz = np.moveaxis(np.asarray(g_quat, np.float64), -1, 0)
    return 0.5 * np.stack([-qx * gw + qw * gx + qz * gy - qy * gz, -qy * gw - qz * gx + qw * gy + qx * gz,
                           -qz * gw + qy * gx - qx * gy + qw * gz], -1)


VJP_H = 1e-6


def vjp64(m, q, g_spheres=None, g_pos=None, g_quat=None, g_com=None, h=VJP_H):
    """d/dq of <g_spheres, spheres> + <g_pos, link_pos> + <g_com, com> by central differences, plus the orientation term
    J_ang^T omega (analytic).  The radius and mass components of the cotangents take no part."""
    q = np.atleast_2d(np.asarray(q, np.float64))

    def scalar(qq):
        T = fk64(m, qq)
        s = np.zeros(qq.shape[0])
        if g_spheres is not None:
            s += (spheres64(m, T)[..., :3] * np.asarray(g_spheres, np.float64)[..., :3]).sum((1, 2))
        if g_pos is not None:
            s += (tool_pose64(m, T)[0] * np.asarray(g_pos, np.float64)).sum((1, 2))
        if g_com is not None:
            s += (com64(m, T)[:, :3] * np.asarray(g_com, np.float64)[:, :3]).sum(1)
        return s

    out = _central(scalar, q, h) if any(g is not None for g in (g_spheres, g_pos, g_com)) else np.zeros_like(q)
    if g_quat is not None:
        T = fk64(m, q)
        om = quat_omega64(matrix_to_quat(tool_pose64(m, T)[1]), g_quat)
        out = out + np.einsum("ntkj,ntk->nj", jacobian64(m, q, T)[:, :, 3:], om)
    return out


JAC_GRAD_H = 1e-6


def jacobian_grad64(m, q, w, h=JAC_GRAD_H):
    """d/dq of <w, J(q)>, w [n, T, 6, D], by central differences of the analytic Jacobian"""
    w = np.asarray(w, np.float64)
    return _central(lambda qq: (jacobian64(m, qq) * w).sum((1, 2, 3)), np.atleast_2d(np.asarray(q, np.float64)), h)


def column_cotangents(w):
    """[D, n, T, 6, D]: ``w`` with everything but the column of dof k zeroed, for every k"""
    w = np.asarray(w)
    out = np.zeros((w.shape[-1],) + w.shape, w.dtype)
    for k in range(w.shape[-1]):
        out[k, ..., k] = w[..., k]
    return out


def jacobian_grad_per_column64(m, q, w):
    """[D (k), n, D (i)]: d/dq_i of <w[..., k], J[..., k]>, the cotangent on the column of dof k alone"""
    return np.stack([jacobian_grad64(m, q, wk) for wk in column_cotangents(w)])


#: (arm of the kernel's dJ/dq, dof k of the Jacobian column, dof i of the derivative): dofs 0, 2, 4 are revolute (0 has the two
#: links l1 and l6), dofs 1, 3, 5 prismatic (5 has fa and fb); along the chain l1 l2 l3 l4 l5 l6 fa|fb
JAC_GRAD_ARMS = (("k revolute, i revolute before k", 4, 2), ("k revolute, i revolute at or after k", 2, 4),
                 ("k revolute, i prismatic after k", 2, 3), ("k prismatic, i revolute before k", 3, 2),
                 ("k prismatic with two links, i revolute with two links", 5, 0), ("k revolute with two links, i prismatic between them", 0, 3))
JAC_GRAD_ZERO = (("k revolute, i prismatic before k", 4, 1), ("k prismatic, i prismatic", 3, 1), ("k prismatic, i revolute after k", 1, 4))


# ------------------------------------------------------------------------------------------------ dynamics, float64
def _inertia_matrices(m):
    i = m.link_inertias.astype(np.float64)
    return np.stack([np.stack([i[:, 0], i[:, 3], i[:, 4]], -1), np.stack([i[:, 3], i[:, 1], i[:, 5]], -1),
                     np.stack([i[:, 4], i[:, 5], i[:, 2]], -1)], -2)


def mass_matrix64(m, q):
    """M(q) [n, D, D] = sum_l m_l Jv_l^T Jv_l + Jw_l^T R_l I_l R_l^T Jw_l from the analytic Jacobians of the links' centres
    of mass; also the potential energy U(q) [n] = 9.81 sum_l m_l z_l and its gradient [n, D]"""
    q = np.atleast_2d(np.asarray(q, np.float64))
    T = fk64(m, q)
    coms, mass, I = link_com64(m, T), m.link_masses_com[:, 3].astype(np.float64), _inertia_matrices(m)
    M, dU = np.zeros((q.shape[0], m.num_dof, m.num_dof)), np.zeros_like(q)
    for l in range(m.num_links):
        Jv, Jw = point_jacobian64(m, T, l, coms[:, l])
        R = T[:, l, :3, :3]
        Iw = R @ I[l][None] @ np.swapaxes(R, 1, 2)
        M += mass[l] * np.einsum("nki,nkj->nij", Jv, Jv) + np.einsum("nki,nkl,nlj->nij", Jw, Iw, Jw)
        dU += GRAVITY * mass[l] * Jv[:, 2]
    return M, GRAVITY * (coms[..., 2] * mass).sum(1), dU


TAU_H = 1e-4


def tau64(m, q, qd, qdd, h=TAU_H, parts=False):
    """inverse dynamics from the Lagrangian: M(q) qdd + Mdot qd - 1/2 grad(qd^T M qd) + grad U, Mdot qd and the gradient of the
    kinetic energy by central differences of M with step ``h``.  ``parts``: (M qdd, Coriolis, gravity) instead of the sum."""
    q, qd, qdd = (np.atleast_2d(np.asarray(x, np.float64)) for x in (q, qd, qdd))
    M, _, dU = mass_matrix64(m, q)
    Mdot = (mass_matrix64(m, q + h * qd)[0] - mass_matrix64(m, q - h * qd)[0]) / (2 * h)
    dT = _central(lambda qq: np.einsum("ni,nij,nj->n", qd, mass_matrix64(m, qq)[0], qd), q, h)
    inertial = np.einsum("nij,nj->ni", M, qdd)
    coriolis = np.einsum("nij,nj->ni", Mdot, qd) - 0.5 * dT
    return (inertial, coriolis, dU) if parts else inertial + coriolis + dU


RNEA_VJP_H = 1e-4


def rnea_vjp64(m, q, qd, qdd, w, h=RNEA_VJP_H, tau_h=TAU_H):
    """(d/dq, d/dqd, d/dqdd) of <w, tau64(q, qd, qdd)> by central differences"""
    q, qd, qdd, w = (np.atleast_2d(np.asarray(x, np.float64)) for x in (q, qd, qdd, w))
    f = lambda a, b, c: (tau64(m, a, b, c, tau_h) * w).sum(1)  # noqa: E731
    return (_central(lambda x: f(x, qd, qdd), q, h), _central(lambda x: f(q, x, qdd), qd, h),
            _central(lambda x: f(q, qd, x), qdd, h))


# ------------------------------------------------------------------------------------------------ shared inputs
N = 65
BATCHES = (1, 17, 65)  # one point; a ragged last 16-lane row group; one point past a 64-point workgroup
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "joint_zoo.npz")


def make_inputs(seed=5):
    """the inputs of the golden (tests/golden/make_joint_zoo_golden.py): q inside the joint limits, cotangents, qd, qdd, f_ext"""
    from conftest import sample_q

    m = model()
    rng = np.random.default_rng(seed)
    S, T, D, L = m.num_spheres, len(m.tool_frame_map), m.num_dof, m.num_links
    f = lambda *s: rng.normal(size=s).astype(np.float32)  # noqa: E731
    g_s, g_b = f(N, S, 4), f(N, S, 4)
    g_s[rng.uniform(size=(N, S)) < 0.4] = 0.0  # sparse, like collision gradients
    g_b[rng.uniform(size=(N, S)) < 0.6] = 0.0
    return dict(q=sample_q(m, N, seed=seed), g_spheres=g_s, g_spheres_b=g_b, g_pos=f(N, T, 3), g_quat=f(N, T, 4), g_com=f(N, 4),
                w_jac=f(N, T, 6, D), qd=f(N, D), qdd=(2 * f(N, D)), w_tau=f(N, D), f_ext=f(N, L, 6))


@functools.lru_cache(maxsize=None)
def golden():
    g = dict(np.load(GOLDEN))
    for v in g.values():
        v.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def expected():
    """the float64 side of every comparison on the golden's inputs (computed once, shared, never modified) and ``g``: the
    largest gap between the reference's fp32 result in the golden and float64, per quantity, pooled over the 65 points.
    Gradients and torques: relative to the largest float64 entry.  Where the reference is known to be wrong, ``g`` is taken
    where it is right: dJ/dq on the tool frames without a mimic link, RNEA with no velocity on the prismatic dofs."""
    m, z = model(), golden()
    q = z["q"]
    T = fk64(m, q)
    pos, rot = tool_pose64(m, T)
    e = dict(T=T, pos=pos, rot=rot, spheres=spheres64(m, T), com=com64(m, T), jacobian=jacobian64(m, q, T))
    e["vjp"] = vjp64(m, q, z["g_spheres"], z["g_pos"], z["g_quat"], z["g_com"])
    e["jac_grad"] = jacobian_grad64(m, q, z["w_jac"])
    e["tau"] = tau64(m, q, z["qd"], z["qdd"])
    e["rnea_vjp"] = rnea_vjp64(m, q, z["qd"], z["qdd"], z["w_tau"])
    e["tau_revolute"] = tau64(m, q, z["qd_revolute_only"], z["qdd"])
    e["rnea_vjp_revolute"] = rnea_vjp64(m, q, z["qd_revolute_only"], z["qdd"], z["w_tau"])
    free = mimic_free_frames(m)
    w_free = np.zeros_like(z["w_jac"])
    w_free[:, free] = z["w_jac"][:, free]
    e["jac_grad_free"] = jacobian_grad64(m, q, w_free)
    gap = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max())  # noqa: E731
    rel = lambda a, b: gap(a, b) / float(np.abs(b).max())  # noqa: E731
    g = dict(pos=gap(z["ref/link_pos"], pos), rot=gap(quat_to_matrix(z["ref/link_quat"]), rot),
             cumul=gap(z["ref/cumul_mat"], T[:, :, :3]), spheres=gap(z["ref/robot_spheres"], e["spheres"]),
             com=gap(z["ref/com"], e["com"]), jacobian=gap(z["ref/jacobian"], e["jacobian"]), vjp=rel(z["ref/vjp"], e["vjp"]),
             jac_grad=rel(z["ref/jac_grad_mimic_free_frames"], e["jac_grad_free"]),
             tau=rel(z["ref/tau_revolute_velocity_only"], e["tau_revolute"]))
    for i, k in enumerate(("q", "qd", "qdd")):
        g[f"rnea_grad_{k}"] = rel(z[f"ref/rnea_grad_{k}_revolute_velocity_only"], e["rnea_vjp_revolute"][i])
    for v in e.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    e["g"] = g
    return e


# ------------------------------------------------------------------------------------------------ the comparison
def gap(a, b, relative=False):
    b = np.asarray(b, np.float64)
    d = float(np.abs(np.asarray(a, np.float64) - b).max())
    return d / float(np.abs(b).max()) if relative else d


def held(name, got, want, g, relative=False, factor=4.0):
    e = gap(got, want, relative)
    print(f"[joint zoo] {name}: g {g:.2e}, gap {e:.2e}{' of the largest entry' if relative else ''}")
    assert e <= factor * g, f"{name}: gap {e:.3e} > {factor} g = {factor * g:.3e}"
