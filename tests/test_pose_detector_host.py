"""The mesh-SDF pose detector on the host: both C entry points and the workspace query validate before any launch, the four
names import from curobo_amd.perception and from curobo/perception.py, RobotMesh's members, the articulated entry points and
the missing initial pose raise.  No GPU is needed."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

from curobo_amd import _lib
from curobo_amd.backends import perception as P
from curobo_amd.backends.mesh import Mesh

V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)


def test_symbols_are_declared_and_the_abi_is_unchanged():
    lib = _lib.load()
    for n in ("curobo_hip_pose_sdf_ws_bytes", "curobo_hip_pose_sdf_evaluate", "curobo_hip_pose_lm_step"):
        assert n in _lib.declared_symbols() and n in _lib._signatures() and hasattr(lib, n)
    assert lib.curobo_hip_abi_version() == 7
    assert C.sizeof(P.PoseLMState) == 4 * P.POSE_STATE_WORDS == 4 * 71


def test_workspace_query():
    lib = _lib.load()
    nbytes = C.c_int64(-1)
    out = C.cast(C.pointer(nbytes), C.c_void_p)
    assert lib.curobo_hip_pose_sdf_ws_bytes(0, out) == 1 and b"n_points must be positive" in lib.curobo_hip_last_error()
    assert lib.curobo_hip_pose_sdf_ws_bytes(5, None) == 1 and b"out_bytes" in lib.curobo_hip_last_error()
    for n, rows in ((1, 1), (256, 1), (257, 2), (5003, 20)):
        assert lib.curobo_hip_pose_sdf_ws_bytes(n, out) == 0 and nbytes.value == rows * P.POSE_WS_ROW * 4
        assert P.pose_sdf_ws_bytes(n) == nbytes.value
    with pytest.raises(ValueError, match="positive"):
        P.pose_sdf_ws_bytes(-3)


def test_evaluate_arguments_are_validated_without_a_gpu():
    lib = _lib.load()
    pts, pos, quat, ws = torch.zeros(300, 3), torch.zeros(3), torch.zeros(4), torch.zeros(64)
    tri, box = torch.zeros(4, 12), torch.zeros(2, 8)
    mesh = Mesh(tri.data_ptr(), box.data_ptr(), None, 4, 1, 8, 0)
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(points=p(pts), position=p(pos), quaternion=p(quat), work=p(ws), nbytes=256, m=mesh, n=300, maxd=0.2, thr=0.2, hub=1, delta=0.1):
        return lib.curobo_hip_pose_sdf_evaluate(None, None, None, work, nbytes, points, position, quaternion, None if m is None else C.addressof(m),
                                                maxd, thr, hub, delta, n, None)

    for kw in (dict(points=None), dict(position=None), dict(quaternion=None), dict(work=None)):
        assert call(**kw) == 1 and b"must not be null" in lib.curobo_hip_last_error()
    assert call(n=0) == 1 and b"n_points must be positive" in lib.curobo_hip_last_error()
    assert call(n=-4) == 1
    assert call(m=None) == 1 and b"mesh must not be null" in lib.curobo_hip_last_error()
    assert call(m=Mesh(tri.data_ptr(), None, None, 4, 1, 8, 0)) == 1 and b"no tree" in lib.curobo_hip_last_error()
    assert call(m=Mesh(tri.data_ptr(), box.data_ptr(), None, 4, 0, 8, 0)) == 1 and b"no tree" in lib.curobo_hip_last_error()
    assert call(m=Mesh(tri.data_ptr(), box.data_ptr(), None, 4, 3, 8, 0)) == 1 and b"power of two" in lib.curobo_hip_last_error()
    assert call(m=Mesh(tri.data_ptr(), box.data_ptr(), None, 40, 1, 8, 0)) == 1 and b"do not hold" in lib.curobo_hip_last_error()
    assert call(nbytes=255) == 1 and b"workspace of 255 bytes, 300 points need 256" in lib.curobo_hip_last_error()
    assert call(maxd=0.0) == 1 and b"positive" in lib.curobo_hip_last_error()
    assert call(delta=0.0) == 1 and b"huber_delta" in lib.curobo_hip_last_error()
    with pytest.raises(ValueError, match="workspace of 255 bytes"):
        _lib.check(call(nbytes=255))
    with pytest.raises(ValueError, match=r"points must be \(N, 3\)"):
        P.pose_sdf_evaluate(ws, torch.zeros(5, 2), pos, quat, mesh, 0.2, 0.2, True, 0.1)
    with pytest.raises(ValueError, match=r"out_valid must be a contiguous torch.int32"):
        P.pose_sdf_evaluate(ws, pts, pos, quat, mesh, 0.2, 0.2, True, 0.1, out_valid=torch.zeros(300))
    with pytest.raises(ValueError, match=r"out_gradient must have shape \(300, 3\)"):
        P.pose_sdf_evaluate(ws, pts, pos, quat, mesh, 0.2, 0.2, True, 0.1, out_gradient=torch.zeros(300))


def test_lm_step_arguments_are_validated_without_a_gpu():
    lib = _lib.load()
    state, ws = torch.zeros(P.POSE_STATE_WORDS), torch.zeros(64)
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(s=p(state), work=p(ws), nbytes=256, n=300, mode=1, l0=1e-3, fac=10.0, lmin=1e-7, lmax=1e7):
        return lib.curobo_hip_pose_lm_step(s, work, nbytes, n, mode, l0, fac, lmin, lmax, 0.25, 10, None)

    assert call(s=None) == 1 and b"must not be null" in lib.curobo_hip_last_error()
    assert call(work=None) == 1 and b"must not be null" in lib.curobo_hip_last_error()
    assert call(n=0) == 1 and b"n_points must be positive" in lib.curobo_hip_last_error()
    assert call(mode=2) == 1 and b"mode must be 0 (initial) or 1 (update), got 2" in lib.curobo_hip_last_error()
    assert call(nbytes=128) == 1 and b"workspace of 128 bytes" in lib.curobo_hip_last_error()
    assert call(fac=0.0) == 1 and b"lambda" in lib.curobo_hip_last_error()
    assert call(lmin=1.0, lmax=0.5) == 1 and b"lambda" in lib.curobo_hip_last_error()
    with pytest.raises(ValueError, match="state must hold 71 words"):
        P.pose_lm_step(torch.zeros(10), ws, 300, 1, 1e-3, 10.0, 1e-7, 1e7, 0.25)


def test_names_import_from_the_package_and_the_facade():
    import importlib.util

    from conftest import ROOT

    from curobo_amd import perception as A

    spec = importlib.util.spec_from_file_location("_facade_curobo_perception_pose", os.path.join(ROOT, "curobo/perception.py"))
    per = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(per)
    for n in ("SDFPoseDetector", "SDFDetectorCfg", "DetectionResult", "RobotMesh"):
        assert n in A.__all__ and getattr(per, n) is getattr(A, n)
    assert per.__all__ == ["FilterDepth", "RobotSegmenter"]  # pinned by tests/test_perception_host.py
    for n in ("PoseDetector", "DetectorCfg", "PoseRefinerRaycast", "Mapper"):
        assert not hasattr(A, n)


def test_robot_mesh_members_and_articulated_entry_points():
    from curobo_amd.perception import RobotMesh

    for v, f in ((V, F), (torch.as_tensor(V), torch.as_tensor(F)), (V.astype(np.float64), F.astype(np.int64))):
        m = RobotMesh(v, f, device="cpu")
        assert m.n_vertices == 4 and m.n_faces == 4 and m.is_articulated is False and m.get_dof() == 0 and m.device == torch.device("cpu")
        assert m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32 and np.array_equal(m.vertices.numpy(), V)
    duck = type("T", (), {"vertices": V, "faces": F})()
    assert RobotMesh.from_trimesh(duck, device="cpu").n_faces == 4
    with pytest.raises(ValueError, match=r"vertices \[V, 3\] and faces \[F, 3\]"):
        RobotMesh(V[:, :2], F, device="cpu")
    with pytest.raises(NotImplementedError, match="articulated meshes are not packaged"):
        RobotMesh.from_kinematics(None)
    with pytest.raises(NotImplementedError, match="articulated meshes are not packaged"):
        RobotMesh(V, F, device="cpu").update(torch.zeros(7))


def test_detector_requires_an_initial_pose_and_carries_the_cfg():
    from curobo_amd.perception import DetectionResult, RobotMesh, SDFDetectorCfg, SDFPoseDetector

    det = SDFPoseDetector(RobotMesh(V, F, device="cpu"))
    assert det.config == SDFDetectorCfg() and det.config.max_distance == det.config.distance_threshold == 0.2
    with pytest.raises(ValueError, match="SDFPoseDetector requires an initial_pose estimate"):
        det.detect_from_points(torch.zeros(10, 3))
    assert [f for f in DetectionResult.__dataclass_fields__] == ["pose", "config", "confidence", "alignment_error", "n_iterations", "compute_time"]
