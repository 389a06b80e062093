"""The ICP pose detector on the host: the four C entry points and the shim validate before any launch, the workspace sizes,
``DetectorCfg`` against the reference's recorded defaults, where the names import from, ``RobotMesh.sample_surface_points`` and
``resample_points`` on the CPU, and the oracle's step on a case worked by hand.  No GPU is needed."""

import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import pose_icp_ref as R
from curobo_amd import _lib
from curobo_amd.backends import perception as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_icp_golden.npz")
V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) * np.array([0.3, 0.2, 0.12], np.float32)
F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)
NAMES = ("curobo_hip_pose_icp_ws_bytes", "curobo_hip_pose_icp_correspond", "curobo_hip_pose_icp_step", "curobo_hip_pose_icp_select")


def test_symbols_are_declared_and_the_abi_is_unchanged():
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.declared_symbols() and n in _lib._signatures() and hasattr(lib, n)
    assert lib.curobo_hip_abi_version() == 7
    assert C.sizeof(P.PoseICPState) == 4 * P.POSE_ICP_STATE_WORDS == 4 * 24
    assert P.pose_icp_state_slice("T") == slice(0, 12) and P.pose_icp_state_slice("error") == slice(12, 13)
    assert [P.pose_icp_state_slice(n).start for n in ("iterations", "stopped", "solver_failed", "n_valid", "x")] == [13, 14, 15, 16, 17]
    assert (P.POSE_ICP_COARSE, P.POSE_ICP_FINE, P.POSE_ICP_FINALIZE) == (0, 1, 2)


def test_workspace_query():
    lib = _lib.load()
    nbytes = C.c_int64(-1)
    out = C.cast(C.pointer(nbytes), C.c_void_p)
    assert lib.curobo_hip_pose_icp_ws_bytes(1, 5, None) == 1 and b"out_bytes must not be null" in lib.curobo_hip_last_error()
    assert lib.curobo_hip_pose_icp_ws_bytes(0, 5, out) == 1 and b"n_hypotheses must be in 1..65535, got 0" in lib.curobo_hip_last_error()
    assert lib.curobo_hip_pose_icp_ws_bytes(70000, 5, out) == 1 and b"n_hypotheses must be in 1..65535" in lib.curobo_hip_last_error()
    assert lib.curobo_hip_pose_icp_ws_bytes(1, 0, out) == 1 and b"n_mesh must be positive, got 0" in lib.curobo_hip_last_error()
    # one row of POSE_WS_ROW words per 64 samples and hypothesis
    for (h, m), rows in (((1, 1), 1), ((1, 256), 4), ((1, 257), 5), ((8, 500), 64)):
        assert lib.curobo_hip_pose_icp_ws_bytes(h, m, out) == 0 and nbytes.value == rows * P.POSE_WS_ROW * 4
        assert P.pose_icp_ws_bytes(h, m) == nbytes.value
    with pytest.raises(ValueError, match="n_mesh must be positive"):
        P.pose_icp_ws_bytes(1, -3)


def test_correspond_arguments_are_validated_without_a_gpu():
    lib = _lib.load()
    mp, mn, ob, st, ws = torch.zeros(100, 3), torch.zeros(100, 3), torch.zeros(50, 3), torch.zeros(2, P.POSE_ICP_STATE_WORDS), torch.zeros(128)
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(work=p(ws), nbytes=512, points=p(mp), normals=p(mn), observed=p(ob), state=p(st), thr=0.1, hub=1, delta=0.02, h=2, m=100, o=50):
        return lib.curobo_hip_pose_icp_correspond(None, None, work, nbytes, points, normals, observed, state, thr, hub, delta, 1, h, m, o, None)

    for kw in (dict(work=None), dict(points=None), dict(normals=None), dict(observed=None), dict(state=None)):
        assert call(**kw) == 1 and b"must not be null" in lib.curobo_hip_last_error()
    assert call(h=0) == 1 and b"n_hypotheses must be in 1..65535, got 0" in lib.curobo_hip_last_error()
    assert call(m=0) == 1 and b"n_mesh must be positive, got 0" in lib.curobo_hip_last_error()
    assert call(o=0) == 1 and b"n_observed must be positive, got 0" in lib.curobo_hip_last_error()
    assert call(o=-2) == 1
    assert call(thr=0.0) == 1 and b"distance_threshold must be positive" in lib.curobo_hip_last_error()
    assert call(thr=float("nan")) == 1 and b"distance_threshold must be positive" in lib.curobo_hip_last_error()
    assert call(delta=0.0) == 1 and b"huber_delta must be positive, got 0" in lib.curobo_hip_last_error()
    assert call(delta=-1.0) == 1 and b"huber_delta" in lib.curobo_hip_last_error()
    assert call(nbytes=511) == 1 and b"workspace of 511 bytes, 2 hypotheses of 100 samples need 512" in lib.curobo_hip_last_error()
    assert call(work=p(ws) + 2) == 1 and b"workspace must be 4-byte aligned" in lib.curobo_hip_last_error()
    assert call(state=p(st) + 1) == 1 and b"state must be 4-byte aligned" in lib.curobo_hip_last_error()
    with pytest.raises(ValueError, match="workspace of 511 bytes"):
        _lib.check(call(nbytes=511))
    # the shim names the shape or dtype
    ok = dict(distance_threshold=0.1, use_huber=True, huber_delta=0.02)
    with pytest.raises(ValueError, match=r"state must be \(H, 24\), got \(24,\)"):
        P.pose_icp_correspond(ws, mp, mn, ob, st[0], **ok)
    with pytest.raises(ValueError, match=r"mesh_points must be \(N, 3\), got \(100, 2\)"):
        P.pose_icp_correspond(ws, torch.zeros(100, 2), mn, ob, st, **ok)
    with pytest.raises(ValueError, match=r"observed_points must be a contiguous torch.float32"):
        P.pose_icp_correspond(ws, mp, mn, ob.double(), st, **ok)
    with pytest.raises(ValueError, match=r"mesh_normals must have shape \(100, 3\), got \(99, 3\)"):
        P.pose_icp_correspond(ws, mp, torch.zeros(99, 3), ob, st, **ok)
    with pytest.raises(ValueError, match=r"out_index must be a contiguous torch.int32"):
        P.pose_icp_correspond(ws, mp, mn, ob, st, out_index=torch.zeros(2, 100), **ok)
    with pytest.raises(ValueError, match=r"out_distance must have shape \(2, 100\), got \(100,\)"):
        P.pose_icp_correspond(ws, mp, mn, ob, st, out_distance=torch.zeros(100), **ok)
    with pytest.raises(ValueError, match="workspace must be a contiguous tensor"):
        P.pose_icp_correspond(torch.zeros(128, 2)[:, 0], mp, mn, ob, st, **ok)


def test_step_and_select_arguments_are_validated_without_a_gpu():
    lib = _lib.load()
    st, ws, idx = torch.zeros(2, P.POSE_ICP_STATE_WORDS), torch.zeros(128), torch.zeros(1, dtype=torch.int32)
    p = lambda t: t.data_ptr()  # noqa: E731

    def step(state=p(st), work=p(ws), nbytes=512, h=2, m=100, mode=0):
        return lib.curobo_hip_pose_icp_step(state, work, nbytes, h, m, mode, None)

    assert step(state=None) == 1 and b"state and workspace must not be null" in lib.curobo_hip_last_error()
    assert step(work=None) == 1 and b"state and workspace must not be null" in lib.curobo_hip_last_error()
    assert step(state=p(st) + 2) == 1 and b"state must be 4-byte aligned" in lib.curobo_hip_last_error()
    assert step(h=0) == 1 and b"n_hypotheses must be in 1..65535" in lib.curobo_hip_last_error()
    assert step(m=-1) == 1 and b"n_mesh must be positive, got -1" in lib.curobo_hip_last_error()
    for mode in (-1, 3):
        assert step(mode=mode) == 1 and f"mode must be 0 (coarse), 1 (fine) or 2 (finalize), got {mode}".encode() in lib.curobo_hip_last_error()
    assert step(nbytes=256) == 1 and b"workspace of 256 bytes, 2 hypotheses of 100 samples need 512" in lib.curobo_hip_last_error()
    with pytest.raises(ValueError, match=r"state must be \(H, 24\)"):
        P.pose_icp_step(torch.zeros(2, 23), ws, 100, 0)
    with pytest.raises(ValueError, match="state must be a contiguous torch.float32"):
        P.pose_icp_step(st.to(torch.int32), ws, 100, 0)

    def select(out=p(idx), state=p(st), h=2):
        return lib.curobo_hip_pose_icp_select(out, None, None, state, h, None)

    assert select(out=None) == 1 and b"out_index and state must not be null" in lib.curobo_hip_last_error()
    assert select(state=None) == 1 and b"out_index and state must not be null" in lib.curobo_hip_last_error()
    assert select(h=0) == 1 and b"n_hypotheses must be positive, got 0" in lib.curobo_hip_last_error()
    with pytest.raises(ValueError, match="out_index must be a contiguous torch.int32"):
        P.pose_icp_select(torch.zeros(1), st)
    with pytest.raises(ValueError, match="out_transform must hold 12 values, got 16"):
        P.pose_icp_select(idx, st, out_transform=torch.zeros(16))
    with pytest.raises(ValueError, match="out_error must hold 1 values, got 2"):
        P.pose_icp_select(idx, st, out_error=torch.zeros(2))


def test_detector_cfg_defaults_are_the_references_and_svd_raises():
    import dataclasses

    from curobo_amd.perception.pose_estimation import DetectorCfg

    g = np.load(GOLDEN)
    names, values = g["cfg_default_names"].tolist(), g["cfg_default_values"].tolist()
    cfg = DetectorCfg()
    assert [f.name for f in dataclasses.fields(DetectorCfg)] == names + ["device_cfg"]
    assert [float(getattr(cfg, n)) for n in names] == values
    assert len(names) == 13 and cfg.n_rotation_samples == 64 and cfg.huber_delta == 0.02
    with pytest.raises(NotImplementedError, match="the SVD solver is not packaged"):
        DetectorCfg(use_svd=True)


def test_names_import_from_the_subpackage_and_the_facade_only():
    from conftest import ROOT

    from curobo_amd import perception as A
    from curobo_amd.perception import pose_estimation as PE

    spec = importlib.util.spec_from_file_location("_facade_curobo_perception_icp", os.path.join(ROOT, "curobo/perception.py"))
    per = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(per)
    for n in ("PoseDetector", "DetectorCfg"):
        assert n in PE.__all__ and getattr(per, n) is getattr(PE, n)
        assert not hasattr(A, n) and n not in per.__all__
    assert per.__all__ == ["FilterDepth", "RobotSegmenter"]
    from curobo_amd.perception.pose_estimation.util import resample_points  # noqa: F401


def test_sample_surface_points_on_the_cpu():
    from curobo_amd.perception.pose_estimation import RobotMesh

    torch.manual_seed(3)
    mesh = RobotMesh(V, F, device="cpu")
    pts, nrm = mesh.sample_surface_points(300)
    assert tuple(pts.shape) == tuple(nrm.shape) == (300, 3) and pts.dtype == nrm.dtype == torch.float32
    assert torch.allclose(nrm.norm(dim=1), torch.ones(300), atol=1e-5)
    # every point lies on a face whose normal is the one returned: barycentric residual below 1e-6
    a, b, c = (V[F[:, k]].astype(np.float64) for k in range(3))
    P64, N64 = pts.numpy().astype(np.float64), nrm.numpy().astype(np.float64)
    best = np.full(300, np.inf)
    for k in range(len(F)):
        M = np.stack([b[k] - a[k], c[k] - a[k]], 1)  # [3, 2]
        uv, *_ = np.linalg.lstsq(M, (P64 - a[k]).T, rcond=None)
        res = np.linalg.norm(M @ uv - (P64 - a[k]).T, axis=0)
        inside = (uv[0] >= -1e-6) & (uv[1] >= -1e-6) & (uv.sum(0) <= 1 + 1e-6)
        fn = np.cross(b[k] - a[k], c[k] - a[k])
        same_normal = np.abs(N64 @ (fn / np.linalg.norm(fn)) - 1.0) < 1e-5
        best = np.where(inside & same_normal, np.minimum(best, res), best)
    assert best.max() < 1e-6
    assert len(set(np.argmax(np.abs(N64 @ np.stack([np.cross(b[k] - a[k], c[k] - a[k]) for k in range(4)]).T), 1))) > 1  # several faces drawn
    again_p, again_n = mesh.sample_surface_points(300)
    assert torch.equal(again_p, pts) and torch.equal(again_n, nrm)  # the cache
    other, _ = mesh.sample_surface_points(200)
    assert tuple(other.shape) == (200, 3) and torch.equal(mesh.sample_surface_points(300)[0], pts)  # kept per count
    fresh, _ = mesh.sample_surface_points(300, resample=True)
    assert not torch.equal(fresh, pts)
    assert torch.equal(mesh.sample_surface_points(300)[0], fresh)


def test_resample_points_gives_exact_counts_both_ways():
    from curobo_amd.perception.pose_estimation.util import resample_points

    torch.manual_seed(5)
    pts = torch.arange(90, dtype=torch.float32).reshape(30, 3)
    down = resample_points(pts, 12)
    assert tuple(down.shape) == (12, 3) and len({tuple(r) for r in down.tolist()}) == 12  # a subset, nothing twice
    up = resample_points(pts, 100)
    assert tuple(up.shape) == (100, 3)
    rows = {tuple(r) for r in pts.tolist()}
    assert all(tuple(r) in rows for r in up.tolist()) and len({tuple(r) for r in up.tolist()}) < 100  # repeats
    assert tuple(resample_points(pts, 30).shape) == (30, 3)


def test_too_few_points_raise_before_any_launch():
    from curobo_amd.perception.pose_estimation import DetectorCfg, PoseDetector, RobotMesh
    from curobo_amd.types import DeviceCfg

    det = PoseDetector(RobotMesh(V, F, device="cpu"), DetectorCfg(device_cfg=DeviceCfg(device="cpu")))
    pts = torch.rand(12, 3)
    pts[:3, 0] = float("nan")
    with pytest.raises(ValueError, match="Not enough valid points: 9"):
        det.detect_from_points(pts)
    R3 = det._sample_rotations(16)
    assert tuple(R3.shape) == (16, 3, 3)
    assert torch.allclose(R3 @ R3.transpose(1, 2), torch.eye(3).expand(16, 3, 3), atol=1e-5) and torch.allclose(torch.linalg.det(R3), torch.ones(16), atol=1e-5)


def test_the_oracle_step_on_a_pure_translation():
    """a unit cube's six face centres, normals along the axes, each observed 1 mm further out along x: with the samples
    placed symmetrically the rotation rows cancel and the solve is t = (sum n n^T + 1e-6 I)^-1 sum n b by hand"""
    p = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * 0.5
    p = np.concatenate([p, p])  # 12 samples: more than the minimum of 10
    n = p / 0.5
    o = p + [1e-3, 0, 0]
    T = np.eye(4)[:3]
    c = R.correspond(p, n, o, T, 0.1, True, 0.02)
    assert c["count"] == 12 and np.array_equal(c["index"], [0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5])  # duplicates: the lowest index
    assert not c["excluded"].any()
    st = R.step(c["JtJ"], c["Jtb"], c["count"], T, R.COARSE)
    # sum n n^T = diag(4, 4, 4); sum n b = (4 * 1e-3, 0, 0); no rotation
    want = np.array([0, 0, 0, 4e-3 / (4 + 1e-6), 0, 0])
    assert np.allclose(st["x"], want, atol=1e-15) and not st["stopped"]
    assert np.allclose(st["T"], np.c_[np.eye(3), want[3:]], atol=1e-15)
    assert R.step(c["JtJ"], c["Jtb"], 9, T, R.COARSE)["stopped"] and R.step(c["JtJ"], c["Jtb"], 9, T, R.COARSE)["x"] is None
    fine = R.step(c["JtJ"] , c["Jtb"] * 0.05, c["count"], T, R.FINE)  # |t| = 5e-5 < 1e-4: stops before the update
    assert fine["stopped"] and np.array_equal(fine["T"], T)
    assert np.allclose(R.pose_error(st["T"], T), (want[3], 0.0), atol=1e-12)
