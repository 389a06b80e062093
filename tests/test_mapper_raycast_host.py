"""The renderer and the pose refiner on the host: the exports, the refusals, the C entry points' checks before any launch, the
stride and iteration arithmetic, the colormaps."""

import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from curobo_amd import _lib
from curobo_amd.perception import mapper as M
from curobo_amd.perception.mapper import renderer as RD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports():
    names = {"BlockSparseTSDFRenderer", "BlockSparseTSDFRendererCfg", "BlockSparseRaycastPoseRefiner", "BlockSparseRaycastRefinerCfg"}
    assert names <= set(M.__all__) and all(hasattr(M, n) for n in names)
    assert {"Mapper", "MapperCfg", "DenseTSDF"} <= set(M.__all__)
    for method in ("_get_renderer", "render", "render_color", "render_depth", "render_color_only", "render_shaded", "render_depth_colormap",
                   "render_normal_colormap"):
        assert callable(getattr(M.Mapper, method))
    import curobo_amd.perception as P

    assert not hasattr(P, "BlockSparseTSDFRenderer") and "BlockSparseTSDFRenderer" not in P.__all__
    spec = importlib.util.spec_from_file_location("_facade_perception", os.path.join(REPO, "curobo", "perception.py"))
    per = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(per)
    assert per.__all__ == ["FilterDepth", "RobotSegmenter"]
    assert _lib.load().curobo_hip_abi_version() == 7
    assert {"curobo_hip_mapper_raycast", "curobo_hip_mapper_ray_align"} <= set(_lib.declared_symbols())


def test_renderer_refusals_come_before_the_device():
    r = object.__new__(M.BlockSparseTSDFRenderer)  # no mapper, no buffers: a refusal must not need them
    K, pose = torch.eye(3), None  # (the pose is never looked at)
    with pytest.raises(NotImplementedError, match="colour channel"):
        r.render_shaded(K, pose, (4, 4), use_color=True)
    for shape in ((0, 4), (4, -1), (4,), 7, (4, 4, 4), ("a", 4)):
        with pytest.raises(ValueError, match="image_shape"):
            r.render(K, pose, shape)
    for bad in (torch.zeros(5), torch.zeros(3, 4), torch.zeros(2, 2), torch.zeros(1, 3, 3)):
        with pytest.raises(ValueError, match="intrinsics"):
            r.render(bad, pose, (4, 4))
    k = RD.intrinsics_matrix(torch.tensor([60.0, 61.0, 40.3, 29.6]))
    assert k.dtype == torch.float32 and k[0, 0] == 60.0 and k[1, 1] == 61.0 and k[0, 2] == pytest.approx(40.3) and k[1, 2] == pytest.approx(29.6)
    assert RD.image_shape_hw([3, 5]) == (3, 5)
    cfg = M.BlockSparseTSDFRendererCfg()
    assert (cfg.depth_minimum_distance, cfg.depth_maximum_distance, cfg.minimum_tsdf_weight, cfg.use_block_acceleration) == (0.2, 15.0, 0.2, True)


def test_refiner_cfg_arithmetic_and_defaults():
    c = M.BlockSparseRaycastRefinerCfg()
    assert (c.n_points, c.minimum_valid_depth_pixels, c.max_iterations, c.inner_iterations) == (92160, 100, 100, 4)
    assert (c.distance_threshold, c.min_valid_ratio, c.n_samples_per_ray, c.tile_block_dim) == (0.1, 0.1, 1, 256)
    assert (c.depth_minimum_distance, c.depth_maximum_distance, c.minimum_tsdf_weight) == (0.1, 10.0, 2.0)
    assert (c.lambda_initial, c.lambda_factor, c.lambda_min, c.lambda_max, c.rho_min) == (1e-3, 10.0, 1e-7, 1e7, 0.25)
    assert c.outer_iterations == 25
    assert M.BlockSparseRaycastRefinerCfg(max_iterations=10, inner_iterations=4).outer_iterations == 2
    assert M.BlockSparseRaycastRefinerCfg(max_iterations=3, inner_iterations=4).outer_iterations == 0
    assert c.stride(720, 1280) == 3 and c.stride(480, 640) == 1 and c.stride(60, 80) == 1
    assert M.BlockSparseRaycastRefinerCfg(n_points=1200).stride(60, 80) == 2
    assert M.BlockSparseRaycastRefinerCfg(n_points=1199).stride(60, 80) == 2 and M.BlockSparseRaycastRefinerCfg(n_points=1201).stride(60, 80) == 1
    from curobo_amd.backends import mapper as B

    assert B.ray_align_samples((60, 80), 2, 5) == 6000 and B.ray_align_samples((13, 17), 3, 1) == 5 * 6 and B.ray_align_samples((1, 1), 4, 9) == 9


def test_entry_points_validate_before_any_launch():
    from curobo_amd.backends import mapper as B
    from curobo_amd.backends import perception as P

    lib = _lib.load()
    err = lib.curobo_hip_last_error
    p = B.make_params((20, 48, 50), 4, (0.0, 0.0, 0.0), 0.02, 0.08, 0.1, 5.0, 0.1)
    pp = ctypes.addressof(p)
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)

    def raycast(hp=a, hn=a, hd=a, hm=a, k=a, pos=a, quat=a, bd=a, bm=a, params=pp, mw=0.1, lo=0.1, hi=5.0, h=60, w=80, acc=1, z=0):
        return lib.curobo_hip_mapper_raycast(hp, hn, hd, hm, k, pos, quat, bd, bm, params, mw, lo, hi, h, w, acc, z, None)

    assert raycast(params=None) == 1 and b"mapper_raycast: params must not be null" in err()
    assert raycast(hd=None) == 1 and b"hit_depths" in err()
    assert raycast(quat=None) == 1 and b"quaternion" in err()
    assert raycast(bm=None) == 1 and b"block_mask" in err()
    assert raycast(h=0) == 1 and b"H x W" in err()
    assert raycast(w=-3) == 1 and b"H x W" in err()
    assert raycast(lo=2.0, hi=1.0) == 1 and b"depth_minimum_distance" in err()
    assert raycast(mw=-1.0) == 1 and b"minimum_tsdf_weight" in err()

    n = B.ray_align_samples((60, 80), 2, 5)
    need = P.pose_sdf_ws_bytes(n)
    assert need == -(-n // 256) * 32 * 4

    def align(ws=a, nbytes=need, depth=a, k=a, pos=a, quat=a, bd=a, bm=a, params=pp, h=60, w=80, stride=2, ns=5):
        return lib.curobo_hip_mapper_ray_align(ws, nbytes, depth, k, pos, quat, bd, bm, params, 0.1, 0.1, 10.0, 0.1, h, w, stride, ns, None)

    assert align(ws=None) == 1 and b"workspace must not be null" in err()
    assert align(depth=None) == 1 and b"depth" in err()
    assert align(pos=None) == 1 and b"position" in err()
    assert align(bd=None) == 1 and b"block_data" in err()
    assert align(params=None) == 1 and b"mapper_ray_align: params must not be null" in err()
    assert align(stride=0) == 1 and b"stride must be at least 1" in err()
    for ns in (0, 4, 10, 11, -1):
        assert align(ns=ns) == 1 and b"n_samples_per_ray must be odd and in 1..9" in err()
    assert align(h=0) == 1 and b"(H, W)" in err()
    assert align(nbytes=need - 32 * 4) == 1 and b"workspace of" in err() and b"6000 samples" in err() and b"curobo_hip_pose_sdf_ws_bytes" in err()
    assert align(ws=a + 2) == 1 and b"4-byte aligned" in err()
    with pytest.raises(ValueError, match="stride"):
        _lib.check(align(stride=-2))


def _turbo(t):
    """the reference's polynomial (renderer.py:466-481), in float64"""
    r = 0.13572138 + t * (4.61539260 + t * (-42.66032258 + t * (132.13108234 + t * (-152.94239396 + t * 59.28637943))))
    g = 0.09140261 + t * (2.19418839 + t * (4.84296658 + t * (-14.18503333 + t * (4.27729857 + t * 2.82956604))))
    b = 0.10667330 + t * (12.64194608 + t * (-60.58204836 + t * (110.36276771 + t * (-89.90310912 + t * 27.34824973))))
    return np.clip(np.stack([r, g, b], -1), 0, 1) * 255


def test_colormaps():
    depth = torch.tensor([[0.05, 0.1, 1.3, 2.55, 4.999, 7.0]])  # below, at the minimum, three inside, above the maximum
    valid = torch.tensor([[True, True, True, False, True, True]])
    out = M.depth_to_colormap(depth, 0.1, 5.0, valid)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1, 6, 3)
    want = _turbo(np.clip((depth.numpy().astype(np.float64) - 0.1) / 4.9, 0, 1))
    got = out.numpy().astype(np.float64)
    keep = valid.numpy()
    assert (np.abs(got - np.floor(want))[keep] <= 1).all()  # (uint8 truncates; the float32 polynomial may sit one step off)
    assert (got[~keep] == 0).all() and got[0, 0].tolist() == got[0, 1].tolist() and got[0, 5].tolist() == np.floor(_turbo(np.float64(1.0))).tolist()
    assert M.depth_to_colormap(torch.tensor([[0.0, 1.0]]))[0, 0].tolist() == [0, 0, 0]  # the default mask is depth > 0
    assert M.depth_to_colormap(depth, 0.1, 5.0, valid, invalid_color=(9, 8, 7))[0, 3].tolist() == [9, 8, 7]
    normals = torch.tensor([[[0.0, 0.0, 1.0], [-1.0, 1.0, 0.0], [0.6, -0.8, 0.0]]])
    n = M.normals_to_colormap(normals, torch.tensor([[True, True, False]]))
    assert n.dtype == torch.uint8 and n[0, 0].tolist() == [127, 127, 255] and n[0, 1].tolist() == [0, 255, 127] and n[0, 2].tolist() == [128, 128, 128]
