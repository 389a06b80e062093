"""curobo_amd.perception.mapper on the host: MapperCfg's arithmetic and refusals, the exports, and the C entry points' checks
before any launch."""

import ctypes
import importlib.util
import os
import re

import pytest
import torch

from curobo_amd import _lib
from curobo_amd.perception.mapper import Mapper, MapperCfg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(extent_meters_xyz=(1.0, 0.96, 0.4), voxel_size=0.02, image_height=60, image_width=80)


def test_grid_shape_is_nz_ny_nx_and_rounds_up():
    cfg = MapperCfg(**BASE)
    assert cfg.grid_shape == (20, 48, 50)
    assert MapperCfg(**{**BASE, "extent_meters_xyz": (1.001, 0.95, 0.39)}).grid_shape == (20, 48, 51)
    assert cfg.get_actual_extent() == pytest.approx((1.0, 0.96, 0.4))
    assert MapperCfg(**{**BASE, "extent_meters_xyz": (1.001, 0.95, 0.39)}).get_actual_extent() == pytest.approx((1.02, 0.96, 0.4))
    assert cfg.block_grid_shape == (5, 12, 13) and cfg.max_blocks == 780 and cfg.hash_capacity == 1560
    assert cfg.dense_bytes == 780 * 64 * 4
    assert cfg.esdf_grid_shape == (128, 128, 128)
    assert MapperCfg(**BASE, esdf_voxel_size=0.04, extent_esdf_meters_xyz=(1.0, 0.95, 0.39)).esdf_grid_shape == (25, 24, 10)
    assert torch.equal(cfg.grid_center, torch.zeros(3)) and cfg.grid_center.dtype == torch.float32
    assert MapperCfg(**BASE, grid_center=[0.1, 0.2, 0.3]).grid_center.dtype == torch.float32


def test_voxel_world_maps_and_bounds():
    cfg = MapperCfg(**BASE, grid_center=[0.5, 0.0, 0.2])
    lo, hi = cfg.get_grid_bounds()
    assert lo == pytest.approx((0.0, -0.48, 0.0), abs=1e-6) and hi == pytest.approx((1.0, 0.48, 0.4), abs=1e-6)  # (the centre is float32)
    assert cfg.voxel_to_world(0, 0, 0) == pytest.approx((0.01, -0.47, 0.01), abs=1e-6)
    assert cfg.voxel_to_world(19, 47, 49) == pytest.approx((0.99, 0.47, 0.39), abs=1e-6)
    assert cfg.world_to_voxel(*cfg.voxel_to_world(3, 17, 41)) == (3, 17, 41)
    assert cfg.world_to_voxel(0.012, -0.474, 0.018) == (0, 0, 0)
    assert cfg.world_to_voxel(1.2, 0.0, 0.2) == (-1, -1, -1) and cfg.world_to_voxel(0.5, 0.0, -0.011) == (-1, -1, -1)


@pytest.mark.parametrize("field,value", [("decay_factor", 0.9), ("frustum_decay_factor", 0.5), ("enable_static", True),
                                         ("lidar_num_sensors", 1), ("feature_dim", 8), ("seeding_method", "scatter"),
                                         ("edt_solver", "jfa")])
def test_fields_of_what_is_not_built_raise_by_name(field, value):
    with pytest.raises(NotImplementedError, match=field):
        MapperCfg(**BASE, **{field: value})


def test_fields_without_effect_are_accepted():
    cfg = MapperCfg(**BASE, hash_load_factor=0.25, roughness=7.0)
    assert cfg.grid_shape == (20, 48, 50) and cfg.max_blocks == 780 and cfg.hash_capacity == 3120


@pytest.mark.parametrize("kw,match", [
    (dict(extent_meters_xyz=(1.0, 0.0, 1.0)), "extent_meters_xyz"), (dict(voxel_size=0.0), "voxel_size"),
    (dict(truncation_distance=-1.0), "truncation_distance"), (dict(depth_minimum_distance=2.0, depth_maximum_distance=1.0), "depth_minimum_distance"),
    (dict(decay_factor=1.5), "decay_factor"), (dict(hash_load_factor=0.0), "hash_load_factor"), (dict(block_size=3), "block_size"),
    (dict(image_height=None), "image_height"), (dict(image_width=0), "image_width"), (dict(seeding_method="both"), "seeding_method"),
    (dict(edt_solver="fmm"), "edt_solver"), (dict(num_cameras=0), "num_cameras")])
def test_invalid_values_raise(kw, match):
    with pytest.raises(ValueError, match=match):
        MapperCfg(**{**BASE, **kw})


def test_max_dense_bytes_states_the_bytes_needed():
    need = 780 * 64 * 4
    assert MapperCfg(**BASE, max_dense_bytes=need).dense_bytes == need
    with pytest.raises(ValueError, match=f"needs {need} bytes"):
        MapperCfg(**BASE, max_dense_bytes=need - 1)
    # the default map of the reference, 2 m at 5 mm, is 256 MB dense and fits the default bound; 1 mm does not
    assert MapperCfg(extent_meters_xyz=(2.0, 2.0, 2.0), image_height=480, image_width=640).dense_bytes == 400 ** 3 * 4
    with pytest.raises(ValueError, match="max_dense_bytes"):
        MapperCfg(extent_meters_xyz=(2.0, 2.0, 2.0), voxel_size=0.001, image_height=480, image_width=640)


def test_esdf_axes_hold_at_most_1024_cells():
    assert MapperCfg(**BASE, esdf_voxel_size=0.001, extent_esdf_meters_xyz=(1.024, 0.5, 0.5)).esdf_grid_shape[0] == 1024
    with pytest.raises(ValueError, match="1024"):
        MapperCfg(**BASE, esdf_voxel_size=0.001, extent_esdf_meters_xyz=(0.5, 1.025, 0.5))


def test_exports():
    """the names live in curobo_amd.perception.mapper.  curobo_amd.perception and curobo/perception.py stay as
    tests/test_pose_detector_host.py and tests/test_perception_host.py pin them: no attribute Mapper, __all__ unchanged"""
    import curobo_amd.perception as P
    from curobo_amd.perception import mapper as M

    assert M.Mapper is Mapper and M.MapperCfg is MapperCfg and {"Mapper", "MapperCfg"} <= set(M.__all__)
    assert not hasattr(P, "Mapper") and "Mapper" not in P.__all__
    spec = importlib.util.spec_from_file_location("_facade_perception", os.path.join(REPO, "curobo", "perception.py"))
    per = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(per)
    assert not hasattr(per, "Mapper") and per.__all__ == ["FilterDepth", "RobotSegmenter"]


def test_params_struct_matches_the_header():
    from curobo_amd.backends import mapper as B

    text = open(_lib.HEADER_PATH).read()
    body = text[text.index("typedef struct curobo_hip_mapper_params {"):text.index("} curobo_hip_mapper_params;")]
    assert ctypes.sizeof(B.MapperParams) == 8 * 4 + 3 * 4 + 6 * 4
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    pos = [re.search(rf"\b{name}\b", body).start() for name, _ in B.MapperParams._fields_]
    assert pos == sorted(pos), "the ctypes fields follow the order of the C struct"
    p = B.make_params((20, 48, 50), 4, (0.0, 0.0, 0.0), 0.02, 0.08, 0.1, 5.0, 0.1)
    assert (p.grid_w, p.grid_h, p.grid_d, p.nbx, p.nby, p.nbz) == (50, 48, 20, 13, 12, 5) and p.n_blocks == 780
    assert p.num_samples == 4 and p.step_size == pytest.approx(0.08 / 1.42) and B.mask_bytes(p) == 780


def test_entry_points_validate_before_any_launch():
    from curobo_amd.backends import mapper as B

    lib = _lib.load()
    err = lib.curobo_hip_last_error
    p = B.make_params((20, 48, 50), 4, (0.0, 0.0, 0.0), 0.02, 0.08, 0.1, 5.0, 0.1)
    pp = ctypes.addressof(p)
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    assert lib.curobo_hip_mapper_clear_mask(None, 4, None) == 1 and b"must not be null" in err()
    assert lib.curobo_hip_mapper_clear_mask(a, 6, None) == 1 and b"multiple of 4" in err()
    assert lib.curobo_hip_mapper_mark_blocks(a, a, a, a, a, a, None, 1, 60, 80, None) == 1 and b"params must not be null" in err()
    assert lib.curobo_hip_mapper_mark_blocks(a, a, None, a, a, a, pp, 1, 60, 80, None) == 1 and b"depth" in err()
    assert lib.curobo_hip_mapper_mark_blocks(None, a, a, a, a, a, pp, 1, 60, 80, None) == 1 and b"frame_mask" in err()
    assert lib.curobo_hip_mapper_integrate(a, a, a, a, a, a, pp, 0, 60, 80, None) == 1 and b"(n_cameras, H, W)" in err()
    assert lib.curobo_hip_mapper_integrate(None, a, a, a, a, a, pp, 1, 60, 80, None) == 1 and b"block_data" in err()
    assert lib.curobo_hip_mapper_esdf_seed(a, a, a, a, a, pp, 1025, 4, 4, None) == 1 and b"10 bits per axis" in err()
    assert lib.curobo_hip_mapper_esdf_seed(None, a, a, a, a, pp, 4, 4, 4, None) == 1 and b"sites" in err()
    assert lib.curobo_hip_mapper_edt_pass(a, a + 128, 2, 2, 2, 3, None) == 1 and b"axis" in err()
    assert lib.curobo_hip_mapper_edt_pass(a, a + 16, 2, 2, 2, 0, None) == 1 and b"overlap" in err()
    assert lib.curobo_hip_mapper_edt_pass(a, a + 128, 2, 0, 2, 0, None) == 1 and b"1..1024" in err()
    assert lib.curobo_hip_mapper_esdf_distance(a, None, a, a, a, a, pp, 4, 4, 4, None) == 1 and b"distance and sites" in err()
    assert lib.curobo_hip_mapper_occupied_flags(None, a, a, pp, 0, 0.02, None) == 1 and b"flags" in err()
    bad = B.make_params((20, 48, 50), 4, (0.0, 0.0, 0.0), 0.02, 0.08, 0.1, 5.0, 0.1)
    bad.block_size = 3
    assert lib.curobo_hip_mapper_occupied_flags(a, a, a, ctypes.addressof(bad), 0, 0.02, None) == 1 and b"power of two" in err()
    bad.block_size, bad.nbx = 4, 12
    assert lib.curobo_hip_mapper_occupied_flags(a, a, a, ctypes.addressof(bad), 0, 0.02, None) == 1 and b"ceil(grid / block_size)" in err()
    with pytest.raises(ValueError, match="axis"):
        _lib.check(lib.curobo_hip_mapper_edt_pass(a, a + 128, 2, 2, 2, -1, None))
