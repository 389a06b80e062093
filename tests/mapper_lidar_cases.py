"""The lidar tests' scene: the grid and the sphere over the ground of tests/mapper_cases.py (50 x 48 x 20 voxels of 0.02 m in blocks
of 4, a 0.25 m sphere at the origin over z = -0.15), seen by lidars that stand INSIDE the grid, as a lidar on a robot does.

Sensor A: 32 x 256 pixels at (0.38, -0.33, 0.10), yawed -0.71 rad, so that its -x axis, where azimuth jumps from +pi to -pi between
the last column and the first, points at the sphere: the seam's columns carry the nearest surface.  Elevation -0.6 .. 0.5 rad, valid
range 0.1 .. 5 m.  Sensor B: the same image from the other side, yawed and tilted about two axes, so that the rotation into the
sensor frame has no zero.  Sensor P: a planar scan, 1 x 256 at elevation -0.3 rad.  What the restatement says about them is
asserted in tests/test_mapper_lidar_host.py, where it costs no GPU time."""

import functools
import math

import numpy as np

import mapper_cases as C
import mapper_lidar_ref as LR
import mapper_ref as R

H, W = 32, 256
VALID_RANGE = (0.1, 5.0)
ELEVATION = (-0.6, 0.5)
PLANAR_ELEVATION = -0.3
LINEAR_VOX, NEAREST_VOX = 2.0, 0.5  # MapperLidarCfg's defaults
#: the guards in metres as the launch receives them: the product in double, passed as a float32
LINEAR_MAX_DIFF = LR.f32(LINEAR_VOX * C.CFG["voxel_size"])
NEAREST_MAX_DIST = LR.f32(NEAREST_VOX * C.CFG["voxel_size"])


def _quat(yaw: float, pitch: float = 0.0, roll: float = 0.0) -> np.ndarray:
    """wxyz of Rz(yaw) Ry(pitch) Rx(roll)"""
    cy, sy, cp, sp, cr, sr = (f(0.5 * a) for a in (yaw, pitch, roll) for f in (math.cos, math.sin))
    return np.array([cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr])


#: name -> (position, wxyz quaternion, H, (min_elev, max_elev))
SENSORS = {"A": ((0.38, -0.33, 0.10), _quat(-0.71), H, ELEVATION),
           "B": ((-0.36, 0.31, 0.12), _quat(0.45, 0.12, -0.08), H, ELEVATION),
           "P": ((0.30, 0.34, 0.11), _quat(-2.2), 1, (PLANAR_ELEVATION, PLANAR_ELEVATION)),
           # the forgetting test's: over the -x -y corner, looking steeply down at a ring of ground, the sphere out of its band
           "T": ((-0.42, -0.40, 0.12), _quat(0.3), H, (-1.4, -1.1))}


@functools.lru_cache(maxsize=None)
def sensor(name: str):
    """(range [H, W], position [3], quaternion [4], valid_range [2], elevation_range [2]) of a sensor, float32"""
    pos, quat, h, elev = SENSORS[name]
    pos, quat, elev = np.asarray(pos, np.float32), np.asarray(quat, np.float32), np.asarray(elev, np.float32)
    return LR.render_range(pos, quat, h, W, float(elev[0]), float(elev[1])), pos, quat, np.asarray(VALID_RANGE, np.float32), elev


def frame(*names: str):
    """the sensors stacked: (range [n, H, W], position [n, 3], quaternion [n, 4], valid_range [n, 2], elevation_range [n, 2])"""
    return tuple(np.stack(a) for a in zip(*(sensor(n) for n in names)))


@functools.lru_cache(maxsize=None)
def grid(block_size: int = 4) -> "R.Grid":
    from curobo_amd.perception.mapper import MapperCfg

    return R.Grid.from_cfg(MapperCfg(**{**C.CFG, "block_size": block_size}))


#: the runs of the device tests, each on a mapper of its own (the number of sensors is the mapper's): name -> the frames in order, a
#: frame = (camera indices of mapper_cases or None, lidar names or None)
RUNS = {"single": ((None, ("A",)), (None, ("B",))),          # k = 2 lidar frames of one sensor
        "pair": ((None, ("A", "B")),),                       # two sensors in one frame
        "planar": ((None, ("P",)),),                         # H = 1
        "mixed": (((0,), ("A",)),)}                          # a camera and a lidar in one frame


def oracle_frame(g: "R.Grid", sw, w, cams, lidars, paths=None):
    """one frame on the oracle: the camera stages, then the lidar stages over the LIDAR's sure blocks (integrator_tsdf.py:485-492).
    dict(sw, w, sure, possible: the frame's union; cam_*, lidar_*: each kind's; updated, ambiguous)"""
    n, v = g.n_blocks, g.bs ** 3
    zero = np.zeros(n, bool)
    out = dict(cam_sure=zero, cam_possible=zero, lidar_sure=zero, lidar_possible=zero, cam_updated=np.zeros((n, v), bool),
               lidar_updated=np.zeros((n, v), bool))
    upd, amb = np.zeros((n, v), bool), np.zeros((n, v), bool)
    if cams is not None:
        f = C.frame(*cams)
        out["cam_sure"], out["cam_possible"] = R.mark_blocks(g, *f)
        sw, w, u, a = R.integrate(g, sw, w, out["cam_sure"], *f)
        out["cam_updated"] = u
        upd, amb = upd | u, amb | a
    if lidars is not None:
        f = frame(*lidars)
        out["lidar_sure"], out["lidar_possible"] = LR.mark_blocks(g, *f)
        sw, w, u, a = LR.integrate(g, sw, w, out["lidar_sure"], *f, LINEAR_MAX_DIFF, NEAREST_MAX_DIST, paths=paths)
        out["lidar_updated"] = u
        upd, amb = upd | u, amb | a
    out.update(sw=sw, w=w, updated=upd, ambiguous=amb, sure=out["cam_sure"] | out["lidar_sure"],
               possible=out["cam_possible"] | out["lidar_possible"])
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(name: str):
    """the oracle over the frames of RUNS[name] from an empty map: a list of oracle_frame dicts (each with ``paths``)"""
    g = grid()
    sw, w = np.zeros((g.n_blocks, g.bs ** 3), np.float16), np.zeros((g.n_blocks, g.bs ** 3), np.float16)
    out = []
    for cams, lidars in RUNS[name]:
        paths = {}
        s = oracle_frame(g, sw, w, cams, lidars, paths)
        s["paths"] = paths
        sw, w = s["sw"], s["w"]
        out.append(s)
    return out


# ---------------------------------------------------------------------------------------------------- decay
TIME_DECAY, FRUSTUM_DECAY = 0.97, 0.5
#: the frustum test's lidars: a short far bound and a narrow elevation band, so that a good part of the visible blocks is out by
#: the range band, another by the elevation band, and the rest in; and a planar one, in only about its one elevation
DECAY_LIDARS = {"band": (((0.38, -0.33, 0.10), _quat(-0.71), (0.1, 0.45), (-0.35, 0.1)), ((-0.36, 0.31, 0.12), _quat(0.45, 0.12, -0.08), (0.2, 0.4), (-0.5, -0.1))),
                "planar": (((0.30, 0.34, 0.11), _quat(-2.2), (0.1, 0.6), (PLANAR_ELEVATION, PLANAR_ELEVATION)),)}


def decay_lidars(name: str):
    """(position [n, 3], quaternion [n, 4], valid_range [n, 2], elevation_range [n, 2], H) float32"""
    rows = DECAY_LIDARS[name]
    return tuple(np.asarray([r[k] for r in rows], np.float32) for k in range(4)) + (1 if name == "planar" else H,)


FORGET_TIME_DECAY = 0.1


@functools.lru_cache(maxsize=None)
def forgetting():
    """the restatement's run of the forgetting test: sensor A once, then sensor T with time_decay = 0.1 (the uniform path: no frustum
    is tested) until every block that A saw and T does not mark is recycled.  dict(frames: how many T frames that took, first:
    A's sure blocks, turned_sure / turned_possible: T's, either_sum: a block sum came within tolerance of the threshold)"""
    import mapper_decay_ref as DR

    g = grid()
    n, v = g.n_blocks, g.bs ** 3
    a = oracle_frame(g, np.zeros((n, v), np.float16), np.zeros((n, v), np.float16), None, ("A",))
    data, visible = np.stack([a["sw"], a["w"]], -1), a["sure"].copy()
    t_sure, t_possible = LR.mark_blocks(g, *frame("T"))
    either = False
    for k in range(1, 40):
        data, visible, _, e = DR.step_uniform(data, visible, g.bs, FORGET_TIME_DECAY)
        either |= bool(e.any())
        s = oracle_frame(g, data[..., 0], data[..., 1], None, ("T",))
        data, visible = np.stack([s["sw"], s["w"]], -1), visible | t_sure
        if not (visible & ~t_possible).any():
            return dict(frames=k, first=a["sure"], first_possible=a["possible"], turned_sure=t_sure, turned_possible=t_possible, either_sum=either)
    raise AssertionError("the first frame's blocks never go")
