"""The mapper tests' scene: the smallest at which every path of csrc/mapper.hip is live.  TSDF 50 x 48 x 20 voxels of 0.02 m in
blocks of 4 (50 = 12 blocks + 2 voxels: the padded last block is exercised), ESDF 25 x 24 x 10 cells of 0.04 m, an 80 x 60 camera
with fx = fy = 60 and the principal point a fraction of a pixel off the centre, rolled and tilted; a 0.25 m sphere at the origin
over the ground z = -0.15, background 0.

The ESDF grid is centred a quarter of a TSDF voxel off the TSDF's centre: concentric grids with a whole ratio of cell to voxel
put the cell centres and the +-half-cell probes ON voxel faces, where the reference's (int) of a float32 quotient and a float64
one may pick different voxels (mapper_ref.tsdf_sample flags such probes)."""

import numpy as np

import mapper_ref as R

H, W = 60, 80
CFG = dict(extent_meters_xyz=(1.0, 0.96, 0.4), voxel_size=0.02, esdf_voxel_size=0.04, extent_esdf_meters_xyz=(1.0, 0.96, 0.4),
           truncation_distance=0.08, block_size=4, image_height=H, image_width=W, num_cameras=2, depth_minimum_distance=0.1,
           depth_maximum_distance=5.0)
ESDF_SHAPE = (25, 24, 10)
ESDF_ORIGIN = (0.005, 0.005, 0.005)
K = np.array([[60.0, 0.0, 40.3], [0.0, 60.0, 29.6], [0.0, 0.0, 1.0]], np.float32)
#: (eye, roll): every camera looks at a point near the sphere
EYES = (((1.0, -0.6, 0.35), 0.3), ((-0.7, 0.8, 0.6), -0.5), ((0.2, -1.1, 0.5), 0.15))


def camera(i: int):
    """(K [3, 3], position [3], quaternion wxyz [4], depth [H, W]) of camera i, float32"""
    eye, roll = EYES[i]
    q = R.look_at(eye, (0.03, -0.02, -0.05), roll).astype(np.float32)
    pos = np.asarray(eye, np.float32)
    return K, pos, q, R.render_depth(K, pos, q, H, W)


def frame(*cams: int):
    """the cameras stacked: (depth [n, H, W], K [n, 3, 3], position [n, 3], quaternion [n, 4])"""
    ks, ps, qs, ds = zip(*(camera(i) for i in cams))
    return np.stack(ds), np.stack(ks), np.stack(ps), np.stack(qs)


#: the frames of the k = 3 run: two cameras in the second (the third camera serves the capture test)
FRAMES = ((0,), (0, 1), (1,))


def oracle_run(grid: "R.Grid", frames=FRAMES):
    """the oracle over the frames from an empty map.  Returns per frame (sure, possible, sw, w, updated, ambiguous) and the
    running ever-visible sets; the oracle integrates the SURE blocks of a frame."""
    n, v = grid.n_blocks, grid.bs ** 3
    sw, w = np.zeros((n, v), np.float16), np.zeros((n, v), np.float16)
    out = []
    for cams in frames:
        f = frame(*cams)
        sure, possible = R.mark_blocks(grid, *f)
        sw, w, upd, amb = R.integrate(grid, sw, w, sure, *f)
        out.append(dict(sure=sure, possible=possible, sw=sw, w=w, updated=upd, ambiguous=amb))
    return out
