"""``BlockSparseRaycastPoseRefiner``: align a new depth image to the map the mapper already holds, KinectFusion-style camera
tracking (reference ``perception/mapper/pose_refiner.py``).

Every sampled pixel is pushed out along its ray to the observed range; the TSDF read there, and at ``n_samples_per_ray`` points
a voxel apart around it, should be 0, +-voxel_size, ...  Levenberg-Marquardt over the camera pose drives the difference to zero.
An iteration is two HIP launches: ``curobo_hip_mapper_ray_align`` at the candidate pose (``csrc/mapper_raycast.hip``), then
``curobo_hip_pose_lm_step``, the same trust-region step ``SDFPoseDetector`` takes -- the reference's refiner calls the same three
functions of ``optim_pose_lm.py`` as its detector.  All state stays on the device and the sums are added in a fixed order, so the
result is bit-identical from run to run (the reference's, which adds with atomics, is not).

``refine_pose`` evaluates the estimate once (the step's INIT mode), then replays ``outer_iterations`` times one recorded block of
``inner_iterations`` iterations: a plain chain of kernel nodes.  Depth and intrinsics are copied into buffers the recorded launches
read, so one graph per image shape serves every call."""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from ...backends import mapper as B
from ...backends import perception as P
from ...types import Pose
from ...util.graph_capture import capture_graph
from .renderer import intrinsics_matrix


@dataclass
class BlockSparseRaycastRefinerCfg:
    """the reference's fields and defaults (pose_refiner.py:167-216).  ``tile_block_dim`` is carried for the interface: a row of
    partial sums belongs to a workgroup of 256 samples."""

    n_points: int = (1280 * 720) // 10
    minimum_valid_depth_pixels: int = 100
    max_iterations: int = 100
    inner_iterations: int = 4
    distance_threshold: float = 0.1
    min_valid_ratio: float = 0.1
    n_samples_per_ray: int = 1
    tile_block_dim: int = 256
    depth_minimum_distance: float = 0.1
    depth_maximum_distance: float = 10.0
    minimum_tsdf_weight: float = 2.0
    lambda_initial: float = 1e-3
    lambda_factor: float = 10.0
    lambda_min: float = 1e-7
    lambda_max: float = 1e7
    rho_min: float = 0.25

    @property
    def outer_iterations(self) -> int:
        return self.max_iterations // self.inner_iterations

    def stride(self, height: int, width: int) -> int:
        """every ``stride``-th pixel along both axes is sampled (pose_refiner.py:342)"""
        return max(1, int(math.sqrt(height * width / self.n_points)))


class _Run:
    """the device buffers of one image shape, and the graph recorded over them"""

    def __init__(self, height: int, width: int, cfg: BlockSparseRaycastRefinerCfg, device: torch.device):
        self.shape = (height, width)
        self.stride = cfg.stride(height, width)
        self.n_samples = B.ray_align_samples(self.shape, self.stride, cfg.n_samples_per_ray)
        self.depth = torch.zeros(height, width, dtype=torch.float32, device=device)
        self.intrinsics = torch.zeros(3, 3, dtype=torch.float32, device=device)
        self.state = torch.zeros(P.POSE_STATE_WORDS, dtype=torch.float32, device=device)
        self.workspace = torch.zeros(P.pose_sdf_ws_bytes(self.n_samples) // 4, dtype=torch.float32, device=device)
        self.graph: Optional[torch.cuda.CUDAGraph] = None

    def field(self, name: str) -> torch.Tensor:
        return P.pose_state_field(self.state, P.PoseLMState, name)


class BlockSparseRaycastPoseRefiner:
    """``BlockSparseRaycastPoseRefiner(mapper)``; ``refine_pose(depth, intrinsics, estimated_pose)`` before ``mapper.integrate``.

    The refiner reads voxels whose weight is at least ITS ``minimum_tsdf_weight`` (the reference's default 2.0), not the mapper's."""

    def __init__(self, mapper, config: Optional[BlockSparseRaycastRefinerCfg] = None, use_graph: bool = True):
        self.mapper = mapper
        self.config = config or BlockSparseRaycastRefinerCfg()
        c = self.config
        if c.n_samples_per_ray < 1 or c.n_samples_per_ray > 9 or c.n_samples_per_ray % 2 == 0:
            raise ValueError(f"n_samples_per_ray must be odd and in 1..9, got {c.n_samples_per_ray}")
        if c.inner_iterations < 1 or c.n_points < 1:
            raise ValueError(f"inner_iterations and n_points must be positive, got {c.inner_iterations} and {c.n_points}")
        self.device = torch.device(mapper.config.device)
        self._use_graph = bool(use_graph)
        self._runs: Dict[Tuple[int, int], _Run] = {}

    # ------------------------------------------------------------------------------------------------ launches
    def _evaluate(self, run: _Run) -> None:
        c, t = self.config, self.mapper.tsdf
        B.mapper_ray_align(run.workspace, run.depth, run.intrinsics, run.field("cand_position"), run.field("cand_quaternion"), t.block_data,
                           t.block_visible, t.params, c.minimum_tsdf_weight, c.depth_minimum_distance, c.depth_maximum_distance,
                           c.distance_threshold, run.stride, c.n_samples_per_ray)

    def _step(self, run: _Run, mode: int) -> None:
        c = self.config
        # minimum_valid_count: the reference passes minimum_valid_depth_pixels (pose_refiner.py:548)
        P.pose_lm_step(run.state, run.workspace, run.n_samples, mode, c.lambda_initial, c.lambda_factor, c.lambda_min, c.lambda_max, c.rho_min,
                       c.minimum_valid_depth_pixels)

    def _refine_inner_iterations(self, run: _Run) -> None:
        for _ in range(self.config.inner_iterations):
            self._evaluate(run)
            self._step(run, P.POSE_LM_UPDATE)

    def _run_block(self, run: _Run) -> None:
        if not self._use_graph:
            self._refine_inner_iterations(run)
            return
        if run.graph is None:
            run.graph, _ = capture_graph(lambda: self._refine_inner_iterations(run), restore=(run.state,), device=self.device)
        run.graph.replay()

    # ------------------------------------------------------------------------------------------------ the reference's interface
    def refine_pose(self, depth: torch.Tensor, intrinsics: torch.Tensor, estimated_pose: Pose) -> Tuple[Pose, float, int]:
        """``depth`` [H, W] metres along the camera's axis, ``intrinsics`` [3, 3] (or [fx, fy, cx, cy]), ``estimated_pose`` the
        camera in the world.  Returns ``(refined pose, final_error, n_iterations)``: the RMS residual at the refined pose (``inf``
        where it has no valid sample) and ``outer_iterations * inner_iterations``; ``(estimated_pose, inf, 0)`` when fewer than
        ``minimum_valid_depth_pixels`` pixels hold a depth inside the configured range."""
        c = self.config
        if depth.dim() != 2:
            raise ValueError(f"depth must be (H, W), got {tuple(depth.shape)}")
        k = intrinsics_matrix(intrinsics)
        depth = depth.to(self.device, torch.float32)
        n_valid_depth = int(torch.logical_and(depth > c.depth_minimum_distance, depth < c.depth_maximum_distance).sum().item())
        if n_valid_depth < c.minimum_valid_depth_pixels:
            return estimated_pose, float("inf"), 0
        shape = (int(depth.shape[0]), int(depth.shape[1]))
        with torch.cuda.device(self.device):
            run = self._runs.get(shape)
            if run is None:
                run = self._runs[shape] = _Run(*shape, c, self.device)
            # the buffers the graph was recorded over are rewritten in place
            run.depth.copy_(depth)
            run.intrinsics.copy_(k.to(self.device))
            run.state.zero_()
            run.field("cand_position").copy_(estimated_pose.position.reshape(-1, 3)[0].to(self.device, torch.float32))
            run.field("cand_quaternion").copy_(estimated_pose.quaternion.reshape(-1, 4)[0].to(self.device, torch.float32))
            self._evaluate(run)
            self._step(run, P.POSE_LM_INIT)
            for _ in range(c.outer_iterations):
                self._run_block(run)
            state = run.state.cpu()
        best_n_valid = int(state[P.pose_state_slice("best_n_valid")].view(torch.int32)[0])
        # the reference's initial error is inf without a valid sample (pose_refiner.py:406-410); the step's INIT mode alone gives 0
        error = float(state[P.pose_state_slice("best_error")][0]) if best_n_valid > 0 else float("inf")
        pose = Pose(run.field("best_position").clone().view(1, 3), run.field("best_quaternion").clone().view(1, 4))
        return pose, error, c.outer_iterations * c.inner_iterations
