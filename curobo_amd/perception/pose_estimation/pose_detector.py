"""``PoseDetector``: 6-DoF pose of a known mesh from a segmented point cloud, from scratch, by point-to-plane ICP with Huber
weights (reference pose_estimation/pose_detector.py): a coarse stage from ``n_rotation_samples`` random rotations, a fine
stage from the best of them.

The reference runs the hypotheses one after the other, about fifteen torch launches per iteration each.  Here every
hypothesis of a stage advances together, an iteration is two HIP launches (``csrc/pose_icp.hip``):
``curobo_hip_pose_icp_correspond`` (brute-force nearest neighbour and the sums of the normal equations) and
``curobo_hip_pose_icp_step`` (the 6 x 6 Cholesky solve and ``T <- T_update T``), all state on the device, sums in a fixed
order.  A stage -- its iterations, a last correspondence without a threshold for the error, and the choice of the best
hypothesis -- is recorded once per (hypotheses, mesh samples, observed points) as a graph, a plain chain of kernel nodes,
and replayed.

Deviations from the reference: the result is bit-identical from run to run for the same samples; the best hypothesis is
the lowest-index minimum of the errors; where the reference falls back to ``lstsq`` after a failed Cholesky factorisation,
the hypothesis stops where it is (``solver_failed`` in its state); only the Cholesky solver; nothing is printed.
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from ...backends import perception as B
from ...types import CameraObservation, Pose
from ...util.graph_capture import capture_graph
from .detection_result import DetectionResult
from .pose_detector_cfg import DetectorCfg
from .util import extract_observed_points, resample_points

#: fewer valid observed points than this cannot be aligned (pose_detector.py:114)
MINIMUM_POINTS = 10


class _Stage:
    """the device buffers of one (mode, H, M, O), and the graph recorded over them"""

    def __init__(self, mode: int, h: int, m: int, o: int, device: torch.device):
        f32 = dict(dtype=torch.float32, device=device)
        self.mode, self.h, self.m, self.o = mode, h, m, o
        self.mesh_points, self.mesh_normals = torch.zeros(m, 3, **f32), torch.zeros(m, 3, **f32)
        self.observed = torch.zeros(o, 3, **f32)
        self.state = torch.zeros(h, B.POSE_ICP_STATE_WORDS, **f32)
        self.workspace = torch.zeros(B.pose_icp_ws_bytes(h, m) // 4, **f32)
        self.best_index = torch.zeros(1, dtype=torch.int32, device=device)
        self.best_error = torch.zeros(1, **f32)
        self.best_transform = torch.zeros(12, **f32)
        self.graph: Optional[torch.cuda.CUDAGraph] = None

    def field(self, name: str) -> torch.Tensor:
        return B.pose_state_field(self.state, B.PoseICPState, name)


class PoseDetector:
    def __init__(self, geometry, config: Optional[DetectorCfg] = None):
        """``geometry``: anything with ``sample_surface_points(n) -> (points, normals)`` and ``get_dof()`` (``RobotMesh``)"""
        self.geometry = geometry
        self.config = config or DetectorCfg()
        self.device_cfg = self.config.device_cfg
        self.device = torch.device(self.device_cfg.device)
        self._stages: Dict[tuple, _Stage] = {}

    # ------------------------------------------------------------------------------------------------ the random parts
    def _resample(self, points: torch.Tensor, n: int) -> torch.Tensor:
        return resample_points(points, n)

    def _sample_rotations(self, n_samples: int) -> torch.Tensor:
        """[n_samples, 3, 3] uniform over SO(3): K. Shoemake, "Uniform random rotations", Graphics Gems III, 1992"""
        u = torch.rand(n_samples, 3, device=self.device, dtype=torch.float32)
        a, b = torch.sqrt(1 - u[:, 0]), torch.sqrt(u[:, 0])
        w, x = a * torch.sin(2 * torch.pi * u[:, 1]), a * torch.cos(2 * torch.pi * u[:, 1])
        y, z = b * torch.sin(2 * torch.pi * u[:, 2]), b * torch.cos(2 * torch.pi * u[:, 2])
        return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(n_samples, 3, 3)

    # ------------------------------------------------------------------------------------------------ launches
    def _iteration(self, st: _Stage, threshold: float) -> None:
        c = self.config
        B.pose_icp_correspond(st.workspace, st.mesh_points, st.mesh_normals, st.observed, st.state, threshold, c.use_huber_loss, c.huber_delta)
        B.pose_icp_step(st.state, st.workspace, st.m, st.mode)

    def _finish(self, st: _Stage) -> None:
        """the final error of every hypothesis, stopped or not, over all its samples (no threshold), and the best of them"""
        c = self.config
        B.pose_icp_correspond(st.workspace, st.mesh_points, st.mesh_normals, st.observed, st.state, math.inf, c.use_huber_loss, c.huber_delta,
                              honour_stopped=False)
        B.pose_icp_step(st.state, st.workspace, st.m, B.POSE_ICP_FINALIZE)
        B.pose_icp_select(st.best_index, st.state, st.best_error, st.best_transform)

    def _run_stage(self, mode: int, transforms: torch.Tensor, mesh: Tuple[torch.Tensor, torch.Tensor], observed: torch.Tensor,
                   n_iterations: int, threshold: float) -> Tuple[_Stage, Optional[List[torch.Tensor]]]:
        """``transforms`` [H, 4, 4]: the stage from these starts.  Returns its buffers (the states, the best index, error and
        transform) and, with ``save_iterations``, the best hypothesis's transform before and after every update."""
        c = self.config
        h, m, o = int(transforms.shape[0]), int(mesh[0].shape[0]), int(observed.shape[0])
        key = (mode, h, m, o, n_iterations, float(threshold), bool(c.use_huber_loss), float(c.huber_delta))
        st = self._stages.get(key)
        if st is None:
            st = self._stages[key] = _Stage(mode, h, m, o, self.device)
        # the buffers the graph was recorded over are rewritten in place
        st.mesh_points.copy_(mesh[0])
        st.mesh_normals.copy_(mesh[1])
        st.observed.copy_(observed)
        st.state.zero_()
        st.field("T").copy_(transforms[:, :3, :].reshape(h, 12))

        def body():
            for _ in range(n_iterations):
                self._iteration(st, threshold)
            self._finish(st)

        if not c.save_iterations:
            if st.graph is None:
                st.graph, _ = capture_graph(body, restore=(st.state,), device=self.device)
            st.graph.replay()
            return st, None
        after = [st.field("T").cpu().clone()]
        for _ in range(n_iterations):
            self._iteration(st, threshold)
            after.append(st.field("T").cpu().clone())
        self._finish(st)
        best = int(st.best_index.item())
        stopped, iterations = int(st.field("stopped")[best, 0]), int(st.field("iterations")[best, 0])
        bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]])
        history = [torch.cat([after[k][best].reshape(3, 4), bottom]) for k in range(iterations - stopped + 1)]
        return st, history

    # ------------------------------------------------------------------------------------------------ the reference's interface
    def detect(self, camera_obs: CameraObservation, config: Optional[torch.Tensor] = None) -> DetectionResult:
        return self.detect_from_points(self._extract_observed_points(camera_obs), config)

    def detect_from_points(self, observed_points: torch.Tensor, config: Optional[torch.Tensor] = None,
                           initial_pose: Optional[Pose] = None) -> DetectionResult:
        """observed_points [N, 3] in the world frame.  With ``initial_pose`` only the fine stage runs, from that pose; without,
        the coarse stage first.  ``config``: joint angles of an articulated geometry (ignored by a rigid one)."""
        observed_points = observed_points.to(device=self.device, dtype=torch.float32)
        observed_points = observed_points[torch.isfinite(observed_points).all(dim=1)]
        if len(observed_points) < MINIMUM_POINTS:
            raise ValueError(f"Not enough valid points: {len(observed_points)}")
        with torch.cuda.device(self.device):
            start_event, end_event = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start_event.record()
            if initial_pose is not None:
                T_start = initial_pose.get_matrix().reshape(-1, 4, 4)[:1].to(device=self.device, dtype=torch.float32)
                best_hypothesis, coarse_history = 0, []
            else:
                coarse, coarse_history = self._icp_coarse(observed_points, config)
                best_hypothesis = int(coarse.best_index.item())
                T_start = torch.eye(4, device=self.device, dtype=torch.float32).unsqueeze(0)
                T_start[0, :3, :] = coarse.best_transform.reshape(3, 4)
            fine, fine_history = self._icp_fine(T_start, observed_points, config)
            T_final = torch.eye(4, device=self.device, dtype=torch.float32)
            T_final[:3, :] = fine.best_transform.reshape(3, 4)
            error_final = float(fine.best_error.item())
            num_iters = int(fine.field("iterations")[0, 0])
            end_event.record()
            end_event.synchronize()
            compute_time = start_event.elapsed_time(end_event) / 1000.0
        result = DetectionResult(pose=Pose.from_matrix(T_final.unsqueeze(0)), config=config, confidence=1.0 - min(error_final / 0.1, 1.0),
                                 alignment_error=error_final, n_iterations=num_iters, compute_time=compute_time)
        save = self.config.save_iterations
        result.coarse_iterations = coarse_history if save else None
        result.fine_iterations = fine_history if save else None
        result.best_hypothesis = best_hypothesis
        return result

    def _extract_observed_points(self, camera_obs: CameraObservation) -> torch.Tensor:
        return extract_observed_points(camera_obs)

    def _icp_coarse(self, observed_points: torch.Tensor, config) -> Tuple[_Stage, Optional[List[torch.Tensor]]]:
        c = self.config
        observed = self._resample(observed_points, c.n_observed_points_coarse)
        if self.geometry.get_dof() > 0:
            self.geometry.update(config)
        mesh = self.geometry.sample_surface_points(c.n_mesh_points_coarse)
        rotations = self._sample_rotations(c.n_rotation_samples).to(device=self.device, dtype=torch.float32)
        transforms = torch.eye(4, device=self.device, dtype=torch.float32).repeat(len(rotations), 1, 1)
        transforms[:, :3, :3] = rotations
        transforms[:, :3, 3] = observed.mean(dim=0)  # every hypothesis starts at the cloud's centre
        return self._run_stage(B.POSE_ICP_COARSE, transforms, mesh, observed, c.n_iterations_coarse, c.distance_threshold_coarse)

    def _icp_fine(self, T_init: torch.Tensor, observed_points: torch.Tensor, config) -> Tuple[_Stage, Optional[List[torch.Tensor]]]:
        c = self.config
        observed = self._resample(observed_points, c.n_observed_points_fine)
        if self.geometry.get_dof() > 0:
            self.geometry.update(config)
        mesh = self.geometry.sample_surface_points(c.n_mesh_points_fine)
        return self._run_stage(B.POSE_ICP_FINE, T_init, mesh, observed, c.n_iterations_fine, c.distance_threshold_fine)
