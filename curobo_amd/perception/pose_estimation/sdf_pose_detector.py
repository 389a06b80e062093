"""``SDFPoseDetector``: 6-DoF pose refinement of a known mesh against a segmented point cloud by Levenberg-Marquardt over
unsigned mesh distances (reference pose_estimation/sdf_pose_detector.py).

The reference spends two Warp launches and about forty torch launches per iteration and sums with float atomics.  Here an
iteration is two HIP launches (``csrc/pose_detect.hip``): ``curobo_hip_pose_sdf_evaluate`` at the candidate pose, then
``curobo_hip_pose_lm_step`` (trust-region update, Cholesky step, next candidate), all state on the device, sums in a fixed
order.  ``inner_iterations`` iterations form one block, recorded once per point count as a graph -- a plain chain of kernel
nodes -- and replayed; after each block the two change vectors are read back for the convergence test, as the reference's
outer loop does.

Deviations from the reference: the result is bit-identical from run to run (the reference's is not); only rigid meshes;
``rho_min`` is carried and, as in the reference's ``trust_region_update``, never consulted (a step is accepted when its
trust ratio is >= 0 and more than 10 points are valid).
"""

from __future__ import annotations

from typing import Dict, Optional

import torch

from ...backends import perception as B
from ...types import CameraObservation, Pose
from ...util.graph_capture import capture_graph
from .detection_result import DetectionResult
from .mesh_robot import RobotMesh
from .sdf_pose_detector_cfg import SDFDetectorCfg
from .util import extract_observed_points

#: ``minimum_valid_count`` of the reference's ``trust_region_update``
MINIMUM_VALID_COUNT = 10


class _Run:
    """the device buffers of one point count, and the graph recorded over them"""

    def __init__(self, n: int, device: torch.device):
        self.n = n
        self.points = torch.zeros(n, 3, dtype=torch.float32, device=device)
        self.state = torch.zeros(B.POSE_STATE_WORDS, dtype=torch.float32, device=device)
        self.workspace = torch.zeros(B.pose_sdf_ws_bytes(n) // 4, dtype=torch.float32, device=device)
        self.graph: Optional[torch.cuda.CUDAGraph] = None

    def field(self, name: str) -> torch.Tensor:
        return B.pose_state_field(self.state, B.PoseLMState, name)


class SDFPoseDetector:
    def __init__(self, robot_mesh: RobotMesh, config: Optional[SDFDetectorCfg] = None):
        self.robot_mesh = robot_mesh
        self.config = config or SDFDetectorCfg()
        self.device = torch.device(robot_mesh.device)
        self._runs: Dict[int, _Run] = {}

    # ------------------------------------------------------------------------------------------------ launches
    def _evaluate(self, run: _Run) -> None:
        c = self.config
        B.pose_sdf_evaluate(run.workspace, run.points, run.field("cand_position"), run.field("cand_quaternion"),
                            self.robot_mesh.device_mesh.struct, c.max_distance, c.distance_threshold, c.use_huber, c.huber_delta)

    def _step(self, run: _Run, mode: int) -> None:
        c = self.config
        B.pose_lm_step(run.state, run.workspace, run.n, mode, c.lambda_initial, c.lambda_factor, c.lambda_min, c.lambda_max, c.rho_min,
                       MINIMUM_VALID_COUNT)

    def _refine_inner_iterations(self, run: _Run) -> None:
        for _ in range(self.config.inner_iterations):
            self._evaluate(run)
            self._step(run, B.POSE_LM_UPDATE)

    def _run_block(self, run: _Run) -> None:
        if not self.config.use_cuda_graph:
            self._refine_inner_iterations(run)
            return
        if run.graph is None:
            run.graph, _ = capture_graph(lambda: self._refine_inner_iterations(run), restore=(run.state,), device=self.device)
        run.graph.replay()

    # ------------------------------------------------------------------------------------------------ the reference's interface
    def detect(self, camera_obs: CameraObservation, config: Optional[torch.Tensor] = None, initial_pose: Optional[Pose] = None) -> DetectionResult:
        return self.detect_from_points(self._extract_observed_points(camera_obs), config, initial_pose)

    def detect_from_points(self, observed_points: torch.Tensor, config: Optional[torch.Tensor] = None,
                           initial_pose: Optional[Pose] = None) -> DetectionResult:
        """observed_points [N, 3] in the world frame, ``initial_pose`` the rough pose of the mesh (required: there is no random
        sampling); ``config`` (joint angles of an articulated mesh) must be None."""
        if initial_pose is None:
            raise ValueError("SDFPoseDetector requires an initial_pose estimate")
        if config is not None:
            self.robot_mesh.update(config)
        cfg = self.config
        points = observed_points.to(device=self.device, dtype=torch.float32)
        if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] == 0:
            raise ValueError(f"observed_points must be (N, 3) with N >= 1, got {tuple(points.shape)}")
        with torch.cuda.device(self.device):
            start_event, end_event = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start_event.record()
            if len(points) > cfg.n_points:
                indices = torch.randperm(len(points), device=self.device)[: cfg.n_points]
                points = points[indices]
            n = int(points.shape[0])
            run = self._runs.get(n)
            if run is None:
                run = self._runs[n] = _Run(n, self.device)
            # _setup_refinement: the buffers the graph was recorded over are rewritten in place
            run.points.copy_(points)
            run.state.zero_()
            run.field("cand_position").copy_(initial_pose.position.reshape(-1, 3)[0].to(self.device, torch.float32))
            run.field("cand_quaternion").copy_(initial_pose.quaternion.reshape(-1, 4)[0].to(self.device, torch.float32))
            self._evaluate(run)
            self._step(run, B.POSE_LM_INIT)
            n_iterations = 0
            for outer_i in range(cfg.max_iterations // cfg.inner_iterations):
                self._run_block(run)
                n_iterations = (outer_i + 1) * cfg.inner_iterations
                delta = run.field("delta").cpu()
                if float(delta[:3].norm()) < cfg.convergence_threshold and float(delta[3:].norm()) < cfg.rotation_convergence_threshold:
                    break
            state = run.state.cpu()
            final_pose = Pose(run.field("best_position").clone().unsqueeze(0), run.field("best_quaternion").clone().unsqueeze(0))
            best_n_valid = int(state[B.pose_state_slice("best_n_valid")].view(torch.int32)[0])
            confidence = min(1.0, (best_n_valid / n) / cfg.min_valid_ratio)
            end_event.record()
            end_event.synchronize()
            compute_time = start_event.elapsed_time(end_event) / 1000.0
        return DetectionResult(pose=final_pose, config=config, confidence=confidence,
                               alignment_error=float(state[B.pose_state_slice("best_error")][0]), n_iterations=n_iterations,
                               compute_time=compute_time)

    def _extract_observed_points(self, camera_obs: CameraObservation) -> torch.Tensor:
        return extract_observed_points(camera_obs)
