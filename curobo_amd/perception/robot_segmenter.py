"""Robot segmentation from depth images (reference ``curobo/_src/perception/robot_segmenter.py``): forward kinematics
gives the robot's collision spheres, one HIP launch turns depth x projection rays x camera pose x spheres into the mask
of the robot's pixels and the depth image without them.  The reference's eager chain writes a pixels x spheres distance
tensor on the way; here that tensor never exists."""

from __future__ import annotations

import copy
from typing import Dict, Optional, Tuple, Union

import torch

from ..backends import perception as _backend
from ..util.cv import get_projection_rays, project_depth_using_rays
from ..util.graph_capture import capture_graph


class RobotSegmenter:
    """``mask, depth_without_robot = segmenter.get_robot_mask(camera_obs, joint_state)``.  A pixel is masked when its depth is
    positive and its point lies within ``distance_threshold`` of a collision sphere (disabled spheres, radius < 0, mask
    nothing).  ``ops_dtype``: ``torch.bfloat16`` (the reference's default: depth, rays, spheres and the depth x ray product
    rounded to bf16, the rest fp32) or ``torch.float32``."""

    def __init__(self, kinematics, distance_threshold: float = 0.05, use_cuda_graph: bool = True,
                 ops_dtype: torch.dtype = torch.bfloat16):
        if ops_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"ops_dtype must be torch.bfloat16 or torch.float32, got {ops_dtype}")
        self._kinematics = kinematics
        self._projection_rays: Optional[torch.Tensor] = None
        self.ready = False
        self.distance_threshold = distance_threshold
        self._ops_dtype = ops_dtype
        self._use_cuda_graph = use_cuda_graph
        self._graph = None  # (graph, static inputs, static outputs, shapes) once captured

    @staticmethod
    def from_robot_file(robot_file: Union[str, Dict], collision_sphere_buffer: Optional[float] = None,
                        distance_threshold: float = 0.05, use_cuda_graph: bool = True, device_cfg=None) -> "RobotSegmenter":
        """``robot_file``: the name of a packaged robot (``"franka"``, also as ``"franka.yml"``) or a robot configuration
        dictionary (``KinematicsCfg.from_data_dict``); ``collision_sphere_buffer`` is added to every sphere radius"""
        from ..kinematics import Kinematics, KinematicsCfg

        device = device_cfg.device if device_cfg is not None else "cuda:0"
        if isinstance(robot_file, str):
            name = robot_file[: -len(".yml")] if robot_file.endswith(".yml") else robot_file
            cfg = KinematicsCfg.from_packaged(name, device=device)
            if collision_sphere_buffer is not None:
                r = cfg.kinematics_config.link_spheres[..., 3]
                r[r >= 0] += float(collision_sphere_buffer)  # (disabled spheres stay disabled)
        elif isinstance(robot_file, dict):
            robot_file = copy.deepcopy(robot_file)
            if collision_sphere_buffer is not None:
                sect = robot_file.get("robot_cfg", robot_file)
                sect.get("kinematics", sect)["collision_sphere_buffer"] = collision_sphere_buffer
            cfg = KinematicsCfg.from_data_dict(robot_file, device=device)
        else:
            raise ValueError("robot_file must be a string path or dict")
        return RobotSegmenter(Kinematics(cfg), distance_threshold=distance_threshold, use_cuda_graph=use_cuda_graph)

    # ------------------------------------------------------------------ camera
    def update_camera_projection(self, camera_obs) -> None:
        """projection rays of the observation's intrinsics and image size, kept for every later call (in place: a captured
        graph sees new intrinsics of the same batch)"""
        intrinsics = camera_obs.intrinsics
        if intrinsics.dim() == 2:
            intrinsics = intrinsics.unsqueeze(0)
        rays = get_projection_rays(camera_obs.depth_image.shape[-2], camera_obs.depth_image.shape[-1], intrinsics,
                                   camera_obs.depth_to_meter).contiguous()
        if self._projection_rays is None or self._projection_rays.shape != rays.shape:
            self._projection_rays = rays
            self._graph = None
        else:
            self._projection_rays.copy_(rays)
        self.ready = True

    def get_pointcloud_from_depth(self, camera_obs) -> torch.Tensor:
        """points (B, H W, 3) in the camera frame, in ``ops_dtype``"""
        if self._projection_rays is None:
            self.update_camera_projection(camera_obs)
        depth = camera_obs.depth_image.to(dtype=self._ops_dtype)
        if depth.dim() == 2:
            depth = depth.unsqueeze(0)
        return project_depth_using_rays(depth, self._projection_rays.to(dtype=self._ops_dtype))

    # ------------------------------------------------------------------ mask
    def get_robot_mask(self, camera_obs, joint_state) -> Tuple[torch.Tensor, torch.Tensor]:
        """one robot, a batch of depth images (B, H, W) with one camera pose each (or one for all)"""
        if camera_obs.depth_image.dim() != 3:
            raise ValueError("Send depth image as (batch, height, width)")
        return self.get_robot_mask_from_active_js(camera_obs, self._kinematics.get_active_js(joint_state))

    def get_robot_mask_from_active_js(self, camera_obs, active_joint_state) -> Tuple[torch.Tensor, torch.Tensor]:
        q = active_joint_state.position
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if self._projection_rays is None:
            self.update_camera_projection(camera_obs)
        depth = camera_obs.depth_image
        pos, quat = camera_obs.pose.position.reshape(-1, 3), camera_obs.pose.quaternion.reshape(-1, 4)
        if not self._use_cuda_graph:
            mask, out = self._mask_op(depth.contiguous(), pos.contiguous(), quat.contiguous(), q)
            return mask, out
        shapes = (tuple(depth.shape), tuple(pos.shape), tuple(q.shape), depth.device)
        if self._graph is None or self._graph[3] != shapes:
            static = (depth.clone().contiguous(), pos.clone().contiguous(), quat.clone().contiguous(), q.clone().contiguous())
            with torch.cuda.device(depth.device):
                graph, outs = capture_graph(lambda: self._mask_op(*static), device=depth.device)
            self._graph = (graph, static, outs, shapes)
        graph, static, outs, _ = self._graph
        for dst, src in zip(static, (depth, pos, quat, q)):
            dst.copy_(src)
        graph.replay()
        return outs[0].clone(), outs[1].clone()  # (the graph's own buffers are overwritten by the next call)

    def _mask_op(self, depth: torch.Tensor, pos: torch.Tensor, quat: torch.Tensor, q: torch.Tensor):
        """FK + the mask launch (what a captured graph replays: one chain of launches)"""
        spheres = self._kinematics.compute_kinematics(q).robot_spheres
        spheres = spheres.reshape(spheres.shape[0], -1, 4)
        if spheres.shape[0] != 1 and spheres.shape[0] != depth.shape[0]:
            raise ValueError(f"robot_spheres batch must be 1 or match points batch: got {spheres.shape[0]} vs {depth.shape[0]}")
        mask = torch.empty(depth.shape, dtype=torch.uint8, device=depth.device)
        out = torch.empty_like(depth)
        _backend.robot_mask(mask, out, depth, self._projection_rays, pos, quat, spheres.contiguous(), self.distance_threshold,
                            _backend.MASK_BF16_OPS if self._ops_dtype == torch.bfloat16 else _backend.MASK_FP32)
        return mask.bool(), out

    @property
    def kinematics(self):
        return self._kinematics

    @property
    def base_link(self) -> str:
        return self._kinematics.base_link
