"""``RobotMesh``: the mesh a pose detector aligns to (reference pose_estimation/mesh_robot.py), rigid meshes only."""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from ...backends.mesh import DeviceMesh, build_mesh_bvh

_NOT_PACKAGED = ("articulated meshes are not packaged: the robot models of this library carry collision spheres, not link "
                 "meshes; build a rigid RobotMesh from vertices and faces")


class RobotMesh:
    """A rigid triangle mesh on the device, queried through the linear BVH of ``backends.mesh.build_mesh_bvh`` (no cell
    lists: the detector walks the tree)."""

    def __init__(self, vertices, faces, device="cuda:0"):
        v = vertices.detach().cpu().numpy() if torch.is_tensor(vertices) else np.asarray(vertices)
        f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0:
            raise ValueError(f"RobotMesh needs vertices [V, 3] and faces [F, 3], got {v.shape} and {f.shape}")
        self.device = torch.device(device)
        self.vertices = torch.as_tensor(v).to(self.device)
        self.faces = torch.as_tensor(f).to(self.device)
        self._host = (v, f)
        self._mesh: Optional[DeviceMesh] = None  # built at its first use: the members above need no GPU
        self._sample_cache: dict = {}  # n_points -> (face indices [n], barycentrics [n, 3])

    @classmethod
    def from_trimesh(cls, mesh, device="cuda:0") -> "RobotMesh":
        """anything with ``.vertices`` [V, 3] and ``.faces`` [F, 3] (a ``trimesh.Trimesh``)"""
        return cls(np.asarray(mesh.vertices), np.asarray(mesh.faces), device=device)

    @classmethod
    def from_kinematics(cls, *args, **kwargs):
        raise NotImplementedError(_NOT_PACKAGED)

    def update(self, joint_angles=None):
        raise NotImplementedError(_NOT_PACKAGED)

    @property
    def device_mesh(self) -> DeviceMesh:
        if self._mesh is None:
            self._mesh = build_mesh_bvh(self._host[0], self._host[1], self.device, cells=False)
        return self._mesh

    def sample_surface_points(self, n_points: int, resample: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """(points [n_points, 3], unit normals [n_points, 3]) on the surface, uniform by area (reference mesh_robot.py:334-413):
        the faces and barycentrics are drawn once per ``n_points`` and kept (a detector asks for its coarse and its fine count
        in turn); ``resample=True`` draws them again"""
        if n_points not in self._sample_cache or resample:
            self._sample_cache[n_points] = self._generate_sample_cache(n_points)
        face_idx, bary = self._sample_cache[n_points]
        faces = self.faces.long()
        v0, v1, v2 = self.vertices[faces[face_idx, 0]], self.vertices[faces[face_idx, 1]], self.vertices[faces[face_idx, 2]]
        points = bary[:, 0:1] * v0 + bary[:, 1:2] * v1 + bary[:, 2:3] * v2
        normals = torch.cross(v1 - v0, v2 - v0, dim=1)
        normals = normals / (torch.norm(normals, dim=1, keepdim=True) + 1e-8)
        return points, normals

    def _generate_sample_cache(self, n_points: int) -> Tuple[torch.Tensor, torch.Tensor]:
        faces = self.faces.long()
        v0, v1, v2 = self.vertices[faces[:, 0]], self.vertices[faces[:, 1]], self.vertices[faces[:, 2]]
        areas = 0.5 * torch.norm(torch.cross(v1 - v0, v2 - v0, dim=1), dim=1)
        face_indices = torch.multinomial(areas / (areas.sum() + 1e-8), n_points, replacement=True)
        r1 = torch.sqrt(torch.rand(n_points, device=self.device))  # the root makes the density uniform over the triangle
        r2 = torch.rand(n_points, device=self.device)
        return face_indices, torch.stack([1 - r1, r1 * (1 - r2), r1 * r2], dim=1)

    @property
    def n_vertices(self) -> int:
        return int(self.vertices.shape[0])

    @property
    def n_faces(self) -> int:
        return int(self.faces.shape[0])

    @property
    def is_articulated(self) -> bool:
        return False

    def get_dof(self) -> int:
        return 0
