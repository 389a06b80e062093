"""``CostSupportPolygon`` / ``ConvexPolygon2DHelper``: keep the centre of mass over the feet (reference
``cost/cost_support_polygon.py:17-109``, ``cost/cost_support_polygon_cfg.py:14-19``, ``geom/convex_polygon_helper.py:13-336``).

The reference builds its hulls in a Python loop with one torch op per vertex and differentiates the distance through ~25
elementwise launches; here the hull build is one launch (``convex_hull_2d_kernel``) plus one host read of the largest vertex
count, and the distance, the cost and its analytic gradient are one launch (``support_polygon_cost_kernel``).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from ..backends import cost as cost_hip
from ..hip_ops.cost import SupportPolygonCostFunction

#: the reference's constants: margin inside the hull that still costs (cost_support_polygon.py:95), soft-min length
#: (convex_polygon_helper.py:287), padding of the lazily built hull (cost_support_polygon.py:50)
MARGIN_TARGET, SMOOTHING, DEFAULT_PADDING = 0.1, 0.01, 0.05
#: most vertices a hull may have in the cost launch, most points the hull launch takes
MAX_HULL_VERTICES, MAX_HULL_POINTS = 32, 64


def convex_hulls(vertices: torch.Tensor, padding: Optional[float]):
    """vertices [N, n, 2] (3 <= n <= 64, on the GPU) -> (hulls [N, n, 2], counts [N] int32): one launch, no host read"""
    v = vertices.detach().to(torch.float32).contiguous()
    hulls, counts = torch.empty_like(v), torch.empty(v.shape[0], dtype=torch.int32, device=v.device)
    cost_hip.convex_hull_2d(hulls, counts, v, 0.0 if padding is None else float(padding))
    return hulls, counts


class ConvexPolygon2DHelper:
    """reference ``ConvexPolygon2DHelper``: ``build_convex_hull`` caches ``_cached_convex_hulls [N, max_count, 2]`` (rows past
    a hull's count repeat its last vertex), ``compute_point_hull_distance`` is the smooth signed distance to them (negative
    inside), differentiable in the points."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._cached_convex_hulls: Optional[torch.Tensor] = None
        self._cached_counts: Optional[torch.Tensor] = None
        self._one = torch.ones(1, device=self.device, dtype=torch.float32)

    def build_convex_hull(self, vertices: torch.Tensor, padding: Optional[float] = None) -> None:
        if vertices.dim() != 3 or vertices.shape[-1] != 2:
            raise ValueError(f"vertices must be (N, n_vertices, 2), got {tuple(vertices.shape)}")
        if vertices.shape[1] < 3:  # not enough points for a polygon: the reference returns them as they are
            self._cached_convex_hulls = vertices.detach().to(self.device, torch.float32).contiguous()
            self._cached_counts = None
            return
        hulls, counts = convex_hulls(vertices.to(self.device), padding)
        max_count = int(counts.max())  # the one host read, at build time (the reference's build is a host loop)
        self._cached_convex_hulls = hulls[:, :max_count].contiguous()
        self._cached_counts = counts

    def compute_point_hull_distance(self, points: torch.Tensor, idxs_batch: torch.Tensor) -> torch.Tensor:
        """points [B, H, n_points, 2], idxs_batch [B] -> signed distance [B, H, n_points] to hull ``idxs_batch[b]``"""
        if self._cached_convex_hulls is None:
            return torch.zeros_like(points[..., 0])
        B, H, P, _ = points.shape
        flat = points.reshape(B, H * P, 2)
        z = lambda *s: torch.empty(*s, device=points.device, dtype=torch.float32)  # noqa: E731
        sd = SupportPolygonCostFunction.apply(
            flat, self._cached_convex_hulls, None, idxs_batch.to(torch.int32).contiguous(), self._one, 0.0, MARGIN_TARGET,
            SMOOTHING, z(B, H * P), z(B, H * P, 4), None, True, 1)
        return sd.view(B, H, P)


@dataclass
class CostSupportPolygonCfg:  # reference CostSupportPolygonCfg
    weight: float = 1.0
    foot_sphere_indices: Optional[torch.Tensor] = None
    foot_link_names: Optional[List[str]] = None
    inside_cost_weight: float = 0.001  # a small pull towards the middle while inside
    use_grad_input: bool = True


class CostSupportPolygon:
    """``forward(robot_com[B,H,3|4], robot_spheres[B,H,S,4]) -> cost[B,H]``: ``weight`` x (the signed distance of the centre
    of mass' xy to the hull of the foot spheres outside it, ``inside_cost_weight * max(0.1 + distance, 0)`` inside).  The hull
    is built from horizon step 0 of the first call (padding 0.05) unless ``build_convex_hull`` was called; row b uses hull b
    (one hull: every row uses it)."""

    def __init__(self, config: CostSupportPolygonCfg, device="cuda"):
        self.config, self.device = config, torch.device(device)
        self._weight = torch.tensor([config.weight], device=self.device, dtype=torch.float32)
        self._polygon_helper = ConvexPolygon2DHelper(self.device)
        self._shape = None

    def build_convex_hull(self, vertices: torch.Tensor, padding: Optional[float] = None) -> None:
        self._polygon_helper.build_convex_hull(vertices, padding)

    def setup_batch_tensors(self, batch_size: int, horizon: int) -> None:
        if self._shape == (batch_size, horizon):
            return
        d = self.device
        self._out_cost, self._out_grad = torch.zeros(batch_size, horizon, device=d), torch.zeros(batch_size, horizon, 4, device=d)
        self._out_distance = torch.zeros(batch_size, horizon, device=d)
        self._idxs = torch.arange(batch_size, device=d, dtype=torch.int32)
        self._idx0 = torch.zeros(batch_size, device=d, dtype=torch.int32)
        self._shape = (batch_size, horizon)

    @property
    def signed_distance(self) -> torch.Tensor:
        """[B, H] of the last ``forward``: negative inside the hull"""
        return self._out_distance

    def forward(self, robot_com: torch.Tensor, robot_spheres: torch.Tensor) -> torch.Tensor:
        B, H = int(robot_com.shape[0]), int(robot_com.shape[1])
        self.setup_batch_tensors(B, H)
        h = self._polygon_helper
        if h._cached_convex_hulls is None:
            if self.config.foot_sphere_indices is None:
                raise ValueError("CostSupportPolygon: foot_sphere_indices is not set and no hull was built")
            feet = robot_spheres[:, :, self.config.foot_sphere_indices, :2].detach()
            self.build_convex_hull(feet[:, 0, :, :], padding=DEFAULT_PADDING)
        n_hulls = int(h._cached_convex_hulls.shape[0])
        if n_hulls not in (1, B):
            raise ValueError(f"CostSupportPolygon: {n_hulls} hulls for a batch of {B} (one per row, or one for all)")
        return SupportPolygonCostFunction.apply(
            robot_com, h._cached_convex_hulls, None, self._idxs if n_hulls == B else self._idx0, self._weight,
            float(self.config.inside_cost_weight), MARGIN_TARGET, SMOOTHING, self._out_cost, self._out_grad,
            self._out_distance, self.config.use_grad_input, 0)

    __call__ = forward

    def update_weight(self, weight: float) -> None:
        self._weight.fill_(weight)
