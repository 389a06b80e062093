"""``RobotBuilder``: a robot configuration from a URDF and collision spheres -- counterpart of the reference's
``curobo.robot_builder.RobotBuilder`` (``curobo/_src/robot/builder/builder_robot.py:41-1172``) where this library can honour
it: the self-collision matrix (``compute_collision_matrix``, on the GPU through ``collision_matrix.py``), manual ignores, and
the ``kinematics`` dictionary / YAML file that ``KinematicsCfg.from_data_dict`` and ``load_robot_model`` read.  Collision spheres
come from the user or an XRDF (``set_collision_spheres``): fitting them to meshes, the viewer and the XRDF writer are absent and
say so."""

from __future__ import annotations

import copy
import os
from typing import Dict, List, Optional, Union

from .collision_matrix import SelfCollisionMatrix, compute_self_collision_matrix, neighbor_ignore
from .loader import build_robot_model
from .urdf import load_urdf

#: keys of a ``kinematics`` dictionary that the builder owns; every other key of a loaded configuration (``lock_joints``,
#: ``extra_links``, ``collision_sphere_buffer`` ...) is carried through ``build()`` unchanged
_OWNED = ("urdf_path", "asset_root_path", "base_link", "tool_frames", "collision_link_names", "collision_spheres",
          "self_collision_ignore", "self_collision_buffer", "cspace", "mesh_link_names")


class RobotBuilder:
    def __init__(self, urdf_path: str, asset_path: str = "", tool_frames: Optional[List[str]] = None, device="cuda:0"):
        """``urdf_path``: the URDF file; ``asset_path``: its mesh directory (recorded as ``asset_root_path``, not read);
        ``tool_frames``: default the last link of the URDF; ``device``: where ``compute_collision_matrix`` runs."""
        self.urdf_path = os.path.abspath(urdf_path)
        self.asset_path = os.path.abspath(asset_path) if asset_path else ""
        self.device = device
        self._urdf = load_urdf(self.urdf_path)
        self._link_names = list(self._urdf.links.keys())
        children = {j.child for j in self._urdf.joints.values()}
        self._base_link = next(name for name in self._link_names if name not in children)  # root of the tree
        self._tool_frames = list(tool_frames) if tool_frames else self._link_names[-1:]
        self._collision_spheres: Optional[Dict[str, List[Dict]]] = None
        self._self_collision_ignore: Optional[Dict[str, List[str]]] = None
        self._self_collision_buffer: Dict[str, float] = {}
        self._cspace_config: Optional[Dict] = None
        self._passthrough: Dict = {}
        self._matrix: Optional[SelfCollisionMatrix] = None

    @classmethod
    def from_config(cls, config: Union[str, Dict], assets_root: str = "", device="cuda:0") -> "RobotBuilder":
        """An existing robot configuration (a YAML path or its dictionary, with or without the ``robot_cfg`` / ``kinematics``
        levels) for editing: ``collision_spheres``, ``self_collision_ignore``, ``self_collision_buffer`` and ``cspace`` are taken
        over (reference ``from_config``, :169-233).  ``urdf_path`` is relative to ``assets_root``, or absolute."""
        if isinstance(config, str):
            import yaml

            with open(config) as fh:
                config = yaml.safe_load(fh)
        data = copy.deepcopy(config)
        data = data.get("robot_cfg", data)
        data = data.get("kinematics", data)
        asset = data.get("asset_root_path") or ""
        b = cls(os.path.join(assets_root, data["urdf_path"]), os.path.join(assets_root, asset) if asset else "",
                data.get("tool_frames"), device)
        if data.get("base_link"):
            b._base_link = data["base_link"]
        if isinstance(data.get("collision_spheres"), str):
            raise ValueError("collision_spheres must be inline in the robot configuration")
        if data.get("collision_spheres") is not None:
            b._collision_spheres = data["collision_spheres"]
        if data.get("self_collision_ignore") is not None:
            b._self_collision_ignore = data["self_collision_ignore"]
        if data.get("self_collision_buffer") is not None:
            b._self_collision_buffer = data["self_collision_buffer"]
        if data.get("cspace") is not None:
            b._cspace_config = data["cspace"]
        b._passthrough = {k: v for k, v in data.items() if k not in _OWNED}
        return b

    # ---- collision spheres
    def set_collision_spheres(self, spheres: Dict[str, List[Dict]]) -> None:
        """``{link: [{"center": [x, y, z], "radius": r}, ...]}`` in the link frames, as a robot file or an XRDF lists them"""
        unknown = [k for k in spheres if k not in self._urdf.links and k not in (self._passthrough.get("extra_links") or {})]
        if unknown:
            raise ValueError(f"collision spheres given for links the URDF does not have: {unknown}")
        self._collision_spheres = {k: [{"center": [float(x) for x in s["center"]], "radius": float(s["radius"])} for s in v]
                                   for k, v in spheres.items()}
        self._matrix = None

    def fit_collision_spheres(self, *args, **kwargs):
        raise NotImplementedError("fit_collision_spheres needs mesh sphere fitting, which this library does not have: give the spheres "
                                  "with set_collision_spheres (from a robot file or an XRDF)")

    def refit_link_spheres(self, *args, **kwargs):
        raise NotImplementedError("refit_link_spheres needs mesh sphere fitting, which this library does not have: give the spheres "
                                  "with set_collision_spheres (from a robot file or an XRDF)")

    def visualize(self, *args, **kwargs):
        raise NotImplementedError("visualize needs a viewer, which this library does not have")

    def save_xrdf(self, *args, **kwargs):
        raise NotImplementedError("save_xrdf needs an XRDF writer, which this library does not have (robot/xrdf.py reads XRDF); "
                                  "save(config, path) writes the YAML form")

    # ---- collision matrix
    def _config(self, ignore: Dict[str, List[str]]) -> Dict:
        if self._collision_spheres is None:
            raise ValueError("no collision spheres: call set_collision_spheres() first")
        cfg = dict(copy.deepcopy(self._passthrough))
        cfg.update(base_link=self._base_link, tool_frames=list(self._tool_frames), urdf_path=self.urdf_path,
                   asset_root_path=self.asset_path, collision_link_names=list(self._collision_spheres.keys()),
                   collision_spheres=copy.deepcopy(self._collision_spheres), mesh_link_names=list(self._collision_spheres.keys()),
                   self_collision_buffer=dict(self._self_collision_buffer), self_collision_ignore=copy.deepcopy(ignore))
        if self._cspace_config is not None:
            cfg["cspace"] = copy.deepcopy(self._cspace_config)
        return cfg

    def compute_collision_matrix(self, prune_collisions: bool = True, num_samples: int = 1000, batch_size: int = 10000,
                                 seed: int = 345, custom_ignore: Optional[Dict[str, List[str]]] = None) -> Dict[str, List[str]]:
        """The ``self_collision_ignore`` table (reference ``compute_collision_matrix``, :417-502): neighbours, ``custom_ignore``,
        link pairs that collide at the default joint position and -- ``prune_collisions`` -- link pairs that never collide over
        ``num_samples`` batches of ``batch_size`` Halton configurations.  Runs on ``device``; the statistics behind the table
        stay in ``collision_matrix_statistics``."""
        from ..kinematics import Kinematics, KinematicsCfg

        kin = Kinematics(KinematicsCfg.from_data_dict(self._config({}), device=self.device))
        self._matrix = compute_self_collision_matrix(kin, num_samples=num_samples, batch_size=batch_size, seed=seed,
                                                     custom_ignore=custom_ignore, prune_collisions=prune_collisions)
        self._self_collision_ignore = self._matrix.ignore
        return self._self_collision_ignore

    def add_collision_ignore(self, link_name: str, ignore_links: List[str]) -> None:
        if self._self_collision_ignore is None:
            self._self_collision_ignore = {}
        row = self._self_collision_ignore.setdefault(link_name, [])
        row.extend(k for k in ignore_links if k not in row)

    def remove_collision_ignore(self, link_name: str, ignore_links: List[str]) -> None:
        if self._self_collision_ignore is None or link_name not in self._self_collision_ignore:
            return
        row = self._self_collision_ignore[link_name]
        for k in ignore_links:
            if k in row:
                row.remove(k)

    # ---- build and save
    def build(self) -> Dict:
        """The ``kinematics`` dictionary that ``KinematicsCfg.from_data_dict`` and ``build_robot_model`` accept.  Without a
        collision matrix the neighbouring links are ignored, as the reference's ``build`` does."""
        if self._collision_spheres is None:
            self._collision_spheres = {}
        if self._self_collision_ignore is None:
            self._self_collision_ignore = neighbor_ignore(build_robot_model(self._config({}), self._urdf))
        return self._config(self._self_collision_ignore)

    def save(self, config: Dict, output_path: str) -> None:
        """YAML under ``robot_cfg: kinematics:`` (what ``load_robot_model`` and ``from_config`` read)"""
        import yaml

        os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
        with open(output_path, "w") as fh:
            yaml.safe_dump({"robot_cfg": {"kinematics": dict(config, format_version=2.0)}}, fh, sort_keys=False)

    # ---- inspection
    @property
    def tool_frames(self) -> List[str]:
        return self._tool_frames

    @property
    def collision_link_names(self) -> List[str]:
        return [] if self._collision_spheres is None else list(self._collision_spheres.keys())

    @property
    def collision_spheres(self) -> Optional[Dict[str, List[Dict]]]:
        return self._collision_spheres

    @property
    def collision_matrix(self) -> Optional[Dict[str, List[str]]]:
        return self._self_collision_ignore

    @property
    def collision_matrix_statistics(self) -> Optional[SelfCollisionMatrix]:
        """the ``SelfCollisionMatrix`` of the last ``compute_collision_matrix`` (None before)"""
        return self._matrix

    @property
    def num_spheres(self) -> int:
        return 0 if self._collision_spheres is None else sum(len(v) for v in self._collision_spheres.values())
