"""Volumetric mapper (reference ``curobo._src.perception.mapper``): ``Mapper`` / ``MapperCfg``, depth frames to a dense TSDF to
the exact fp16 ESDF the planners read."""

from .mapper import DenseTSDF, Mapper
from .mapper_cfg import MapperCfg

__all__ = ["DenseTSDF", "Mapper", "MapperCfg"]
