"""Volumetric mapper (reference ``curobo._src.perception.mapper``): ``Mapper`` / ``MapperCfg``, depth frames and lidar range images
(``MapperLidarCfg``) to a dense TSDF to the exact fp16 ESDF the planners read; ``BlockSparseTSDFRenderer`` ray-casts the TSDF into
images and ``BlockSparseRaycastPoseRefiner`` tracks the camera against it; ``decay_and_recycle`` /
``decay_frustum_aware_multi_camera`` / ``decay_frustum_aware_multi_sensor`` let the map forget (reference ``kernel/wp_decay.py``)."""

from .decay import decay_and_recycle, decay_frustum_aware_multi_camera, decay_frustum_aware_multi_sensor
from .mapper import DenseTSDF, Mapper
from .mapper_cfg import MapperCfg, MapperLidarCfg
from .pose_refiner import BlockSparseRaycastPoseRefiner, BlockSparseRaycastRefinerCfg
from .renderer import BlockSparseTSDFRenderer, BlockSparseTSDFRendererCfg, depth_to_colormap, normals_to_colormap

__all__ = ["DenseTSDF", "Mapper", "MapperCfg", "BlockSparseTSDFRenderer", "BlockSparseTSDFRendererCfg", "BlockSparseRaycastPoseRefiner",
           "BlockSparseRaycastRefinerCfg", "depth_to_colormap", "normals_to_colormap", "decay_and_recycle",
           "decay_frustum_aware_multi_camera", "decay_frustum_aware_multi_sensor", "MapperLidarCfg"]
