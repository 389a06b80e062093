"""Depth-camera front end (reference ``curobo.perception``): ``FilterDepth`` cleans a depth image, ``RobotSegmenter``
removes the robot from it.  What is left goes to a mapper (the reference's block-sparse TSDF / ESDF ``Mapper`` is not
part of this package; any ESDF producer will do) whose grid reaches the planners through
``SceneData.update_voxel_features`` / ``update_voxel_data``."""

from .filter_depth import FilterDepth, FilterDepthConfig
from .robot_segmenter import RobotSegmenter

__all__ = ["FilterDepth", "FilterDepthConfig", "RobotSegmenter"]
