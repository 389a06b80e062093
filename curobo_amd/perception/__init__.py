"""Depth-camera front end (reference ``curobo.perception``): ``FilterDepth`` cleans a depth image, ``RobotSegmenter``
removes the robot from it, ``SDFPoseDetector`` refines the pose of a known mesh (where the camera is relative to the
robot, where the object is) against the segmented points; the ICP ``PoseDetector`` / ``DetectorCfg`` that find such a
pose from scratch live in ``curobo_amd.perception.pose_estimation``.  What is left of the depth goes to a mapper (the reference's
block-sparse TSDF / ESDF ``Mapper`` is not part of this package; any ESDF producer will do) whose grid reaches the planners
through ``SceneData.update_voxel_features`` / ``update_voxel_data``.  Not packaged either: articulated ``RobotMesh`` and
the mapper's ``PoseRefinerRaycast``."""

from .filter_depth import FilterDepth, FilterDepthConfig
from .pose_estimation import DetectionResult, RobotMesh, SDFDetectorCfg, SDFPoseDetector
from .robot_segmenter import RobotSegmenter

__all__ = ["FilterDepth", "FilterDepthConfig", "RobotSegmenter", "DetectionResult", "RobotMesh", "SDFDetectorCfg", "SDFPoseDetector"]
