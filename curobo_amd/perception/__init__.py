"""Depth-camera front end (reference ``curobo.perception``): ``FilterDepth`` cleans a depth image, ``RobotSegmenter``
removes the robot from it, ``SDFPoseDetector`` refines the pose of a known mesh (where the camera is relative to the
robot, where the object is) against the segmented points; the ICP ``PoseDetector`` / ``DetectorCfg`` that find such a
pose from scratch live in ``curobo_amd.perception.pose_estimation``.  What is left of the depth goes to ``Mapper`` /
``MapperCfg``, which live in ``curobo_amd.perception.mapper`` (the reference's calls over a dense TSDF, ``integrate(obs)`` then
``compute_esdf()``; tests/test_pose_detector_host.py pins this package as having no attribute ``Mapper``), whose grid reaches
the planners through ``SceneData.update_voxel_data`` / ``update_voxel_features``.
Not packaged: articulated ``RobotMesh``, the mapper's ``PoseRefinerRaycast``, and what ``mapper/mapper.py`` lists."""

from .filter_depth import FilterDepth, FilterDepthConfig
from .pose_estimation import DetectionResult, RobotMesh, SDFDetectorCfg, SDFPoseDetector
from .robot_segmenter import RobotSegmenter

__all__ = ["FilterDepth", "FilterDepthConfig", "RobotSegmenter", "DetectionResult", "RobotMesh", "SDFDetectorCfg", "SDFPoseDetector"]
