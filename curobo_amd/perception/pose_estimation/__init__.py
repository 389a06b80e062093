"""Object / camera pose refinement against a known mesh (reference ``curobo/_src/perception/pose_estimation``): the
mesh-SDF Levenberg-Marquardt detector ``SDFPoseDetector``.  Not packaged: the ICP ``PoseDetector`` / ``DetectorCfg``,
articulated ``RobotMesh`` (the robot models carry spheres, not link meshes) and the mapper's ``PoseRefinerRaycast``."""

from .detection_result import DetectionResult
from .mesh_robot import RobotMesh
from .sdf_pose_detector import SDFPoseDetector
from .sdf_pose_detector_cfg import SDFDetectorCfg
from .util import extract_observed_points

__all__ = ["DetectionResult", "RobotMesh", "SDFDetectorCfg", "SDFPoseDetector", "extract_observed_points"]
