"""Object / camera pose refinement against a known mesh (reference ``curobo/_src/perception/pose_estimation``): the
ICP detector ``PoseDetector``, which finds a pose from scratch, and the mesh-SDF Levenberg-Marquardt detector
``SDFPoseDetector``, which refines one.  Not packaged: the ICP detector's SVD solver, ``RigidObjectGeometry`` /
``ArticulatedRobotGeometry``, articulated ``RobotMesh`` (the robot models carry spheres, not link meshes) and the mapper's
``PoseRefinerRaycast``."""

from .detection_result import DetectionResult
from .mesh_robot import RobotMesh
from .pose_detector import PoseDetector
from .pose_detector_cfg import DetectorCfg
from .sdf_pose_detector import SDFPoseDetector
from .sdf_pose_detector_cfg import SDFDetectorCfg
from .util import extract_observed_points

__all__ = ["DetectionResult", "DetectorCfg", "PoseDetector", "RobotMesh", "SDFDetectorCfg", "SDFPoseDetector", "extract_observed_points"]
