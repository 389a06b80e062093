"""depth-camera front end (``curobo_amd.perception``; reference curobo/perception.py; the mapper: ``curobo_amd.perception.mapper``)"""
from curobo_amd.perception import FilterDepth, RobotSegmenter  # noqa: F401
# the mesh-SDF pose detector: importable from here, but not listed -- tests/test_perception_host.py pins __all__ as it is
from curobo_amd.perception import DetectionResult, RobotMesh, SDFDetectorCfg, SDFPoseDetector  # noqa: F401
# the ICP pose detector: likewise importable and not listed
from curobo_amd.perception.pose_estimation import DetectorCfg, PoseDetector  # noqa: F401
# the depth mapper (Mapper / MapperCfg) is imported from curobo_amd.perception.mapper: tests/test_perception_host.py pins this
# module as having no attribute Mapper
# the mapper's decay and recycling functions (reference kernel/wp_decay.py): importable from here and not listed, like the detectors
from curobo_amd.perception.mapper.decay import decay_and_recycle, decay_frustum_aware_multi_camera, decay_frustum_aware_multi_sensor  # noqa: F401

__all__ = ["FilterDepth", "RobotSegmenter"]
