"""depth-camera front end (``curobo_amd.perception``; reference curobo/perception.py, without the mapper and the detectors)"""
from curobo_amd.perception import FilterDepth, RobotSegmenter  # noqa: F401

__all__ = ["FilterDepth", "RobotSegmenter"]
