"""frame-by-frame motion retargeting: global IK on the first frame, warm-started velocity-limited IK after it (``curobo_amd.motion_retargeter``)"""
from curobo_amd.motion_retargeter import MotionRetargeter, MotionRetargeterCfg, RetargetResult  # noqa: F401
from curobo_amd.types import GoalToolPose, SequenceGoalToolPose  # noqa: F401

__all__ = ["GoalToolPose", "MotionRetargeter", "MotionRetargeterCfg", "RetargetResult", "SequenceGoalToolPose"]
