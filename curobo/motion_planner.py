"""IK -> trajectory optimisation -> time-optimal finetune, grasp planning (``curobo_amd.motion_planner``; reference
curobo/motion_planner.py; the PRM graph planner behind ``MotionPlannerCfg.create(use_graph_planner=True)``)"""
from curobo_amd.motion_planner import GraspPlanResult, MotionPlanner, MotionPlannerCfg  # noqa: F401

__all__ = ["MotionPlanner", "MotionPlannerCfg", "GraspPlanResult"]
