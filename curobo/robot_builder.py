"""a robot configuration from a URDF and collision spheres, with its self-collision matrix computed on the GPU
(``curobo_amd.robot.builder``, ``curobo_amd.robot.collision_matrix``; reference curobo/robot_builder.py)"""
from curobo_amd.robot.builder import RobotBuilder  # noqa: F401
from curobo_amd.robot.collision_matrix import (SelfCollisionMatrix, candidate_link_pairs, compute_self_collision_matrix,  # noqa: F401
                                               pruned_collision_pairs)

__all__ = ["RobotBuilder", "SelfCollisionMatrix", "candidate_link_pairs", "compute_self_collision_matrix", "pruned_collision_pairs"]
