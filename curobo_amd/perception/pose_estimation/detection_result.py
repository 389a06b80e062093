"""Result of a pose detection (reference pose_estimation/detection_result.py)."""

from dataclasses import dataclass
from typing import Optional

from ...types import Pose


@dataclass
class DetectionResult:
    pose: Pose                 # camera-to-object transform
    config: Optional[object]   # joint configuration (robots) or None (rigid objects)
    confidence: float
    alignment_error: float
    n_iterations: int
    compute_time: float = 0.0
