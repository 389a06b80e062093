"""Configuration of ``SDFPoseDetector`` (reference pose_estimation/sdf_pose_detector_cfg.py: same fields, same defaults)."""

from dataclasses import dataclass, field

from ...types import DeviceCfg


@dataclass
class SDFDetectorCfg:
    # optimisation
    max_iterations: int = 100
    inner_iterations: int = 25                    # iterations per captured graph (no convergence check inside)
    convergence_threshold: float = 1e-5           # translation (m)
    rotation_convergence_threshold: float = 1e-5  # rotation (rad)

    use_cuda_graph: bool = True                   # (hipGraph here; the reference's name is kept)

    # correspondences
    distance_threshold: float = 0.2               # reject correspondences beyond this (m)
    min_valid_ratio: float = 0.1

    # robust estimation
    use_huber: bool = True
    huber_delta: float = 0.1

    # Levenberg-Marquardt
    lambda_initial: float = 1e-3
    lambda_factor: float = 10.0
    lambda_min: float = 1e-7
    lambda_max: float = 1e7
    #: carried for the reference's interface; its trust-region update accepts on ``ratio >= 0`` and never reads this
    rho_min: float = 0.25

    n_points: int = 5000

    device_cfg: DeviceCfg = field(default_factory=DeviceCfg)

    @property
    def max_distance(self):
        return self.distance_threshold
