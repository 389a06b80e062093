"""Configuration of ``PoseDetector`` (reference pose_estimation/pose_detector_cfg.py: same fields, same defaults)."""

from dataclasses import dataclass, field

from ...types import DeviceCfg


@dataclass
class DetectorCfg:
    # coarse stage
    n_mesh_points_coarse: int = 500
    n_observed_points_coarse: int = 2000
    n_rotation_samples: int = 64
    n_iterations_coarse: int = 50
    distance_threshold_coarse: float = 0.5

    # fine stage
    n_mesh_points_fine: int = 2000
    n_observed_points_fine: int = 10000
    n_iterations_fine: int = 50
    distance_threshold_fine: float = 0.01

    #: the reference's second solver; not packaged
    use_svd: bool = False

    # robust estimation
    use_huber_loss: bool = True
    huber_delta: float = 0.02

    #: run without the graphs and keep the transform after every iteration
    save_iterations: bool = False

    device_cfg: DeviceCfg = field(default_factory=DeviceCfg)

    def __post_init__(self):
        if self.use_svd:
            raise NotImplementedError("the SVD solver is not packaged: use_svd must be False (the Cholesky solver)")
