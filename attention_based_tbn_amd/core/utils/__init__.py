from .create_dataloader import ClipLoader, create_dataloader
from .metric import DeviceMetric, Metric
from .misc import get_modality, get_time_diff, load_checkpoint, save_checkpoint, save_scores
from .optim import FusedAdam, FusedSGD, clip_grad_norm_
from .train_step import TrainStep
from .warmup import GradualWarmupScheduler, build_optimizer

__all__ = ["ClipLoader", "create_dataloader", "Metric", "DeviceMetric", "get_modality", "get_time_diff", "save_checkpoint", "load_checkpoint", "save_scores",
           "FusedSGD", "FusedAdam", "clip_grad_norm_", "TrainStep", "GradualWarmupScheduler",
           "build_optimizer"]
