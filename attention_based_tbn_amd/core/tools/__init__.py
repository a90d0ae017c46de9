"""The epoch loops of the reference (`core/tools/__init__.py`, `train.py`, `test.py`) joined from this package's parts,
and its visualisation module (`vis.py`)."""
from .test import run_tester, test
from .train import run_trainer, train, validate
from .vis import create_dataset, get_info, initialize, save_action_segment, visualize

__all__ = ["train", "validate", "run_trainer", "test", "run_tester",
           "initialize", "create_dataset", "visualize", "get_info", "save_action_segment"]
