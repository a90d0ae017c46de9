"""The epoch loops of the reference (`core/tools/__init__.py`, `train.py`, `test.py`) joined from this package's parts."""
from .test import run_tester, test
from .train import run_trainer, train, validate

__all__ = ["train", "validate", "run_trainer", "test", "run_tester"]
