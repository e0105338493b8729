"""fastegnn_amd -- MI355X-native (gfx950) forward/backward of the FastEGNN model.

Only the hot path of GLAD-RUC/FastEGNN lives here: the drop-in ``FastEGNN`` module
(``model.py``), its ctypes binding (``_lib.py``) and the HIP sources (``csrc/``).
"""
from .model import FastEGNN, SortedGraph  # noqa: F401
from .egnn import EGNN  # noqa: F401
from .fastrf import FastRF  # noqa: F401
from .train import FusedAdam, MMDSampler, evaluate, train_epoch, train_step  # noqa: F401
from .checkpoint import fit, load_checkpoint, save_checkpoint  # noqa: F401
from .rollout import Rollout, rollout  # noqa: F401
from .data import apply_motion  # noqa: F401

__all__ = ["FastEGNN", "FastRF", "EGNN", "SortedGraph", "FusedAdam", "MMDSampler", "train_step", "train_epoch", "evaluate",
           "fit", "save_checkpoint", "load_checkpoint", "Rollout", "rollout", "apply_motion"]
