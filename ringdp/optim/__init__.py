"""ringdp.optim - optimizers with fused CDNA4 update kernels."""
from .adamw import Adam, AdamW  # noqa: F401
from . import lr_scheduler  # noqa: F401
from .sgd import SGD  # noqa: F401

__all__ = ["SGD", "Adam", "AdamW", "lr_scheduler"]
