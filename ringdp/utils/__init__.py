"""ringdp.utils - hipGraph step capture, timing, tracing, checkpointing helpers, model EMA."""
from .ema import ModelEma  # noqa: F401
