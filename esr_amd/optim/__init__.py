from .flat_adam import LOSS_SCALE_DEFAULTS, FlatAdam, FlatAdamW

__all__ = ["FlatAdam", "FlatAdamW", "LOSS_SCALE_DEFAULTS"]
