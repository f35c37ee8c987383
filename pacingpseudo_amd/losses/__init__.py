from .losses import normalized_cut_loss  # noqa: F401
