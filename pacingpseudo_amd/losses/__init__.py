from .losses import mumford_shah_loss, normalized_cut_loss  # noqa: F401
