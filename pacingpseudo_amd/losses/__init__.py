from .losses import (bidirectional_kl_loss, hard_label_cross_entropy_loss, js_loss, mumford_shah_loss,  # noqa: F401
                     normalized_cut_loss, teacher_consistency_loss)
