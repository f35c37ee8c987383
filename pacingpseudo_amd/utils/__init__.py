from .utils import AvgMeter, cosine_lr_decay, gaussian_ramp_up, linear_lr_decay, poly_lr_decay  # noqa: F401
from .postprocess import keep_largest_components, label_components  # noqa: F401
from .tta import TTA_MODES, tta_ops, tta_predict, tta_view  # noqa: F401
from .metrics import batch_surface_metrics, compute_hd, surface_metrics_from_reduction  # noqa: F401
from .crf_refine import check_crf_refine_params, crf_refine  # noqa: F401
from .random_walker import check_rw_params, expand_scribbles, random_walker  # noqa: F401
from .random_walker import SharedMaps, check_rw_prior_params, random_walker_prior, refresh_dataset, refresh_scribbles  # noqa: F401
from .uncertainty import add_noise, check_uncertainty_params, uncertainty_mask, uncertainty_threshold  # noqa: F401
from .distance import distance_transform_edt, signed_distance_maps  # noqa: F401
from .geodesic import check_geo_params, expand_dataset_geo, geodesic_distance, geodesic_expand_scribbles  # noqa: F401
from .volume import (distance_transform_edt_3d, group_volumes, keep_largest_components_3d, label_components_3d, volume_dice,  # noqa: F401
                     volume_surface_metrics)
from .morphology import (binary_fill_holes, check_morph_params, fill_holes, fill_holes_3d, remove_small_components,  # noqa: F401
                         remove_small_components_3d)
from .sorting import sort_descending  # noqa: F401
