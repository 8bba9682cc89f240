"""MI355X-native failure-aware classification path.

``Backend`` is the drop-in scorer; everything it computes runs in the HIP
library behind include/fav.h.  Importing this package does not load the
library; constructing a Backend does, and raises if it (or a gfx950 GPU) is
missing — there is no CPU fallback.
"""
from .backend import Backend, anomaly_score_from_confidence, unpack_uncertainty  # noqa: F401
from .conformal import Conformal, calibrate_qhat, unpack_sets  # noqa: F401
from .calibration import (Calibration, fit_temperature, reliability, risk_coverage, tau_for_risk, temperature_grid,  # noqa: F401
                          unpack_cells)
from .corrupt import CORRUPTIONS, SEVERITY, Corruptor  # noqa: F401
from .distributed import classify_sharded, shard_range  # noqa: F401
from . import autoencoder, cam, coreset, faithfulness, ood, patch, robustness, rollout, synth, views, weights  # noqa: F401
from .autoencoder import Autoencoder, blob_from_state_dict, make_synthetic_ae, torch_module, unpack_ae_records  # noqa: F401
from .coreset import CoresetSelection, select_coreset  # noqa: F401
from .patch import PatchBank, build_patch_bank, unpack_patch_records  # noqa: F401
from .cam import box_to_pixels, evidence_share, unpack_cam_records  # noqa: F401
from .rollout import patch_box_to_pixels, unpack_rollout_records  # noqa: F401
from .faithfulness import random_maps, unpack_curve_records  # noqa: F401
from .ood import (DriftReference, KNNBank, OODModel, build_drift_reference, build_knn_bank, fit_mahalanobis,  # noqa: F401
                  unpack_drift_record)
from .views import View  # noqa: F401
from .robustness import summarize  # noqa: F401
