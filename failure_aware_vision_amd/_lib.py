"""ctypes binding of include/fav.h (the C-ABI drop-in boundary).

Loads ``failure_aware_vision_amd/lib/libfav_hip.so`` (built in-tree by
``__graft_entry__.build()`` / ``csrc/Makefile``).  There is NO fallback: if the
library is missing the import of this module raises, and if no gfx950 device is
present ``fav_create`` returns FAV_ERR_NO_DEVICE, which ``Backend`` turns into a
RuntimeError.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FAV_LIB_PATH") or os.path.join(_HERE, "lib", "libfav_hip.so")   # FAV_LIB_PATH: A/B of two builds

FAV_OK = 0
FAV_ERR_INVALID_ARG = 1
STATUS_NAMES = {0: "FAV_OK", 1: "FAV_ERR_INVALID_ARG", 2: "FAV_ERR_BAD_BLOB", 3: "FAV_ERR_NO_WEIGHTS",
                4: "FAV_ERR_HIP", 5: "FAV_ERR_NO_DEVICE", 6: "FAV_ERR_UNSUPPORTED"}
LAYOUT_NHWC_U8, LAYOUT_NHWC_F32 = 0, 1
ARCH_RESNET18_CIFAR, ARCH_RESNET50, ARCH_VIT_B16, ARCH_VIT_TINY = 0, 1, 2, 3
CONF_MAX_SOFTMAX, CONF_ENTROPY, CONF_MUTUAL_INFO = 0, 1, 2
MATH_BF16, MATH_F32_EXACT = 0, 1
K_STEM, K_CONV, K_MAXPOOL, K_AVGPOOL, K_DROPOUT, K_HEAD, K_COUNT = 0, 1, 2, 3, 4, 5, 6
KERNEL_CLASS_NAMES = ("stem_im2col", "conv_igemm", "maxpool", "avgpool", "entry_dropout", "head")


class FavConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("device", C.c_int32), ("arch", C.c_int32), ("num_classes", C.c_int32),
        ("in_h", C.c_int32), ("in_w", C.c_int32), ("max_batch", C.c_int32),
        ("mean", C.c_float * 3), ("stdev", C.c_float * 3),
        ("n_samples", C.c_int32), ("site_mask", C.c_uint32), ("dropout_p", C.c_float), ("seed", C.c_uint64),
        ("temperature", C.c_float), ("conf_kind", C.c_int32), ("tau", C.c_float), ("math_mode", C.c_int32),
        ("chunk_a", C.c_int32), ("chunk_b", C.c_int32), ("regroup_block", C.c_int32), ("n_members", C.c_int32),
        ("tail_min_rows", C.c_int32), ("ens_grouped_max", C.c_int32), ("vit_streams", C.c_int32), ("stem_fused", C.c_int32),
    ]


class FavDropoutDesc(C.Structure):
    _fields_ = [("site", C.c_int32), ("threshold", C.c_uint32), ("scale", C.c_float), ("seed", C.c_uint64),
                ("v0", C.c_int64), ("n_img", C.c_int32), ("first_image_index", C.c_int64)]


class FavConvDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("res", C.c_void_p), ("y", C.c_void_p),
                ("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32),
                ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
                ("relu", C.c_int32), ("out_f32", C.c_int32), ("math_mode", C.c_int32), ("drop", FavDropoutDesc)]


class FavLinearDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("res", C.c_void_p), ("y", C.c_void_p),
                ("rows", C.c_int64), ("K", C.c_int32), ("N", C.c_int32), ("act", C.c_int32)]


class FavTailDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("wb", C.c_void_p), ("bias_b", C.c_void_p), ("wc", C.c_void_p), ("bias_c", C.c_void_p),
                ("res", C.c_void_p), ("y", C.c_void_p), ("wa", C.c_void_p), ("bias_a", C.c_void_p), ("t1n", C.c_void_p),
                ("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cmid", C.c_int32), ("Nred", C.c_int32),
                ("drop", FavDropoutDesc), ("res_entry", C.c_int32), ("entry_site", C.c_int32)]


class FavUncertainty(C.Structure):
    """fav_uncertainty: one 72-byte record per frame (18 dwords; backend.unpack_uncertainty reads it as int32[n, 18])."""
    _fields_ = [("label", C.c_int32), ("confidence", C.c_float), ("mean_prob", C.c_float), ("prob_std", C.c_float),
                ("pred_entropy", C.c_float), ("expected_entropy", C.c_float), ("mutual_info", C.c_float),
                ("agreement", C.c_float), ("top_label", C.c_int32 * 5), ("top_prob", C.c_float * 5)]


CP_LAC, CP_APS = 0, 1


class FavConformal(C.Structure):
    """fav_conformal: the split-conformal score and its calibrated threshold (32 bytes)."""
    _fields_ = [("struct_size", C.c_uint32), ("score_kind", C.c_int32), ("randomized", C.c_int32), ("k_reg", C.c_int32),
                ("lambda_", C.c_float), ("qhat", C.c_float), ("seed", C.c_uint64)]


class FavPredSet(C.Structure):
    """fav_pred_set: one 160-byte prediction-set record per frame (40 dwords; conformal.unpack_sets reads it as int32[n, 40])."""
    _fields_ = [("label", C.c_int32), ("confidence", C.c_float), ("set_size", C.c_int32), ("set_mass", C.c_float),
                ("u", C.c_float), ("reserved", C.c_int32 * 3), ("member", C.c_uint32 * 32)]


SWEEP_MAX_TEMPS = 32


class FavCalibCell(C.Structure):
    """fav_calib_cell: one 16-byte cell per (frame, temperature) of a sweep (calibration.unpack_cells reads int32[n, K, 4])."""
    _fields_ = [("label", C.c_int32), ("confidence", C.c_float), ("nll", C.c_float), ("brier", C.c_float)]


#: fav_corruption, in enum order
CORRUPTION_KINDS = ("impulse_noise", "speckle_noise", "gaussian_blur", "defocus_blur", "contrast", "pixelate", "brightness",
                    "saturate")


class FavCorruptionDesc(C.Structure):
    """fav_corruption_desc: one corruption of fav_op_corrupt_c (32 bytes)."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("a", C.c_float), ("b", C.c_float), ("seed", C.c_uint64),
                ("first_frame_index", C.c_int64)]


MAX_VIEWS = 64
BORDER_REFLECT101, BORDER_REPLICATE, BORDER_ZERO = 0, 1, 2


class FavView(C.Structure):
    """fav_view: one test-time-augmentation view (24 bytes; views.View mirrors it)."""
    _fields_ = [("flip_x", C.c_int32), ("flip_y", C.c_int32), ("transpose", C.c_int32), ("dy", C.c_int32), ("dx", C.c_int32),
                ("border", C.c_int32)]


class FavOodModel(C.Structure):
    """fav_ood_model: the Mahalanobis model as a whitening projection, host pointers (ood.OODModel.to_c fills it)."""
    _fields_ = [("struct_size", C.c_uint32), ("D", C.c_int32), ("k", C.c_int32), ("R", C.c_int32),
                ("mu", C.POINTER(C.c_float)), ("P", C.POINTER(C.c_float)), ("M", C.POINTER(C.c_float)),
                ("class_id", C.POINTER(C.c_int32)), ("threshold", C.c_float)]


class FavOodRecord(C.Structure):
    """fav_ood_record: one 16-byte score per frame (ood.unpack_records reads it as int32[n, 4])."""
    _fields_ = [("min_dist", C.c_float), ("min_class", C.c_int32), ("label_dist", C.c_float), ("ood", C.c_int32)]


class FavKnnBank(C.Structure):
    """fav_knn_bank: a bank of L2-normalised bf16 feature rows, host pointers (ood.KNNBank.to_c fills it)."""
    _fields_ = [("struct_size", C.c_uint32), ("D", C.c_int32), ("N", C.c_int32), ("k", C.c_int32),
                ("rows", C.POINTER(C.c_uint16)), ("class_id", C.POINTER(C.c_int32)), ("threshold", C.c_float)]


class FavKnnRecord(C.Structure):
    """fav_knn_record: one 24-byte score per frame (ood.unpack_knn_records reads it as int32[n, 6])."""
    _fields_ = [("kth_dist", C.c_float), ("kth_sim", C.c_float), ("nn_sim", C.c_float), ("nn_row", C.c_int32),
                ("nn_class", C.c_int32), ("ood", C.c_int32)]


class FavDriftRef(C.Structure):
    """fav_drift_ref: a reference of L2-normalised bf16 feature rows, host pointers (ood.DriftReference.to_c fills it)."""
    _fields_ = [("struct_size", C.c_uint32), ("D", C.c_int32), ("R", C.c_int32), ("n_perm", C.c_int32),
                ("rows", C.POINTER(C.c_uint16)), ("seed", C.c_uint64), ("alpha", C.c_float)]


class FavDriftRecord(C.Structure):
    """fav_drift_record: one 48-byte record per call (ood.unpack_drift_record reads it as int32[12])."""
    _fields_ = [("statistic", C.c_double), ("s_ab", C.c_int64), ("s_aa", C.c_int64), ("s_bb", C.c_int64),
                ("p_value", C.c_float), ("n_exceed", C.c_int32), ("drift", C.c_int32), ("n_degenerate", C.c_int32)]


class FavCamRecord(C.Structure):
    """fav_cam_record: one 32-byte summary per (frame, class) map (cam.unpack_cam_records reads it as int32[..., 8])."""
    _fields_ = [("class_id", C.c_int32), ("logit_mean", C.c_float), ("peak", C.c_float), ("peak_cell", C.c_int32),
                ("floor", C.c_float), ("pos_sum", C.c_float), ("n_above", C.c_int32), ("box", C.c_int32)]


class FavRolloutRecord(C.Structure):
    """fav_rollout_record: one 32-byte summary per frame (rollout.unpack_rollout_records reads it as int32[..., 8]); peak and
    floor stand where FavCamRecord has them."""
    _fields_ = [("n_layers", C.c_int32), ("cls_mass", C.c_float), ("peak", C.c_float), ("peak_cell", C.c_int32),
                ("floor", C.c_float), ("patch_sum", C.c_float), ("n_above", C.c_int32), ("box", C.c_int32)]


class FavPatchBank(C.Structure):
    """fav_patch_bank: a bank of L2-normalised bf16 patch-feature rows, host pointers (patch.PatchBank.to_c fills it)."""
    _fields_ = [("struct_size", C.c_uint32), ("D", C.c_int32), ("N", C.c_int32), ("chunk_rows", C.c_int32),
                ("rows", C.POINTER(C.c_uint16)), ("threshold", C.c_float)]


class FavPatchSite(C.Structure):
    """fav_patch_site: where a patch bank's rows come from - the residual stage 1 .. 4 and the neighbourhood radius 0 .. 2."""
    _fields_ = [("struct_size", C.c_uint32), ("stage", C.c_int32), ("radius", C.c_int32)]


class FavPatchRecord(C.Structure):
    """fav_patch_record: one 32-byte summary per frame (patch.unpack_patch_records reads it as int32[..., 8]); peak and floor
    stand where FavCamRecord has them."""
    _fields_ = [("n_degenerate", C.c_int32), ("mean_dist", C.c_float), ("peak", C.c_float), ("peak_cell", C.c_int32),
                ("floor", C.c_float), ("peak_row", C.c_int32), ("n_above", C.c_int32), ("box", C.c_int32)]


CURVE_DELETION, CURVE_INSERTION = 0, 1
CURVE_MODES = ("deletion", "insertion")


class FavCurve(C.Structure):
    """fav_curve: the steps of a deletion / insertion curve and the fill of an occluded pixel in either layout (32 bytes)."""
    _fields_ = [("struct_size", C.c_uint32), ("steps", C.c_int32), ("fill_u8", C.c_uint32 * 3), ("fill_f32_bits", C.c_uint32 * 3)]


class FavCurveRecord(C.Structure):
    """fav_curve_record: one 32-byte summary per frame (faithfulness.unpack_curve_records reads it as int32[..., 8])."""
    _fields_ = [("class_id", C.c_int32), ("auc", C.c_float), ("p_first", C.c_float), ("flip_step", C.c_int32),
                ("p_last", C.c_float), ("p_min", C.c_float), ("flip_cells", C.c_int32), ("reserved", C.c_int32)]


class FavRise(C.Structure):
    """fav_rise: the masks of a RISE map - their number, the grid, the keep threshold in 256ths, the seed - and the fill of a
    masked-out pixel in either layout (48 bytes)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_masks", C.c_int32), ("grid", C.c_int32), ("keep", C.c_int32), ("seed", C.c_uint64),
                ("fill_u8", C.c_uint32 * 3), ("fill_f32_bits", C.c_uint32 * 3)]


class FavRiseRecord(C.Structure):
    """fav_rise_record: one 32-byte summary per frame (rise.unpack_rise_records reads it as int32[..., 8])."""
    _fields_ = [("class_id", C.c_int32), ("p_full", C.c_float), ("peak", C.c_float), ("peak_cell", C.c_int32),
                ("floor", C.c_float), ("p_mean", C.c_float), ("n_above", C.c_int32), ("box", C.c_int32)]


class FavAeConfig(C.Structure):
    """fav_ae_config: the autoencoder sensor's frame size, level count, batch and cell (24 bytes)."""
    _fields_ = [("struct_size", C.c_uint32), ("in_h", C.c_int32), ("in_w", C.c_int32), ("levels", C.c_int32),
                ("max_batch", C.c_int32), ("cell", C.c_int32)]


class FavAeRecord(C.Structure):
    """fav_ae_record: one 32-byte summary per frame (autoencoder.unpack_ae_records reads it as int32[..., 8]); peak and floor
    stand where FavCamRecord has them."""
    _fields_ = [("sse_lo", C.c_uint32), ("mse", C.c_float), ("peak", C.c_float), ("peak_cell", C.c_int32),
                ("floor", C.c_float), ("sse_hi", C.c_uint32), ("n_above", C.c_int32), ("box", C.c_int32)]


class FavProfile(C.Structure):
    _fields_ = [("ms", C.c_double * K_COUNT), ("flops", C.c_double * K_COUNT), ("bytes", C.c_double * K_COUNT),
                ("launches", C.c_int64 * K_COUNT)]


class FavOpProfile(C.Structure):
    _fields_ = [("op_index", C.c_int32), ("kind", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
                ("Ho", C.c_int32), ("Wo", C.c_int32), ("Cout", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
                ("stride", C.c_int32), ("reserved", C.c_int32), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double), ("launches", C.c_int64)]


_SIGNATURES = {
    "fav_abi_version": (C.c_int32, []),
    "fav_default_config": (None, [C.POINTER(FavConfig), C.c_int32]),
    "fav_create": (C.c_int, [C.POINTER(FavConfig), C.POINTER(C.c_void_p)]),
    "fav_load_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "fav_load_member_weights": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "fav_destroy": (None, [C.c_void_p]),
    "fav_check_blob": (C.c_int, [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]),
    "fav_plan_schedule": (C.c_int, [C.POINTER(FavConfig), C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_last_error": (C.c_char_p, [C.c_void_p]),
    "fav_classify": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_classify_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_classify_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "fav_classify_uncertainty": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "fav_classify_sets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(FavConformal),
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_conformal_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(FavConformal),
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_classify_sweep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(C.c_float),
                                     C.c_int32, C.c_void_p, C.c_void_p]),
    "fav_set_temperature": (C.c_int, [C.c_void_p, C.c_float]),
    "fav_set_tau": (C.c_int, [C.c_void_p, C.c_float]),
    "fav_set_conf_kind": (C.c_int, [C.c_void_p, C.c_int32]),
    "fav_check_views": (C.c_int, [C.POINTER(FavView), C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_set_views": (C.c_int, [C.c_void_p, C.POINTER(FavView), C.c_int32]),
    "fav_get_views": (C.c_int, [C.c_void_p, C.POINTER(FavView), C.c_int32, C.POINTER(C.c_int32)]),
    "fav_set_feature_tap": (C.c_int, [C.c_void_p, C.c_int32]),
    "fav_get_features": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.c_void_p]),
    "fav_check_ood_model": (C.c_int, [C.POINTER(FavOodModel), C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_set_ood": (C.c_int, [C.c_void_p, C.POINTER(FavOodModel)]),
    "fav_classify_ood": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_ood_score": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "fav_check_knn_bank": (C.c_int, [C.POINTER(FavKnnBank), C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_set_knn": (C.c_int, [C.c_void_p, C.POINTER(FavKnnBank)]),
    "fav_classify_knn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_knn_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "fav_op_knn_score": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "fav_check_drift_ref": (C.c_int, [C.POINTER(FavDriftRef), C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_set_drift": (C.c_int, [C.c_void_p, C.POINTER(FavDriftRef)]),
    "fav_classify_drift": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_drift_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "fav_op_drift_test": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64,
                                    C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_set_map_tap": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t]),
    "fav_get_maps": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                               C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "fav_map_tap_info": (C.c_int, [C.POINTER(FavConfig), C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]),
    "fav_cam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_classify_cam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_cam": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                             C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_cam_heatmap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p]),
    "fav_set_attn_tap": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t]),
    "fav_get_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), C.c_void_p]),
    "fav_attn_tap_info": (C.c_int, [C.POINTER(FavConfig), C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                    C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]),
    "fav_rollout": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_classify_rollout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_attn_mean": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "fav_op_attn_rollout": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "fav_check_curve": (C.c_int, [C.POINTER(FavCurve), C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_set_curve": (C.c_int, [C.c_void_p, C.POINTER(FavCurve)]),
    "fav_classify_curve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_rank_cells": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "fav_op_occlude": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                 C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.c_void_p]),
    "fav_op_head_class_prob": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_curve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                               C.c_void_p, C.c_void_p]),
    "fav_check_rise": (C.c_int, [C.POINTER(FavRise), C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_set_rise": (C.c_int, [C.c_void_p, C.POINTER(FavRise)]),
    "fav_classify_rise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_rise_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(FavRise), C.c_int64,
                                   C.c_int32, C.c_int32, C.c_void_p]),
    "fav_op_rise_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(FavRise), C.c_int64, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_check_patch_bank": (C.c_int, [C.POINTER(FavPatchBank), C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_set_patch_bank": (C.c_int, [C.c_void_p, C.POINTER(FavPatchBank)]),
    "fav_patch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_classify_patch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_patch_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "fav_patch_chunk_rows": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
    "fav_op_patch_score": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                     C.c_int32, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_patch_score_at": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                        C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "fav_op_patch_query": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "fav_check_patch_site": (C.c_int, [C.POINTER(FavPatchSite), C.c_char_p, C.c_size_t]),
    "fav_set_patch_bank_at": (C.c_int, [C.c_void_p, C.POINTER(FavPatchBank), C.POINTER(FavPatchSite)]),
    "fav_set_stage_tap": (C.c_int, [C.c_void_p, C.c_int32, C.c_size_t]),
    "fav_get_stage_maps": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "fav_stage_tap_info": (C.c_int, [C.POINTER(FavConfig), C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]),
    "fav_check_coreset": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_coreset_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "fav_op_coreset_select": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "fav_check_ae_config": (C.c_int, [C.POINTER(FavAeConfig), C.c_char_p, C.c_size_t]),
    "fav_ae_info": (C.c_int, [C.POINTER(FavAeConfig), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                              C.POINTER(C.c_int32), C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]),
    "fav_ae_check_blob": (C.c_int, [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]),
    "fav_ae_create": (C.c_int, [C.POINTER(FavAeConfig), C.POINTER(C.c_void_p)]),
    "fav_ae_load_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "fav_ae_set_threshold": (C.c_int, [C.c_void_p, C.c_float]),
    "fav_ae_destroy": (None, [C.c_void_p]),
    "fav_ae_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_ae_decode_compare": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "fav_classify_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "fav_get_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "fav_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "fav_get_profile": (C.c_int, [C.c_void_p, C.POINTER(FavProfile), C.c_int32]),
    "fav_get_op_profile": (C.c_int, [C.c_void_p, C.POINTER(FavOpProfile), C.c_int32, C.POINTER(C.c_int32)]),
    "fav_op_conv2d": (C.c_int, [C.POINTER(FavConvDesc), C.c_void_p]),
    "fav_op_bottleneck_tail": (C.c_int, [C.POINTER(FavTailDesc), C.c_void_p]),
    "fav_op_last_route": (C.c_int, [C.c_char_p, C.c_size_t]),
    "fav_route_conv2d": (C.c_int, [C.POINTER(FavConvDesc), C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_route_bottleneck_tail": (C.c_int, [C.POINTER(FavTailDesc), C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_route_attention": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]),
    "fav_op_linear_streamk": (C.c_int, [C.POINTER(FavLinearDesc), C.c_void_p]),
    "fav_op_stem_im2col": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.c_void_p, C.c_void_p]),
    "fav_op_stem_pool": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_maxpool3x3s2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "fav_op_avgpool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(FavDropoutDesc),
                                 C.c_void_p]),
    "fav_op_entry_dropout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(FavDropoutDesc),
                                       C.c_void_p]),
    "fav_op_entry_reduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.POINTER(FavDropoutDesc), C.c_void_p]),
    "fav_op_layernorm": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                   C.c_void_p]),
    "fav_op_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "fav_op_vit_assemble": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "fav_op_head": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_float,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_head_uncertainty": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                          C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_op_head_sets": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_float,
                                   C.c_int64, C.POINTER(FavConformal), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "fav_op_head_sweep": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "fav_corruption_params": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "fav_corruption_taps": (C.c_int, [C.c_int32, C.c_float, C.c_float, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32)]),
    "fav_op_corrupt_c": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(FavCorruptionDesc),
                                   C.c_void_p]),
    "fav_op_views": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(FavView), C.c_int32,
                               C.c_void_p]),
}

_lib = None


def load():
    """Load the shared library once.  torch is imported first so that the HIP
    runtime both sides use is the single libamdhip64.so.7 torch already mapped
    (device pointers and streams are then interchangeable)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C failure_aware_vision_amd/csrc`).  There is no CPU fallback for this path.")
    import torch  # noqa: F401  (maps torch's libamdhip64 first)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_route() -> str:
    """fav_op_last_route: the kernel the calling thread's most recent fav_op_* launch took ('' after a refusal)."""
    buf = C.create_string_buffer(96)
    check(load().fav_op_last_route(buf, len(buf)))
    return buf.value.decode("ascii")


def _route_query(fn, *args):
    """(status, text) of a fav_route_*: the route name with FAV_OK, the refusal text with FAV_ERR_INVALID_ARG."""
    buf = C.create_string_buffer(160)
    status = fn(*args, buf, len(buf))
    return status, buf.value.decode("ascii")


def route_conv2d(desc: FavConvDesc, vit: int = 0, groups: int = 1):
    """fav_route_conv2d: the kernel fav_op_conv2d would take for this descriptor; no device, nothing launched."""
    return _route_query(load().fav_route_conv2d, C.byref(desc), vit, groups)


def route_bottleneck_tail(desc: FavTailDesc, groups: int = 1):
    """fav_route_bottleneck_tail: likewise for fav_op_bottleneck_tail."""
    return _route_query(load().fav_route_bottleneck_tail, C.byref(desc), groups)


def route_attention(n: int, T: int, D: int, heads: int, math_mode: int = 0):
    """fav_route_attention: likewise for fav_op_attention."""
    return _route_query(load().fav_route_attention, n, T, D, heads, math_mode)


class FavError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


def check(status: int, handle=None):
    if status != FAV_OK:
        msg = load().fav_last_error(handle)
        raise FavError(status, (msg or b"").decode("utf-8", "replace"))
