"""ctypes binding of libbodyfit.so (include/bodyfit.h).  No fallback: without the HIP library the
product path raises - there is deliberately no CPU implementation behind this ABI."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BODYFIT_LIB selects a diagnostic build (e.g. libbodyfit_stamp.so) for bring-up tools; never a different backend
LIB_PATH = os.environ.get("BODYFIT_LIB") or os.path.join(_HERE, "libbodyfit.so")


class BodyfitError(RuntimeError):
    pass


class ModelDesc(C.Structure):
    _fields_ = [
        ("n_verts", C.c_int32), ("n_joints", C.c_int32), ("n_betas", C.c_int32),
        ("v_template", C.POINTER(C.c_float)), ("shapedirs", C.POINTER(C.c_float)),
        ("posedirs", C.POINTER(C.c_float)), ("j_regressor", C.POINTER(C.c_float)),
        ("lbs_weights", C.POINTER(C.c_float)), ("parents", C.POINTER(C.c_int32)),
        ("n_selector", C.c_int32), ("selector_ids", C.POINTER(C.c_int32)),
        ("n_extra", C.c_int32), ("j_regressor_extra", C.POINTER(C.c_float)),
        ("n_joint_map", C.c_int32), ("joint_map", C.POINTER(C.c_int32)),
        ("n_loss_joints", C.c_int32),
        ("gmm_components", C.c_int32), ("gmm_dim", C.c_int32),
        ("gmm_means", C.POINTER(C.c_float)), ("gmm_precisions", C.POINTER(C.c_float)),
        ("gmm_nll_weights", C.POINTER(C.c_float)),
        ("n_faces", C.c_int32), ("faces", C.POINTER(C.c_int32)),
        ("model_kind", C.c_int32), ("pose_mean", C.POINTER(C.c_float)), ("n_hand_pca", C.c_int32),
        ("left_hand_components", C.POINTER(C.c_float)), ("right_hand_components", C.POINTER(C.c_float)),
        ("n_lmk_static", C.c_int32), ("lmk_faces_idx", C.POINTER(C.c_int32)), ("lmk_bary_coords", C.POINTER(C.c_float)),
        ("n_lmk_dynamic", C.c_int32), ("n_dyn_rows", C.c_int32), ("dynamic_lmk_faces_idx", C.POINTER(C.c_int32)),
        ("dynamic_lmk_bary_coords", C.POINTER(C.c_float)), ("neck_joint", C.c_int32),
    ]


class SmplxParams(C.Structure):          # bf_smplx_params
    _fields_ = [(n, C.POINTER(C.c_float)) for n in (
        "betas", "global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")]


class SmplxOutputs(C.Structure):         # bf_smplx_outputs
    _fields_ = [(n, C.POINTER(C.c_float)) for n in ("vertices", "joints", "joints_all", "full_pose")] + [("dyn_row", C.POINTER(C.c_int32))]


class SmplxCotangents(C.Structure):      # bf_smplx_cotangents
    _fields_ = [(n, C.POINTER(C.c_float)) for n in ("dvertices", "djoints", "djoints_all", "dfull_pose")]


class SmplxGrads(C.Structure):           # bf_smplx_grads
    _fields_ = [(n, C.POINTER(C.c_float)) for n in (
        "dbetas", "dglobal_orient", "dbody_pose", "djaw_pose", "dleye_pose", "dreye_pose", "dleft_hand_pose", "dright_hand_pose")]


class KeypointLossIn(C.Structure):      # bf_keypoint_loss_in
    _fields_ = [("n", C.c_int32), ("n_views", C.c_int32), ("n_rows", C.c_int32),
                ("joints", C.POINTER(C.c_float)), ("w2c", C.POINTER(C.c_float)), ("K", C.POINTER(C.c_float)),
                ("keypoints", C.POINTER(C.c_float)), ("present", C.POINTER(C.c_uint8)), ("divisor", C.POINTER(C.c_int32)),
                ("pose_dim", C.c_int32), ("poses", C.POINTER(C.c_float)), ("n_betas", C.c_int32), ("betas", C.POINTER(C.c_float))]


class Hyper(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "sigma", "pose_prior_weight", "angle_prior_weight", "shape_prior_weight", "constant_scale",
        "imsize", "lr", "lr_transl_scale", "adam_beta1", "adam_beta2", "adam_eps", "lr_displacement", "mask_cdist_form", "dense_after")]


CONTOUR_OPENCV_FIRST, CONTOUR_RASTER_FIRST, CONTOUR_LONGEST = 0, 1, 2
NEAREST_REFERENCE, NEAREST_FAST = 0, 1
DENSE_GRAD_LATE, DENSE_GRAD_SUBMODEL = 1, 2
FIT_DEFAULT, FIT_DENSE, FIT_NO_VERTICES, FIT_FETCH, FIT_RESET, FIT_GRAPH, FIT_NOTIME = 0, 1, 2, 4, 8, 16, 32

# every entry point include/bodyfit.h declares: name -> (restype, argtypes)
_FP = C.POINTER(C.c_float)
_IP = C.POINTER(C.c_int32)
_DP = C.POINTER(C.c_double)
_VP = C.c_void_p


class NrCameraDev(C.Structure):
    """bf_nr_camera_dev: K, R, t as device addresses (NULL: that one comes by value)"""
    _fields_ = [("K", _VP), ("R", _VP), ("t", _VP)]


SIGNATURES = {
    "bf_last_error": (C.c_char_p, []),
    "bf_version": (C.c_char_p, []),
    "bf_device_count": (C.c_int, []),
    "bf_hyper_default": (None, [C.POINTER(Hyper)]),
    "bf_model_create": (C.c_int, [C.POINTER(ModelDesc), C.c_int, C.POINTER(_VP)]),
    "bf_model_destroy": (None, [_VP]),
    "bf_model_n_params": (C.c_int, [_VP]),
    "bf_model_fit_instance": (C.c_int, [_VP]),
    "bf_model_sub_vertices": (C.c_int, [_VP, C.c_int, _IP]),
    "bf_device_cache_trim": (C.c_int64, [C.c_int]),
    "bf_batch_dense_timing": (C.c_int, [_VP, C.c_int, _FP]),
    "bf_batch_dense_resident": (C.c_int, [_VP]),
    "bf_smpl_forward": (C.c_int, [_VP, C.c_int, _FP, _FP, _FP, _FP, _FP, _FP]),
    "bf_model_forward": (C.c_int, [_VP, C.c_int, _FP, _FP, _FP]),
    "bf_smpl_vjp": (C.c_int, [_VP, C.c_int, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP]),
    "bf_smplx_forward": (C.c_int, [_VP, C.c_int, C.POINTER(SmplxParams), C.POINTER(SmplxOutputs)]),
    "bf_smplx_vjp": (C.c_int, [_VP, C.c_int, C.POINTER(SmplxParams), C.POINTER(SmplxCotangents), C.POINTER(SmplxGrads)]),
    "bf_model_set_expression": (C.c_int, [_VP, C.c_int, _FP]),
    "bf_model_n_expression": (C.c_int, [_VP]),
    "bf_model_set_shape_space": (C.c_int, [_VP, C.c_int, C.c_int, _FP]),
    "bf_model_n_betas": (C.c_int, [_VP]),
    "bf_model_shape_ext_wide": (C.c_int, [_VP]),
    "bf_smplx_forward_expr": (C.c_int, [_VP, C.c_int, C.POINTER(SmplxParams), _FP, C.POINTER(SmplxOutputs)]),
    "bf_smplx_vjp_expr": (C.c_int, [_VP, C.c_int, C.POINTER(SmplxParams), _FP, C.POINTER(SmplxCotangents), C.POINTER(SmplxGrads), _FP]),
    "bf_gmm_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _FP, _FP, _FP, C.POINTER(_VP)]),
    "bf_gmm_destroy": (None, [_VP]),
    "bf_keypoint_loss": (C.c_int, [C.c_int, _VP, C.POINTER(KeypointLossIn), C.POINTER(Hyper), _FP, _FP, _FP, _FP, _FP]),
    "bf_workspace_create": (C.c_int, [C.c_int, C.POINTER(_VP)]),
    "bf_workspace_destroy": (None, [_VP]),
    # the device route: (model,) workspace, stream, then the host call's arguments as device addresses
    "bf_smpl_forward_dev": (C.c_int, [_VP, _VP, _VP, C.c_int] + [_VP] * 6),
    "bf_smpl_vjp_dev": (C.c_int, [_VP, _VP, _VP, C.c_int] + [_VP] * 9),
    "bf_smplx_forward_dev": (C.c_int, [_VP, _VP, _VP, C.c_int, C.POINTER(SmplxParams), _VP, C.POINTER(SmplxOutputs)]),
    "bf_smplx_vjp_dev": (C.c_int, [_VP, _VP, _VP, C.c_int, C.POINTER(SmplxParams), _VP, C.POINTER(SmplxCotangents), C.POINTER(SmplxGrads), _VP]),
    "bf_keypoint_loss_dev": (C.c_int, [_VP, _VP, _VP, C.POINTER(KeypointLossIn), C.POINTER(Hyper)] + [_VP] * 5),
    "bf_device_pointer_check": (C.c_int, [C.c_int, _VP]),
    "bf_dev_route_stats": (C.c_int, [C.POINTER(C.c_int64)]),
    "bf_topo_create": (C.c_int, [C.c_int, C.c_int, C.c_int, _IP, C.POINTER(_VP)]),
    "bf_topo_destroy": (None, [_VP]),
    "bf_vertex_normals": (C.c_int, [_VP, _FP, _FP]),
    "bf_vertex_normals_vjp": (C.c_int, [_VP, _FP, _FP, _FP]),
    "bf_normal_laplacian": (C.c_int, [_VP, _FP, _FP, _FP]),
    "bf_scan_point_loss": (C.c_int, [_VP, C.c_int, _FP, _FP, _IP, _FP, _FP]),
    "bf_normal_loss": (C.c_int, [C.c_int, C.c_int, _FP, _FP, _FP, _FP]),
    # their device route: the host call's arguments as device addresses, then workspace, stream
    "bf_vertex_normals_dev": (C.c_int, [_VP] * 5),
    "bf_vertex_normals_vjp_dev": (C.c_int, [_VP] * 6),
    "bf_normal_laplacian_dev": (C.c_int, [_VP] * 6),
    "bf_scan_point_loss_dev": (C.c_int, [_VP, C.c_int] + [_VP] * 7),
    "bf_scan_nearest_dev": (C.c_int, [_VP, C.c_int] + [_VP] * 6),
    "bf_normal_loss_dev": (C.c_int, [C.c_int, C.c_int, _VP, _VP, C.c_int] + [_VP] * 5),
    "bf_scale_gradient_dev": (C.c_int, [C.c_int, C.c_int, _VP, _VP, C.c_int, _VP, _VP]),
    "bf_batch_create": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(_VP)]),
    "bf_batch_destroy": (None, [_VP]),
    "bf_batch_set_cameras": (C.c_int, [_VP, _FP, _FP]),
    "bf_batch_set_keypoints": (C.c_int, [_VP, _FP, _IP]),
    "bf_batch_set_init": (C.c_int, [_VP, _FP, _FP]),
    "bf_batch_stage_inputs": (C.c_int, [_VP, _FP, _IP, _FP, _FP]),
    "bf_batch_get_previous": (C.c_int, [_VP, _FP, _FP, _FP, _FP, _FP]),
    "bf_batch_reset": (C.c_int, [_VP]),
    "bf_batch_set_params": (C.c_int, [_VP, _FP]),
    "bf_batch_get_params": (C.c_int, [_VP, _FP]),
    "bf_fit": (C.c_int, [_VP, C.c_int, C.POINTER(Hyper), C.c_uint32]),
    "bf_loss_grad": (C.c_int, [_VP, C.POINTER(Hyper), _FP, _FP]),
    "bf_dense_iter_grad": (C.c_int, [_VP, C.POINTER(Hyper), C.c_uint32, _FP, _FP, _FP]),
    "bf_batch_sync": (C.c_int, [_VP]),
    "bf_batch_get_result": (C.c_int, [_VP, _FP, _FP, _FP, _FP]),
    "bf_batch_export_params_dev": (C.c_int, [_VP, _VP]),
    "bf_scan_create": (C.c_int, [C.c_int, C.c_int, _FP, C.c_int, _IP, C.POINTER(_VP)]),
    "bf_scan_destroy": (None, [_VP]),
    "bf_scan_height": (C.c_float, [_VP]),
    "bf_scan_grid_info": (C.c_int, [_VP, _IP, _FP]),
    "bf_scan_grid_lists": (C.c_int, [_VP, _IP, _IP, _IP]),
    "bf_scan_inside": (C.c_int, [_VP, C.c_int, _FP, _FP]),
    "bf_scan_intersects": (C.c_int, [_VP, C.c_int, _FP, _FP, C.POINTER(C.c_uint8)]),
    "bf_scan_nearest": (C.c_int, [_VP, C.c_int, _FP, _IP, _FP, _FP]),
    "bf_scan_nearest_hinted": (C.c_int, [_VP, C.c_int, _FP, _FP, _IP, _FP, _FP, C.c_int, _FP]),
    "bf_scan_nearest_backward": (C.c_int, [_VP, C.c_int, _IP, _FP, _FP, _FP]),
    "bf_batch_mesh_span": (C.c_int, [_VP, C.c_int, _FP]),
    "bf_nearest_rule_set": (C.c_int, [C.c_int]),
    "bf_nearest_rule_get": (C.c_int, []),
    "bf_mask_fold_set": (C.c_int, [C.c_int]),
    "bf_mask_fold_get": (C.c_int, []),
    "bf_nearest_selftest_quot": (C.c_int, [C.c_int, C.c_int, _FP, _FP, _FP]),
    "bf_nearest_selftest_rule": (C.c_int, [C.c_int, C.c_int, _FP, C.c_int, _FP, _FP]),
    "bf_batch_set_scans": (C.c_int, [_VP, C.POINTER(_VP)]),
    "bf_batch_set_masks": (C.c_int, [_VP, C.c_int, _IP, C.c_int, C.c_int, C.POINTER(C.c_uint8), _IP, _FP, C.c_int]),
    "bf_batch_stage_masks": (C.c_int, [_VP, C.c_int, _IP, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int]),
    "bf_extract_contours": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), _IP, _FP, C.c_int]),
    "bf_batch_mask_loss": (C.c_int, [_VP, C.POINTER(Hyper), _FP, _FP]),
    "bf_silhouette_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), _IP, _FP, C.c_int, C.POINTER(_VP)]),
    "bf_silhouette_destroy": (None, [_VP]),
    "bf_silhouette_contours": (C.c_int, [_VP, _IP, _FP]),
    "bf_silhouette_loss": (C.c_int, [_VP, C.c_int, C.c_int, _FP, _FP, _FP, C.c_float, C.c_float, C.c_int, _FP, _FP, _FP]),
    "bf_silhouette_create_dev": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _VP, C.c_int, C.c_int, _VP, C.POINTER(_VP)]),
    "bf_silhouette_contours_dev": (C.c_int, [_VP, _VP, _VP]),
    "bf_silhouette_rows_dev": (C.c_int, [C.c_int, C.c_int, _VP, _VP, _VP, _VP]),
    "bf_silhouette_loss_dev": (C.c_int, [_VP, C.c_int, C.c_int, _VP, _VP, _VP, C.c_float, C.c_float, C.c_int, _VP, _VP, _VP, _VP]),
    "bf_fit_displacement": (C.c_int, [_VP, C.c_int, C.POINTER(Hyper)]),
    "bf_batch_get_displacement": (C.c_int, [_VP, _FP]),
    "bf_batch_last_timing": (C.c_int, [_VP, _FP]),
    "bf_batch_timing_reset": (C.c_int, [_VP]),
    "bf_batch_timing_sum": (C.c_int, [_VP, _FP, _IP]),
    "bf_shard_range": (C.c_int, [C.c_int, C.c_int, C.c_int, _IP, _IP]),
    "bf_shard_capacity": (C.c_int, [C.c_int, C.c_int]),
    "bf_shard_unpack": (C.c_int, [_FP, C.c_int, C.c_int, C.c_int, _FP]),
    "bf_shard_contour_offsets": (C.c_int, [C.c_int, C.c_int, C.c_int, _IP, C.POINTER(C.c_int64)]),
    "bf_group_create": (C.c_int, [C.POINTER(ModelDesc), C.c_int, _IP, C.c_int, C.c_int, C.POINTER(_VP)]),
    "bf_group_destroy": (None, [_VP]),
    "bf_group_n_devices": (C.c_int, [_VP]),
    "bf_group_n_params": (C.c_int, [_VP]),
    "bf_group_shard": (C.c_int, [_VP, C.c_int, _IP, _IP, _IP]),
    "bf_group_batch": (_VP, [_VP, C.c_int]),
    "bf_group_model": (_VP, [_VP, C.c_int]),
    "bf_group_set_cameras": (C.c_int, [_VP, _FP, _FP]),
    "bf_group_set_keypoints": (C.c_int, [_VP, _FP, _IP]),
    "bf_group_set_init": (C.c_int, [_VP, _FP, _FP]),
    "bf_group_stage_inputs": (C.c_int, [_VP, _FP, _IP, _FP, _FP]),
    "bf_group_set_masks": (C.c_int, [_VP, C.c_int, _IP, C.c_int, C.c_int, C.POINTER(C.c_uint8), _IP, _FP, C.c_int]),
    "bf_group_stage_masks": (C.c_int, [_VP, C.c_int, _IP, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int]),
    "bf_group_set_scans": (C.c_int, [_VP, C.POINTER(_VP)]),
    "bf_group_fit": (C.c_int, [_VP, C.c_int, C.POINTER(Hyper), C.c_uint32]),
    "bf_group_fit_displacement": (C.c_int, [_VP, C.c_int, C.POINTER(Hyper)]),
    "bf_group_sync": (C.c_int, [_VP]),
    "bf_group_comm_size": (C.c_int, [_VP]),
    "bf_group_gather_params": (C.c_int, [_VP, _FP, C.c_int]),
    "bf_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "bf_comm_create": (C.c_int, [C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    "bf_comm_destroy": (None, [_VP]),
    "bf_comm_size": (C.c_int, [_VP]),
    "bf_comm_barrier": (C.c_int, [_VP]),
    "bf_comm_allreduce": (C.c_int, [_VP, C.POINTER(C.c_double), C.c_int]),
    "bf_comm_gather_params": (C.c_int, [_VP, _VP, C.c_int, _FP]),
    "bf_texfit_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _FP, C.c_int, C.POINTER(_VP)]),
    "bf_texfit_destroy": (None, [_VP]),
    "bf_texfit_set_mesh": (C.c_int, [_VP, C.c_int, C.c_int, _FP, C.c_int, _IP, _FP]),
    "bf_texfit_render": (C.c_int, [_VP, C.c_int, _FP, _FP, _FP, C.c_float, _FP]),
    "bf_texfit_render_ndc": (C.c_int, [_VP, C.c_int, _FP, C.c_int, _IP, _FP, _FP, _FP]),
    "bf_texfit_step": (C.c_int, [_VP, _FP, _FP, _FP, C.c_float, C.c_float, C.POINTER(C.c_double)]),
    "bf_texfit_loss_grad": (C.c_int, [_VP, _FP, _FP, _FP, C.c_float, C.POINTER(C.c_double), _FP]),
    "bf_texfit_get_textures": (C.c_int, [_VP, _FP]),
    "bf_texfit_render_depth": (C.c_int, [_VP, C.c_int, _FP, _FP, _FP, C.c_float, _FP, _FP]),
    "bf_texfit_load_textures": (C.c_int, [C.c_int, C.c_int, _FP, _IP, _FP, C.c_int, C.POINTER(C.c_void_p), _IP, _IP, C.c_int, C.c_int,
                                          C.c_int, _FP, _FP]),
    "bf_nr_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, _FP, C.POINTER(_VP)]),
    "bf_nr_destroy": (None, [_VP]),
    "bf_nr_set_light": (C.c_int, [_VP, C.c_float, C.c_float, _FP, _FP, _FP]),
    "bf_nr_mesh_create": (C.c_int, [_VP, C.c_int, _FP, C.c_int, _IP, C.c_int, _FP, C.POINTER(_VP)]),
    "bf_nr_mesh_set_textures": (C.c_int, [_VP, _FP]),
    "bf_nr_mesh_destroy": (None, [_VP]),
    "bf_nr_render": (C.c_int, [_VP, _VP, _FP, _FP, _FP, C.c_float, C.c_int, C.c_int, C.c_int, _FP, _FP, _FP, C.POINTER(_VP)]),
    "bf_nr_tape_texture_grad": (C.c_int, [_VP, _FP, _FP]),
    "bf_nr_tape_destroy": (None, [_VP]),
    "bf_nr_mesh_set_vertices": (C.c_int, [_VP, _FP]),
    "bf_nr_render_taped": (C.c_int, [_VP, _VP, _FP, _FP, _FP, C.c_float, C.c_int, C.c_int, C.c_int, _FP, _FP, _FP, C.c_int, C.POINTER(_VP)]),
    "bf_nr_tape_vertex_grad": (C.c_int, [_VP, _FP, _FP, _FP, _FP, _FP, _FP]),
    "bf_nr_render_dev": (C.c_int, [_VP, _VP, _FP, _FP, _FP, C.c_float, C.c_int, C.c_int, C.c_int, _VP, _VP, _VP, C.c_int, C.POINTER(_VP), _VP, _VP,
                                   C.POINTER(NrCameraDev), _VP, C.c_size_t, _VP, _VP]),
    "bf_nr_tape_texture_grad_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "bf_nr_tape_vertex_grad_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "bf_nr_tape_layout": (C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_uint64)]),
    "bf_nr_route_stats": (C.c_int, [C.POINTER(C.c_int64)]),
    "bf_hmr_n_weights": (C.c_int64, []),
    "bf_hmr_create": (C.c_int, [C.c_int, _FP, C.c_int64, _FP, C.c_int, C.POINTER(_VP)]),
    "bf_hmr_destroy": (None, [_VP]),
    "bf_hmr_predict": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), _FP, _FP, _FP]),
    "bf_hmr_features": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), _FP]),
    "bf_hmr_preprocess": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _FP]),
    "bf_hmr_selftest_conv": (C.c_int, [C.c_int] * 9 + [_FP, _FP, _FP, _FP, C.c_int, _FP]),
    "bf_openpose_n_weights": (C.c_int64, []),
    "bf_openpose_create": (C.c_int, [C.c_int, _FP, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    "bf_openpose_destroy": (None, [_VP]),
    "bf_openpose_maps": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), _DP, _DP]),
    "bf_openpose_network": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), _FP, _FP]),
    "bf_openpose_inject": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _FP, C.c_int64, _DP, _DP]),
    "bf_openpose_map_size": (C.c_int, [_VP, _IP]),
    "bf_openpose_peaks": (C.c_int, [_VP, C.c_int, C.c_int, _DP, _IP, _IP, _DP]),
    "bf_openpose_pairs": (C.c_int, [_VP, C.c_int, C.c_int, _IP, _DP, _IP]),
    "bf_openpose_selftest_conv": (C.c_int, [C.c_int] * 8 + [_FP, _FP, _FP, _FP]),
    "bf_openpose_hand_n_weights": (C.c_int64, []),
    "bf_openpose_hand_create": (C.c_int, [C.c_int, _FP, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    "bf_openpose_hand_destroy": (None, [_VP]),
    "bf_openpose_hand_maps": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, _IP, _DP]),
    "bf_openpose_hand_network": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, _IP, _FP, _FP]),
    "bf_openpose_hand_inject": (C.c_int, [_VP, C.c_int, _IP, _FP, C.c_int64, _DP]),
    "bf_openpose_hand_peaks": (C.c_int, [_VP, C.c_int, _DP, _IP, _DP, _IP]),
    "bf_openpose_hand_selftest_label": (C.c_int, [C.c_int] * 4 + [C.POINTER(C.c_uint8), _IP, _IP]),
    "bf_views_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    "bf_views_destroy": (None, [_VP]),
    "bf_views_bbox": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), _IP]),
    "bf_views_prepare": (C.c_int, [_VP, C.c_int, _IP, C.POINTER(C.c_void_p), _IP, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                                   C.POINTER(C.c_int64)]),
    "bf_views_last_timing": (C.c_int, [_VP, _FP, C.POINTER(C.c_int64)]),
    "bf_inpaint_n_weights": (C.c_int64, []),
    "bf_inpaint_create": (C.c_int, [C.c_int, _FP, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(_VP)]),
    "bf_inpaint_destroy": (None, [_VP]),
    "bf_inpaint_run": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _FP]),
    "bf_inpaint_hole_mask": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, _FP, C.POINTER(C.c_uint8)]),
    "bf_inpaint_texture": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, _FP, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "bf_morph_u8": (C.c_int, [C.c_int] * 7 + [C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "bf_inpaint_select_faces": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, _FP, C.POINTER(C.c_uint8)]),
    "bf_inpaint_selftest_conv": (C.c_int, [C.c_int] * 7 + [_FP] * 6),
    "bf_overlay_stamp": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_int, _FP, _DP, C.POINTER(C.c_uint8)]),
    "bf_batch_debug_dump": (C.c_int, [_VP, _FP, C.c_int]),
    "bf_batch_debug_disp_moment": (C.c_int, [_VP, _FP]),
    "bf_batch_debug_disp_moment2": (C.c_int, [_VP, _FP]),
    "bf_batch_debug_vertices": (C.c_int, [_VP, _FP]),
    "bf_batch_lane_stats": (C.c_int, [_VP, _IP]),
    "bf_batch_lane_feed_stats": (C.c_int, [_VP, C.POINTER(C.c_int64)]),
}

# entry points of the frame loop bound a second time with plain addresses for their array arguments (native.conforming_address): an
# integer converts in a fraction of the time an ndarray's ctypes.data_as() takes
ADDRESS_SIGNATURES = {
    "bf_batch_stage_inputs": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "bf_group_stage_inputs": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
}
_by_address = {}

_lib = None


def load():
    """Return the loaded library; raise BodyfitError (never fall back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BodyfitError(
            f"{LIB_PATH} is missing - build it with `make -C bodyfitting_amd/csrc` (or "
            "`python -c 'import __graft_entry__ as g; g.build()'`).  There is no CPU fallback.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise BodyfitError(f"could not load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in ADDRESS_SIGNATURES.items():
        _by_address[name] = C.CFUNCTYPE(res, *args)((name, lib))
    _lib = lib
    return lib


def by_address(name):
    """the entry point `name` of ADDRESS_SIGNATURES taking integer addresses"""
    load()
    return _by_address[name]


def check(rc, what=""):
    if rc != 0:
        msg = load().bf_last_error().decode("utf-8", "replace")
        raise BodyfitError(f"{what or 'libbodyfit'} failed ({rc}): {msg}")


def fptr(a):
    return a.ctypes.data_as(_FP) if a is not None else None


def iptr(a):
    return a.ctypes.data_as(_IP) if a is not None else None


def at(address, kind=_FP):
    """a device address (an integer; 0 / None: NULL) as the pointer type a struct field of the ABI takes"""
    return C.cast(C.c_void_p(address), kind) if address else None
