"""ctypes binding of libactmi.so (C ABI declared in include/actmi.h).

There is NO CPU fallback: if the HIP library is missing or a call fails, a RuntimeError is raised.
torch is imported before the library so that libactmi's ``libamdhip64.so.7`` dependency resolves (by SONAME)
to the one HIP runtime already loaded by PyTorch-ROCm; device pointers and streams are then shared.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must be loaded first, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
# ACTMI_LIB: another build of the library (A/B runs of two builds on one GPU box: tools/ab_bench.sh); default: the in-tree one
LIB_PATH = os.environ.get("ACTMI_LIB") or os.path.join(_HERE, "libactmi.so")

IMG_U8_NHWC = 0
IMG_F32_NCHW = 1


class ActmiConfig(C.Structure):
    # struct_size first: the ABI guard of include/actmi.h (actmi_create rejects a binding whose struct differs)
    _fields_ = [("struct_size", C.c_uint32)] + [(n, C.c_int32) for n in (
        "num_cams", "image_h", "image_w", "base_width", "hidden_dim", "nheads", "dim_feedforward", "enc_layers",
        "dec_layers", "num_queries", "state_dim", "action_dim", "latent_dim", "has_cvae_encoder", "max_batch",
        "enable_training")] + [("kl_weight", C.c_float)] + [(n, C.c_int32) for n in ("vq", "vq_class", "vq_dim")]


class ActmiPcdConfig(C.Structure):
    # the point-cloud branch of a handle (actmi_create_ex); struct_size guards it like ActmiConfig's
    _fields_ = [("struct_size", C.c_uint32), ("max_points", C.c_int32), ("hidden_dim", C.c_int32), ("output_dim", C.c_int32)]


class ActmiDepthConfig(C.Structure):
    # the depth cameras of a handle (actmi_create_ex2); struct_size guards it like ActmiConfig's
    _fields_ = [("struct_size", C.c_uint32), ("num_depth_cams", C.c_int32)]


class GemmDesc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("lda", C.c_int64), ("mode", C.c_int32),
        ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("KH", C.c_int32), ("KW", C.c_int32),
        ("stride", C.c_int32), ("pad", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32),
        ("img_stride", C.c_int64),
        ("A_add", C.c_void_p), ("ld_add", C.c_int64), ("add_mod", C.c_int32), ("add_ncols", C.c_int32),
        ("Bw", C.c_void_p), ("ldb", C.c_int64),
        ("scale", C.c_void_p), ("bias", C.c_void_p), ("res", C.c_void_p), ("ldres", C.c_int64),
        ("res_mod", C.c_int32), ("relu", C.c_int32),
        ("C", C.c_void_p), ("ldc", C.c_int64), ("rowmap", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("groups", C.c_int32),
        ("gA", C.c_int64), ("gB", C.c_int64), ("gSB", C.c_int64), ("gC", C.c_int64), ("gRes", C.c_int64),
        ("ta", C.c_int32), ("tb", C.c_int32), ("a_rowmap", C.c_void_p),
        ("B_add", C.c_void_p), ("ld_badd", C.c_int64), ("badd_mod", C.c_int32), ("splitk", C.c_int32),
        ("mask", C.c_void_p), ("ldmask", C.c_int64), ("C2", C.c_void_p), ("scale2", C.c_void_p),
        ("alpha", C.c_float), ("groups_inner", C.c_int32),
        ("gA2", C.c_int64), ("gB2", C.c_int64), ("gC2", C.c_int64), ("gRes2", C.c_int64),
        ("gMask", C.c_int64), ("gC2out", C.c_int64),
        ("drop_p", C.c_float), ("drop_seed", C.c_uint64), ("stamps", C.c_void_p), ("prec", C.c_int32), ("b_split", C.c_int32), ("b_scale", C.c_float), ("a_scale", C.c_float), ("a_scale_dev", C.c_void_p), ("b_scale_dev", C.c_void_p),
        ("split_stride", C.c_int64), ("amax_out", C.c_void_p),
        ("epi", C.c_int32), ("epi_scale", C.c_float), ("epi_row", C.c_void_p), ("gRow", C.c_int64), ("gRow2", C.c_int64),
        ("epi_colkill", C.c_void_p), ("gColkill", C.c_int64), ("tile_hint", C.c_int32),
        ("finite_flag", C.c_void_p), ("finite_bit", C.c_uint32),
        ("Ax", C.c_void_p), ("kx_begin", C.c_int32), ("Hx", C.c_int32), ("Wx", C.c_int32), ("Cx", C.c_int32),
        ("stride_x", C.c_int32), ("gAx", C.c_int64),
        ("A_alt", C.c_void_p), ("alt_ncols", C.c_int32), ("k_tap_inner", C.c_int32),
    ]


class AttnBwdDesc(C.Structure):
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("o", C.c_void_p), ("d_o", C.c_void_p), ("lse", C.c_void_p),
                ("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p)] + \
               [(n, C.c_int64) for n in ("q_bs", "q_rs", "k_bs", "k_rs", "v_bs", "v_rs", "dq_bs", "dq_rs", "dk_bs", "dk_rs", "dv_bs", "dv_rs")] + \
               [("kpm", C.c_void_p), ("kpm_bs", C.c_int64)] + [(n, C.c_int32) for n in ("B", "H", "Nq", "Nk", "HD")] + \
               [("drop_p", C.c_float), ("drop_seed", C.c_uint64), ("delta_ws", C.c_void_p), ("do_scale", C.c_void_p), ("amax_out", C.c_void_p)]


class AttnDesc(C.Structure):
    _fields_ = [
        ("Q", C.c_void_p), ("q_bs", C.c_int64), ("q_rs", C.c_int64),
        ("K", C.c_void_p), ("k_bs", C.c_int64), ("k_rs", C.c_int64),
        ("V", C.c_void_p), ("v_bs", C.c_int64), ("v_rs", C.c_int64),
        ("O", C.c_void_p), ("o_bs", C.c_int64), ("o_rs", C.c_int64),
        ("kpm", C.c_void_p), ("kpm_bs", C.c_int64), ("lse", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("Nq", C.c_int32), ("Nk", C.c_int32), ("HD", C.c_int32),
        ("scale", C.c_float), ("ws", C.c_void_p), ("ws_floats", C.c_int64),
        ("drop_p", C.c_float), ("drop_seed", C.c_uint64), ("prec", C.c_int32), ("causal", C.c_int32),
    ]


class AttnLayout(C.Structure):
    # actmi_attn_layout: the token order of the decoder's cross-attention map
    _fields_ = [(k, C.c_int32) for k in ("Q", "N", "n_extra", "K", "Kd", "fh", "fw", "rgb0", "depth0")]


RGBD_MAX_CAMS = 8


class RgbdCam(C.Structure):
    # one fusion camera of the device parameter block (actmi_rgbd_cam): 20 words
    _fields_ = [("cam_index", C.c_int32), ("quota", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("depth_scale", C.c_float), ("T", C.c_float * 12), ("reserved", C.c_float)]


class RgbdCalib(C.Structure):
    _fields_ = [("cam", RgbdCam * RGBD_MAX_CAMS), ("box", C.c_float * 6), ("reserved", C.c_float * 2)]


class RgbdDesc(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("image", C.c_void_p), ("calib", C.c_void_p), ("seed", C.c_void_p), ("xyz", C.c_void_p),
                ("rgb", C.c_void_p), ("n", C.c_void_p), ("src_idx", C.c_void_p), ("survivors", C.c_void_p), ("ws", C.c_void_p),
                ("ws_bytes", C.c_int64)] + [(k, C.c_int32) for k in ("B", "K", "C", "H", "W", "P")] + \
               [("quota", C.c_int32 * RGBD_MAX_CAMS), ("cam_index", C.c_int32 * RGBD_MAX_CAMS)]


RGBD_FPS_MAX_POOL = 16384      # ACTMI_RGBD_FPS_MAX_POOL


class RgbdFpsDesc(C.Structure):
    # actmi_rgbd_fps_desc: the key draw's descriptor, the candidate pool per camera, the optional pick-order output
    _fields_ = [("base", RgbdDesc), ("pool", C.c_int32), ("reserved", C.c_int32), ("order", C.c_void_p)]


class AugmentRecord(C.Structure):
    # actmi_augment_record: the device parameter record of one sample, 32 bytes
    _fields_ = [("top", C.c_int32), ("left", C.c_int32), ("order", C.c_int32), ("cos", C.c_float), ("sin", C.c_float),
                ("fb", C.c_float), ("fc", C.c_float), ("fs", C.c_float)]


class AugmentDesc(C.Structure):
    # actmi_augment_desc: actmi_op_augment_u8 and actmi_op_warp_u16 take the same descriptor
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("records", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_int64)] + \
               [(k, C.c_int32) for k in ("B", "K", "H", "W", "ch", "cw")]


class CloudAugmentRecord(C.Structure):
    # actmi_cloud_augment_record: the device parameter record of one sample, 56 bytes
    _fields_ = [(k, C.c_float) for k in ("cos", "sin", "scale", "tx", "ty", "tz", "jitter", "drop", "fb", "fc", "fs")] + \
               [("order", C.c_int32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32)]


class CloudAugmentDesc(C.Structure):
    # actmi_cloud_augment_desc
    _fields_ = [(k, C.c_void_p) for k in ("xyz", "rgb", "counts", "records", "out_xyz", "out_rgb", "out_counts")] + \
               [("pivot", C.c_float * 3), ("B", C.c_int32), ("P", C.c_int32)]


class EpisodeRec(C.Structure):
    # actmi_episode_rec: one entry of the device episode table, 16 bytes
    _fields_ = [("row0", C.c_int64), ("T", C.c_int32), ("is_sim", C.c_int32)]


class GatherChunksDesc(C.Structure):
    # actmi_gather_chunks_desc
    _fields_ = [(k, C.c_void_p) for k in ("actions", "qpos", "episodes", "samples", "action_mean", "action_std", "qpos_mean",
                                          "qpos_std", "qpos_out", "action_out", "is_pad")] + \
               [("n_rows", C.c_int64)] + [(k, C.c_int32) for k in ("n_episodes", "B", "A", "S", "Q")]


class GatherMirrorDesc(C.Structure):
    # actmi_gather_mirror_desc
    _fields_ = [("arena", C.c_void_p), ("arena_bytes", C.c_int64), ("src_off", C.c_void_p), ("flip", C.c_void_p), ("out", C.c_void_p),
                ("n_items", C.c_int64)] + [(k, C.c_int32) for k in ("H", "W", "px_bytes", "aligned")]


class CloudItem(C.Structure):
    # actmi_cloud_item: the device record of one sample of actmi_op_gather_clouds, 32 bytes
    _fields_ = [("xyz_off", C.c_int64), ("rgb_off", C.c_int64)] + [(k, C.c_int32) for k in ("rows", "n", "flags", "pad")]


class GatherCloudsDesc(C.Structure):
    # actmi_gather_clouds_desc
    _fields_ = [("arena", C.c_void_p), ("arena_bytes", C.c_int64), ("items", C.c_void_p), ("out_xyz", C.c_void_p), ("out_rgb", C.c_void_p),
                ("out_n", C.c_void_p)] + [(k, C.c_int32) for k in ("B", "P", "rgb_fmt", "mirror_axis")] + \
               [("mirror_c2", C.c_float), ("aligned", C.c_int32)]


class JpegDesc(C.Structure):
    # actmi_jpeg_desc
    _fields_ = [("stream", C.c_void_p), ("stream_bytes", C.c_int64), ("frames", C.c_void_p), ("tables", C.c_void_p), ("dst", C.c_void_p),
                ("dst_bytes", C.c_int64), ("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("status", C.c_void_p)] + \
               [(k, C.c_int32) for k in ("n", "n_tables", "H", "W", "mode", "form")]


class JpegEncDesc(C.Structure):
    # actmi_jpeg_enc_desc
    _fields_ = [("src", C.c_void_p), ("src_bytes", C.c_int64), ("frames", C.c_void_p), ("dst", C.c_void_p), ("dst_bytes", C.c_int64),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("seg_len", C.c_void_p), ("status", C.c_void_p), ("q", C.c_uint16 * 64 * 2)] + \
               [(k, C.c_int32) for k in ("n", "H", "W", "mode", "form")]


class DepthPackDesc(C.Structure):
    # actmi_depth_pack_desc
    _fields_ = [("src", C.c_void_p), ("src_bytes", C.c_int64), ("frames", C.c_void_p), ("dst", C.c_void_p), ("dst_bytes", C.c_int64),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("seg_len", C.c_void_p), ("status", C.c_void_p)] + \
               [(k, C.c_int32) for k in ("n", "H", "W", "reserved")]


class DepthUnpackDesc(C.Structure):
    # actmi_depth_unpack_desc
    _fields_ = [("stream", C.c_void_p), ("stream_bytes", C.c_int64), ("frames", C.c_void_p), ("dst", C.c_void_p), ("dst_bytes", C.c_int64),
                ("status", C.c_void_p), ("sticky", C.c_void_p)] + [(k, C.c_int32) for k in ("n", "H", "W", "reserved")]


class JpegMarks(C.Structure):
    # actmi_jpeg_marks
    _fields_ = [("marks", C.c_void_p), ("n_marks", C.c_int64), ("first", C.c_void_p), ("sticky", C.c_void_p), ("rows_per_mark", C.c_int32),
                ("reserved", C.c_int32)]


_lib = None


def load():
    """Load libactmi.so; raise loudly when it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C act-plus-plus_amd/csrc). There is no CPU fallback for the ACT path.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
    sigs = {
        "actmi_version": ([], i32),
        "actmi_create": ([C.POINTER(ActmiConfig), C.POINTER(vp)], i32),
        "actmi_create_ex": ([C.POINTER(ActmiConfig), C.POINTER(ActmiPcdConfig), C.POINTER(vp)], i32),
        "actmi_set_pointcloud": ([vp, vp, vp, i32, i32], i32),
        "actmi_set_pointcloud_n": ([vp, vp, vp, vp, i32, i32], i32),
        "actmi_create_ex2": ([C.POINTER(ActmiConfig), C.POINTER(ActmiPcdConfig), C.POINTER(ActmiDepthConfig), C.POINTER(vp)], i32),
        "actmi_set_depth": ([vp, vp, i32], i32),
        "actmi_set_depth_u16": ([vp, vp, i32], i32),
        "actmi_destroy": ([vp], i32),
        "actmi_last_error": ([vp], C.c_char_p),
        "actmi_num_params": ([vp], i32),
        "actmi_param_info": ([vp, i32, C.POINTER(C.c_char_p), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)], i32),
        "actmi_set_param": ([vp, C.c_char_p, vp, C.POINTER(i64), i32, i32], i32),
        "actmi_get_param": ([vp, C.c_char_p, vp, i64, i32], i32),
        "actmi_param_ptr": ([vp, C.c_char_p, C.POINTER(vp), C.POINTER(i64)], i32),
        "actmi_finalize": ([vp, vp], i32),
        "actmi_set_forward_phase": ([vp, i32], i32),
        "actmi_forward_infer_vq": ([vp, vp, vp, i32, i32, vp, vp, vp], i32),
        "actmi_forward_infer": ([vp, vp, vp, i32, i32, vp, vp], i32),
        "actmi_forward_train": ([vp, vp, vp, i32, vp, vp, vp, C.c_uint64, f32, i32, vp, vp, vp, vp, vp], i32),
        "actmi_backward": ([vp, f32, vp], i32),
        "actmi_zero_grad": ([vp, vp], i32),
        "actmi_adamw_step": ([vp, f32, f32, f32, f32, f32, f32, i64, vp], i32),
        "actmi_adamw_step_range": ([vp, f32, f32, f32, f32, f32, f32, i64, i64, i64, vp], i32),
        "actmi_refresh_weights": ([vp, vp], i32),
        "actmi_param_arena": ([vp, C.POINTER(vp), C.POINTER(i64)], i32),
        "actmi_grad_ptr": ([vp, C.c_char_p, C.POINTER(vp), C.POINTER(i64)], i32),
        "actmi_grad_arena": ([vp, C.POINTER(vp), C.POINTER(i64)], i32),
        "actmi_grad_phase_range": ([vp, i32, C.POINTER(i64), C.POINTER(i64)], i32),
        "actmi_wait_grad_phase": ([vp, i32, vp], i32),
        "actmi_ensemble_step": ([vp, vp, vp, f64, vp, vp, i32, i32, i32, vp], i32),
        "actmi_op_ensemble_episode": ([vp, vp, f64, vp, vp, i32, i32, i32, i32, vp], i32),
        "actmi_op_action_error": ([vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp], i32),
        "actmi_op_chunk_error": ([vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp], i32),
        "actmi_op_ensemble_sweep": ([vp, i32, vp, vp, vp, i32, i32, i32, i32, vp], i32),
        "actmi_op_sweep_error": ([vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, vp], i32),
        "actmi_op_gemm": ([C.POINTER(GemmDesc), vp], i32),
        "actmi_op_split16": ([vp, vp, C.c_int64, C.c_float, vp], i32),
        "actmi_op_permute_conv_k": ([vp, vp, C.c_int64, i32, i32, i32, vp], i32),
        "actmi_op_sample_onehot": ([vp, i32, i32, C.c_float, C.c_uint64, vp, vp, vp], i32),
        "actmi_op_pow2_scale": ([vp, C.c_int64, i32, i32, vp, vp], i32),
        "actmi_op_splitk_combine": ([vp, i32, C.c_int64, C.c_int64, i32, i32, vp, vp, vp, C.c_int64, i32, vp, C.c_int64, vp], i32),
        "actmi_op_attention": ([C.POINTER(AttnDesc), vp], i32),
        "actmi_op_attn_weights": ([C.POINTER(AttnDesc), vp, i64, i64, vp], i32),
        "actmi_op_heat_overlay_u8": ([vp, vp, vp, f32, vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
        "actmi_bind_attention_out": ([vp, vp, i32], i32),
        "actmi_attention_layout": ([vp, C.POINTER(AttnLayout)], i32),
        "actmi_bind_features_out": ([vp, vp, i32], i32),
        "actmi_op_knn_workspace_bytes": ([i64, i64], i64),
        "actmi_op_knn_topk": ([vp, vp, vp, vp, vp, vp, f32, i32, i64, i64, i32, i32, vp, vp, vp, vp, i64, vp], i32),
        "actmi_op_knn_predict": ([vp, vp, vp, i32, i32, vp, i64, vp, vp, i64, i32, i32, vp, vp, vp, vp, i64, vp], i32),
        "actmi_op_knn_ksweep": ([vp, vp, vp, i32, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, i64, vp], i32),
        "actmi_op_attention_bwd": ([C.POINTER(AttnBwdDesc), vp], i32),
        "actmi_op_layernorm": ([vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, f32, vp], i32),
        "actmi_op_layernorm_ex": ([vp, i32, i64, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, C.c_uint32, i32, i32,
                                   f32, vp], i32),
        "actmi_op_maxpool3x3s2": ([vp, vp, i32, i32, i32, i32, vp], i32),
        "actmi_op_conv1": ([vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
        "actmi_op_conv1_depth": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
        "actmi_op_depth_minmax_u16": ([vp, vp, i32, i64, vp], i32),
        "actmi_op_conv1_depth_u16": ([vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
        "actmi_op_conv1_workspace_floats": ([i32, i32], C.c_int64),
        "actmi_op_conv1_prepare": ([vp, vp, i32, i32, i32, vp], i32),
        "actmi_op_conv1_prepared": ([vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
        "actmi_op_conv1_prepared_ex": ([vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp], i32),
        "actmi_op_conv1_seam_floats": ([i32, i32, i32, i32, i32], C.c_int64),
        "actmi_op_conv1_pooled": ([vp, i32, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp], i32),
        "actmi_op_hpool": ([vp, vp, i32, i32, i32, vp], i32),
        "actmi_op_conv3x3_c64": ([vp, vp, C.c_float, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
        "actmi_op_conv3x3_c64_dgrad": ([vp, vp, C.c_float, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp], i32),
        "actmi_op_wgrad7x7s2": ([vp, vp, vp, vp, C.c_int64, vp, i32, i32, i32, i32, vp], i32),
        "actmi_op_wgrad3x3_c64": ([vp, vp, vp, vp, C.c_int64, vp, i32, i32, i32, i32, vp], i32),
        "actmi_op_wgrad7x7s2_ex": ([vp, vp, vp, vp, C.c_int64, vp, i32, i32, i32, i32, i32, vp], i32),
        "actmi_op_wgrad3x3_c64_ex": ([vp, vp, vp, vp, C.c_int64, vp, i32, i32, i32, i32, i32, vp], i32),
        "actmi_op_groupnorm": ([vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, i32, i32, vp, C.c_int64, vp], i32),
        "actmi_op_spatial_softmax": ([vp, vp, i32, i32, i32, i32, f32, vp], i32),
        "actmi_op_unfold1d": ([vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp], i32),
        "actmi_op_ddim_step": ([vp, vp, C.c_int64, f32, f32, f32, f32, i32, vp], i32),
        "actmi_op_mish": ([vp, vp, C.c_int64, vp], i32),
        "actmi_op_gelu": ([vp, vp, C.c_int64, vp], i32),
        "actmi_op_gelu_bwd": ([vp, vp, vp, C.c_int64, vp], i32),
        "actmi_op_dropout": ([vp, vp, C.c_int64, C.c_float, C.c_uint64, vp], i32),
        "actmi_op_small_attention": ([vp, vp, i32, i32, i32, i32, i32, C.c_float, C.c_uint64, vp], i32),
        "actmi_op_small_attention_bwd": ([vp, vp, vp, i32, i32, i32, i32, i32, C.c_float, C.c_uint64, vp], i32),
        "actmi_op_soft_ce_dim1": ([vp, vp, i32, i32, i32, vp, vp, vp, vp], i32),
        "actmi_op_argmax_l1": ([vp, vp, i32, i32, vp, vp, vp], i32),
        "actmi_op_layernorm_bwd": ([vp, vp, vp, vp, vp, vp, vp, i32, i32, C.c_float, vp, C.c_int64, vp], i32),
        "actmi_op_colsum": ([vp, C.c_int64, vp, i32, i32, vp, C.c_int64, vp], i32),
        "actmi_op_pcd_embed": ([vp, vp, vp, vp, vp, C.c_int64, i32, vp], i32),
        "actmi_op_colmax": ([vp, i32, i32, i32, C.c_int64, vp, vp, vp, C.c_int64, vp], i32),
        "actmi_op_colmax_n": ([vp, i32, i32, i32, C.c_int64, vp, vp, vp, vp, C.c_int64, vp], i32),
        "actmi_op_rgbd_cloud_workspace_bytes": ([i32, i32, i32, i32], C.c_int64),
        "actmi_op_rgbd_cloud": ([C.POINTER(RgbdDesc), vp], i32),
        "actmi_op_rgbd_cloud_fps_workspace_bytes": ([i32, i32, i32, i32, i32], C.c_int64),
        "actmi_op_rgbd_cloud_fps": ([C.POINTER(RgbdFpsDesc), vp], i32),
        "actmi_op_augment_workspace_bytes": ([i32, i32, i32, i32], C.c_int64),
        "actmi_op_augment_u8": ([C.POINTER(AugmentDesc), vp], i32),
        "actmi_op_warp_u16": ([C.POINTER(AugmentDesc), vp], i32),
        "actmi_op_cloud_augment": ([C.POINTER(CloudAugmentDesc), vp], i32),
        "actmi_op_gather_frames": ([vp, i64, vp, vp, i64, i64, i32, vp], i32),
        "actmi_op_gather_frames_mirror": ([C.POINTER(GatherMirrorDesc), vp], i32),
        "actmi_op_gather_clouds": ([C.POINTER(GatherCloudsDesc), vp], i32),
        "actmi_op_gather_chunks": ([C.POINTER(GatherChunksDesc), vp], i32),
        "actmi_op_jpeg_workspace_bytes": ([i64, i32, i32, i32], i64),
        "actmi_op_jpeg_decode": ([C.POINTER(JpegDesc), vp], i32),
        "actmi_jpeg_decode_host": ([C.POINTER(JpegDesc)], i32),
        "actmi_op_jpeg_index": ([C.POINTER(JpegDesc), C.POINTER(JpegMarks), vp], i32),
        "actmi_jpeg_index_host": ([C.POINTER(JpegDesc), C.POINTER(JpegMarks)], i32),
        "actmi_op_jpeg_decode_marked": ([C.POINTER(JpegDesc), C.POINTER(JpegMarks), vp], i32),
        "actmi_jpeg_decode_marked_host": ([C.POINTER(JpegDesc), C.POINTER(JpegMarks)], i32),
        "actmi_op_jpeg_encode_workspace_bytes": ([i64, i32, i32, i32], i64),
        "actmi_jpeg_encode_bound": ([i32, i32, i32], i64),
        "actmi_op_jpeg_encode": ([C.POINTER(JpegEncDesc), vp], i32),
        "actmi_jpeg_encode_host": ([C.POINTER(JpegEncDesc)], i32),
        "actmi_op_jpeg_encode_marked": ([C.POINTER(JpegEncDesc), C.POINTER(JpegMarks), vp], i32),
        "actmi_jpeg_encode_marked_host": ([C.POINTER(JpegEncDesc), C.POINTER(JpegMarks)], i32),
        "actmi_depth_pack_bound": ([i32, i32], i64),
        "actmi_op_depth_pack_workspace_bytes": ([i64, i32], i64),
        "actmi_op_depth_pack": ([C.POINTER(DepthPackDesc), vp], i32),
        "actmi_depth_pack_host": ([C.POINTER(DepthPackDesc)], i32),
        "actmi_op_depth_unpack": ([C.POINTER(DepthUnpackDesc), vp], i32),
        "actmi_depth_unpack_host": ([C.POINTER(DepthUnpackDesc)], i32),
        "actmi_op_sum_batch": ([vp, C.c_int64, C.c_int64, vp, i32, i32, i32, i32, vp], i32),
        "actmi_op_adamw": ([vp, vp, vp, vp, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int64, vp], i32),
        "actmi_op_u8_to_nhwc4": ([vp, vp, i32, i32, i32, i32, vp], i32),
        "actmi_op_maxpool3x3s2_idx": ([vp, vp, vp, i32, i32, i32, i32, vp], i32),
        "actmi_op_maxpool3x3s2_bwd": ([vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, vp, vp], i32),
        "actmi_op_relu_bn_bwd": ([vp, vp, vp, vp, vp, vp, i32, i64, i32, vp, vp], i32),
        "actmi_op_act_losses": ([vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, f32, vp], i32),
        "actmi_op_l1_bwd": ([vp, vp, vp, vp, i32, i32, i32, f32, vp], i32),
        "actmi_op_reparam": ([vp, vp, vp, vp, vp, i32, i32, vp], i32),
        "actmi_op_reparam_kl_bwd": ([vp, vp, vp, vp, i32, i32, f32, vp], i32),
        "actmi_op_vq_bwd": ([vp, vp, vp, i32, i32, i32, vp], i32),
        "actmi_op_dropout_bwd": ([vp, vp, i64, f32, C.c_uint64, vp], i32),
        "actmi_op_attn_delta": ([vp, vp, vp, i32, i32, i32, i32, vp], i32),
        "actmi_op_attn_drop": ([vp, vp, C.c_uint64, f32, i32, i32, i32, i32, vp], i32),
        "actmi_op_attn_ds_drop": ([vp, vp, vp, f32, C.c_uint64, f32, i32, i32, i32, i32, vp], i32),
        "actmi_op_zero_cols": ([vp, i64, i32, i32, vp], i32),
        "actmi_op_adamw_groups": ([vp, vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, f32, i64, vp, C.c_uint32, vp], i32),
        "actmi_op_layernorm_bwd_ex": ([vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp, i64, vp, vp], i32),
        "actmi_op_last_error": ([], C.c_char_p),
        "actmi_debug_tensor": ([vp, C.c_char_p, C.POINTER(vp), C.POINTER(i64)], i32),
        "actmi_debug_stop_after": ([vp, C.c_char_p], i32),
        "actmi_set_gemm_prec": ([vp, i32], i32),
        "actmi_set_train_prec": ([vp, i32], i32),
        "actmi_get_flags": ([vp, C.POINTER(C.c_uint32), i32, vp], i32),
        "actmi_flags_ptr": ([vp, C.POINTER(vp)], i32),
        "actmi_profile_enable": ([i32], i32),
        "actmi_profile_reset": ([], i32),
        "actmi_profile_report": ([C.c_char_p, i32], i32),
    }
    for name, (args, res) in sigs.items():
        if os.environ.get("ACTMI_LIB") and not hasattr(lib, name):
            continue                     # an A/B run against an older build: it lacks the newer entries (calling one fails there)
        fn = getattr(lib, name)          # AttributeError here = header and library disagree
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def declared_symbols(header_path):
    """Names of every function declared in include/actmi.h (used by the no-GPU export test)."""
    import re
    txt = open(header_path).read()
    return sorted(set(re.findall(r"\b(actmi_[a-z0-9_]+)\s*\(", txt)))


def current_stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, handle=None, what=""):
    if rc != 0:
        lib = load()
        msg = lib.actmi_last_error(handle) if handle is not None else lib.actmi_op_last_error()
        raise RuntimeError(f"libactmi {what} failed (code {rc}): {msg.decode() if msg else ''}")


def profile_enable(on: bool):
    lib = load()
    lib.actmi_profile_reset() if on else None
    lib.actmi_profile_enable(1 if on else 0)


def profile_report():
    """-> list of {name,count,ms,flops,bytes}; synchronises the recorded events."""
    import json
    lib = load()
    buf = C.create_string_buffer(1 << 18)
    rc = lib.actmi_profile_report(buf, len(buf))
    if rc != 0:
        raise RuntimeError(f"actmi_profile_report failed ({rc})")
    return json.loads(buf.value.decode())
