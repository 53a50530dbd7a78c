"""ctypes binding of the C ABI in include/f5h.h (libf5h.so, gfx950).

torch is imported first on purpose: torch ships its own libamdhip64.so (SONAME
libamdhip64.so.7); libf5h.so's NEEDED entry then resolves to that already-loaded
runtime, so torch's device pointers and streams are valid inside the engine.

There is no fallback: if the library is missing or cannot load, every engine
entry point raises (the product path never drops to PyTorch or to the oracle).
"""

from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL load, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("F5H_LIB", os.path.join(_HERE, "lib", "libf5h.so"))

F5H_DIT, F5H_UNETT, F5H_MMDIT = 0, 1, 2
BACKBONE = {"DiT": F5H_DIT, "UNetT": F5H_UNETT, "MMDiT": F5H_MMDIT}
F5H_FP32, F5H_BF16, F5H_FP16, F5H_MXFP8 = 0, 1, 2, 3
# "mxfp8": opt-in (never chosen by "auto"): the bf16 mode with MXFP8 operands in the four per-layer DiT GEMMs
COMPUTE = {"fp32": F5H_FP32, "bf16": F5H_BF16, "fp16": F5H_FP16, "mxfp8": F5H_MXFP8}
# class bits of f5h_set_mx8_classes (the store policy's)
MX8_CLASS_BITS = {"qkv": 1, "out": 4, "ffn1": 8, "ffn2": 16}
F5H_DT_F32, F5H_DT_BF16, F5H_DT_F16 = 0, 1, 2
F5H_EULER, F5H_MIDPOINT, F5H_RK4 = 0, 1, 2
ODE_METHOD = {"euler": F5H_EULER, "midpoint": F5H_MIDPOINT, "rk4": F5H_RK4}

# exported symbols, checked by tests/test_boundary.py against include/f5h.h
EXPORTS = (
    "f5h_engine_create_views",
    "f5h_engine_create",
    "f5h_engine_destroy",
    "f5h_release_pending",
    "f5h_workspace_size",
    "f5h_sample",
    "f5h_workspace_size_ode",
    "f5h_sample_ode",
    "f5h_workspace_size_ragged",
    "f5h_sample_ragged",
    "f5h_debug_ode_tableau",
    "f5h_debug_ode_eval_times",
    "f5h_forward",
    "f5h_probe_enable",
    "f5h_probe_read",
    "f5h_probe_timeline",
    "f5h_set_graph_mode",
    "f5h_set_cfg_streams",
    "f5h_graph_stats",
    "f5h_last_call_host_ms",
    "f5h_set_pad_skip",
    "f5h_set_chain",
    "f5h_chain_stats",
    "f5h_chain_debug_spin_limit",
    "f5h_set_ln_fold",
    "f5h_ln_fold_stats",
    "f5h_set_store_policy",
    "f5h_store_policy_stats",
    "f5h_store_policy_force",
    "f5h_op_linear",
    "f5h_op_attention",
    "f5h_op_attention_qlen",
    "f5h_op_attention_split",
    "f5h_op_attention_ranges",
    "f5h_op_conv_pos",
    "f5h_op_norm",
    "f5h_op_dwconv_ln",
    "f5h_op_dwconv_ln_len",
    "f5h_op_grn",
    "f5h_op_grn_len",
    "f5h_op_attention_ragged",
    "f5h_op_conv_pos_ragged",
    "f5h_op_grn_ragged",
    "f5h_op_gemm_epi",
    "f5h_op_text_upsample",
    "f5h_op_lnfold_uv",
    "f5h_op_scale_cols",
    "f5h_op_mel_frames",
    "f5h_op_mel_frames_ragged",
    "f5h_op_mel_mag",
    "f5h_op_mel_log",
    "f5h_op_mel_log_ragged",
    "f5h_op_vocos_imcol",
    "f5h_op_vocos_imcol_ragged",
    "f5h_op_vocos_spec",
    "f5h_op_vocos_ola",
    "f5h_op_vocos_ola_ragged",
    "f5h_op_time_sinus",
    "f5h_op_rope_table",
    "f5h_op_text_embed",
    "f5h_op_build_ct",
    "f5h_op_pack_y",
    "f5h_op_masks",
    "f5h_op_final_where_out",
    "f5h_op_copy_pred",
    "f5h_op_cfg_euler",
    "f5h_op_cfg_rk",
    "f5h_gemm_force_config",
    "f5h_attn_force_safe",
    "f5h_debug_tile_live",
    "f5h_debug_magic_div_sweep",
    "f5h_debug_step_modes",
    "f5h_vocos_create",
    "f5h_vocos_destroy",
    "f5h_vocos_workspace_size",
    "f5h_vocos_decode",
    "f5h_vocos_ragged_workspace_size",
    "f5h_vocos_decode_ragged",
    "f5h_mel_create",
    "f5h_mel_destroy",
    "f5h_mel_workspace_size",
    "f5h_mel_forward",
    "f5h_mel_ragged_workspace_size",
    "f5h_mel_forward_ragged",
    "f5h_last_error",
    "f5h_version",
)

# the MXFP8 mode's entry points (compute="mxfp8"; tests/test_mx8_host.py checks them against include/f5h.h)
MX8_EXPORTS = (
    "f5h_set_mx8_classes",
    "f5h_mx8_stats",
    "f5h_debug_mx8_quant_block",
    "f5h_op_quant_mx8",
    "f5h_op_ln_modulate_mx8",
    "f5h_op_gemm_mx8",
)

KCLASS = {"ffn1": 0, "attention": 1, "qkv": 2, "ffn2": 3, "conv": 4, "out": 5, "norm": 6, "chain": 7}


class Arch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "backbone", "dim", "depth", "heads", "dim_head", "ff_dim", "text_dim", "text_num_embeds", "mel_dim",
        "conv_layers", "text_mask_padding", "pe_attn_head", "attn_mask_enabled", "compute",
        # appended options: read by a library that exports f5h_op_text_upsample (has_dit_options)
        "qk_norm", "long_skip_connection", "text_average_upsampling")]


class VocosArch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "input_channels", "dim", "intermediate_dim", "num_layers", "n_fft", "hop_length", "compute")]


class MelArch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("n_fft", "hop_length", "n_mels", "sample_rate")]


class Weight(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("numel", ctypes.c_int64)]


class TensorView(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("dtype", ctypes.c_int32),
                ("on_device", ctypes.c_int32), ("numel", ctypes.c_int64)]


class SampleArgs(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int32), ("N", ctypes.c_int32), ("nt", ctypes.c_int32), ("nfe", ctypes.c_int32),
        ("cond", ctypes.c_void_p), ("cond_mask", ctypes.c_void_p), ("text", ctypes.c_void_p),
        ("duration", ctypes.c_void_p), ("y0", ctypes.c_void_p), ("t_grid", ctypes.c_void_p),
        ("cfg_strength", ctypes.c_float), ("use_batch_mask", ctypes.c_int32),
        ("out", ctypes.c_void_p), ("trajectory", ctypes.c_void_p),
    ]


class ForwardArgs(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int32), ("N", ctypes.c_int32), ("nt", ctypes.c_int32),
        ("x", ctypes.c_void_p), ("cond", ctypes.c_void_p), ("cond_mask", ctypes.c_void_p),
        ("text", ctypes.c_void_p), ("duration", ctypes.c_void_p), ("t", ctypes.c_float),
        ("use_batch_mask", ctypes.c_int32), ("pred", ctypes.c_void_p),
        ("cfg_infer", ctypes.c_int32), ("drop_audio_cond", ctypes.c_int32), ("drop_text", ctypes.c_int32),
        ("t_dev", ctypes.c_void_p), ("text_cache", ctypes.c_int32),
    ]


class OpGemmArgs(ctypes.Structure):
    _fields_ = [
        ("compute", ctypes.c_int32), ("epi", ctypes.c_int32), ("M", ctypes.c_int32), ("N", ctypes.c_int32),
        ("K", ctypes.c_int32), ("k_split", ctypes.c_int32),
        ("A", ctypes.c_void_p), ("A2", ctypes.c_void_p), ("W", ctypes.c_void_p), ("bias", ctypes.c_void_p),
        ("C", ctypes.c_void_p), ("resid", ctypes.c_void_p), ("gate", ctypes.c_void_p), ("rowkeep", ctypes.c_void_p),
        ("live_len", ctypes.c_void_p), ("live_seq", ctypes.c_int32),
        ("seq_len", ctypes.c_int32), ("heads", ctypes.c_int32), ("rope_heads", ctypes.c_int32),
        ("q_scale", ctypes.c_float),
        ("add", ctypes.c_void_p), ("ld_add", ctypes.c_int64), ("dual_rows", ctypes.c_int64),
        ("q", ctypes.c_void_p), ("k", ctypes.c_void_p), ("v", ctypes.c_void_p), ("rope_out", ctypes.c_void_p),
        # LayerNorm / RMSNorm fold forms (all zero: none)
        ("hs_scale", ctypes.c_void_p), ("hs_out", ctypes.c_void_p), ("ln_part_out", ctypes.c_void_p),
        ("ln_part_in", ctypes.c_void_p), ("ln_u", ctypes.c_void_p), ("ln_v", ctypes.c_void_p),
        ("ln_nparts", ctypes.c_int32), ("ln_rms", ctypes.c_int32), ("ln_eps", ctypes.c_float),
        ("poison", ctypes.c_int32),
        # qk_norm (both null: none)
        ("q_norm_w", ctypes.c_void_p), ("k_norm_w", ctypes.c_void_p), ("qk_norm_eps", ctypes.c_float),
        # rows of a destination (sequence, head) panel (0 = seq_len); read by a library with has_mmdit()
        ("qkv_dst_len", ctypes.c_int32),
        # epi 7 over packed rows: HOST segment table [n_seq + 1] (null: none); read by a library with
        # has_ragged_sampler()
        ("seg_off", ctypes.c_void_p), ("n_seq", ctypes.c_int32),
    ]


class RaggedArgs(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int32), ("Lmax", ctypes.c_int32), ("nt", ctypes.c_int32), ("nfe", ctypes.c_int32),
        ("R", ctypes.c_int64),
        ("cond", ctypes.c_void_p), ("cond_mask", ctypes.c_void_p), ("text", ctypes.c_void_p),
        ("duration", ctypes.c_void_p), ("y0", ctypes.c_void_p), ("t_grid", ctypes.c_void_p),
        ("cfg_strength", ctypes.c_float),
        ("out", ctypes.c_void_p), ("trajectory", ctypes.c_void_p),
    ]


class OpStepArgs(ctypes.Structure):
    """f5h_op_step_args (f5h_op_cfg_euler / f5h_op_cfg_rk)"""
    _fields_ = [
        ("compute", ctypes.c_int32), ("method", ctypes.c_int32),
        ("B", ctypes.c_int32), ("N", ctypes.c_int32), ("mel", ctypes.c_int32), ("use_cfg", ctypes.c_int32),
        ("cfg", ctypes.c_float), ("dt", ctypes.c_float),
        ("y", ctypes.c_void_p), ("p", ctypes.c_void_p),
        ("p_seq_stride", ctypes.c_int64), ("p_ld", ctypes.c_int64),
        ("p_row_off", ctypes.c_int32), ("nfe", ctypes.c_int32),
        ("ypad", ctypes.c_void_p), ("traj", ctypes.c_void_p), ("kbuf", ctypes.c_void_p),
        ("kstep", ctypes.c_void_p), ("tgrid", ctypes.c_void_p), ("trajp", ctypes.c_void_p),
        ("next_src", ctypes.c_void_p), ("next_stride", ctypes.c_int64), ("next_n", ctypes.c_int32),
        ("next_dst", ctypes.c_void_p), ("arrive", ctypes.c_void_p), ("tick", ctypes.c_void_p),
    ]


OP_GUARD_ROWS = 4  # F5H_OP_GUARD_ROWS


_lib = None
_load_error = None


def lib():
    """Load libf5h.so once; raise a clear error if it is absent (no silent fallback)."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if _load_error is not None:
        raise RuntimeError(_load_error)
    if not os.path.exists(LIB_PATH):
        _load_error = (f"libf5h.so not found at {LIB_PATH}: build it with `python -c \"import __graft_entry__ as g; "
                       f"g.build()\"` or `make -C f5-tts_amd/csrc`")
        raise RuntimeError(_load_error)
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    L.f5h_engine_create.argtypes = [ctypes.POINTER(Arch), ctypes.POINTER(Weight), i32, i32, ctypes.POINTER(vp)]
    L.f5h_engine_create.restype = ctypes.c_int
    L.f5h_engine_create_views.argtypes = [ctypes.POINTER(Arch), ctypes.POINTER(TensorView), i32, i32,
                                          ctypes.POINTER(vp)]
    L.f5h_engine_create_views.restype = ctypes.c_int
    L.f5h_engine_destroy.argtypes = [vp]
    L.f5h_engine_destroy.restype = None
    L.f5h_release_pending.argtypes = [i32]
    L.f5h_release_pending.restype = ctypes.c_int
    L.f5h_workspace_size.argtypes = [vp, i32, i32, i32, i32, i32]
    L.f5h_workspace_size.restype = sz
    L.f5h_sample.argtypes = [vp, vp, ctypes.POINTER(SampleArgs), vp, sz]
    L.f5h_sample.restype = ctypes.c_int
    if hasattr(L, "f5h_sample_ode"):  # absent from an older build loaded through F5H_LIB: Euler only (has_ode)
        L.f5h_workspace_size_ode.argtypes = [vp, i32, i32, i32, i32, i32, i32]
        L.f5h_workspace_size_ode.restype = sz
        L.f5h_sample_ode.argtypes = [vp, vp, ctypes.POINTER(SampleArgs), i32, vp, sz]
        L.f5h_sample_ode.restype = ctypes.c_int
        fp = ctypes.POINTER(ctypes.c_float)
        L.f5h_debug_ode_tableau.argtypes = [i32, ctypes.POINTER(i32), fp, fp, fp]
        L.f5h_debug_ode_tableau.restype = ctypes.c_int
        L.f5h_debug_ode_eval_times.argtypes = [i32, i32, fp, i32, fp]
        L.f5h_debug_ode_eval_times.restype = ctypes.c_int
    L.f5h_forward.argtypes = [vp, vp, ctypes.POINTER(ForwardArgs), vp, sz]
    L.f5h_forward.restype = ctypes.c_int
    L.f5h_probe_enable.argtypes = [vp, i32, i32]
    L.f5h_probe_enable.restype = ctypes.c_int
    L.f5h_probe_read.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_double)]
    L.f5h_probe_read.restype = ctypes.c_int
    L.f5h_probe_timeline.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), i32, ctypes.POINTER(i32),
                                     ctypes.POINTER(ctypes.c_double)]
    L.f5h_probe_timeline.restype = ctypes.c_int
    L.f5h_set_graph_mode.argtypes = [vp, i32]
    L.f5h_set_graph_mode.restype = ctypes.c_int
    L.f5h_set_cfg_streams.argtypes = [vp, i32]
    L.f5h_set_cfg_streams.restype = ctypes.c_int
    L.f5h_graph_stats.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32)]
    L.f5h_graph_stats.restype = ctypes.c_int
    if hasattr(L, "f5h_last_call_host_ms"):
        L.f5h_last_call_host_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double), i32]
        L.f5h_last_call_host_ms.restype = ctypes.c_int
    L.f5h_set_pad_skip.argtypes = [vp, i32]
    L.f5h_set_pad_skip.restype = ctypes.c_int
    L.f5h_op_linear.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz]
    L.f5h_op_linear.restype = ctypes.c_int
    L.f5h_op_attention.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, sz]
    L.f5h_op_attention.restype = ctypes.c_int
    if hasattr(L, "f5h_op_gemm_epi"):  # op-level test entry points (absent from an older build, F5H_LIB)
        L.f5h_op_attention_qlen.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, sz]
        L.f5h_op_attention_qlen.restype = ctypes.c_int
        L.f5h_op_conv_pos.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, i32, i64, i64, vp, vp, sz]
        L.f5h_op_conv_pos.restype = ctypes.c_int
        L.f5h_op_norm.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz]
        L.f5h_op_norm.restype = ctypes.c_int
        L.f5h_op_dwconv_ln.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, sz]
        L.f5h_op_dwconv_ln.restype = ctypes.c_int
        L.f5h_op_grn.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz]
        L.f5h_op_grn.restype = ctypes.c_int
        L.f5h_op_gemm_epi.argtypes = [vp, ctypes.POINTER(OpGemmArgs), vp, sz]
        L.f5h_op_gemm_epi.restype = ctypes.c_int
        if hasattr(L, "f5h_op_lnfold_uv"):  # (a build with the op hooks but without the fold's)
            L.f5h_op_lnfold_uv.argtypes = [vp, i32, i32, i32, i32, i32, vp, i64, i64, vp, vp, vp, sz]
            L.f5h_op_lnfold_uv.restype = ctypes.c_int
            L.f5h_op_scale_cols.argtypes = [vp, i32, i64, i32, vp, vp, vp, vp, sz]
            L.f5h_op_scale_cols.restype = ctypes.c_int
    if hasattr(L, "f5h_op_attention_split"):  # absent from an older build (has_mmdit)
        L.f5h_op_attention_split.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, sz]
        L.f5h_op_attention_split.restype = ctypes.c_int
    if hasattr(L, "f5h_op_attention_ranges"):  # absent from an older build (has_isolate)
        L.f5h_op_attention_ranges.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, sz]
        L.f5h_op_attention_ranges.restype = ctypes.c_int
        L.f5h_op_dwconv_ln_len.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, sz]
        L.f5h_op_dwconv_ln_len.restype = ctypes.c_int
        L.f5h_op_grn_len.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz]
        L.f5h_op_grn_len.restype = ctypes.c_int
    if hasattr(L, "f5h_op_text_upsample"):  # absent from an older build (has_dit_options)
        L.f5h_op_text_upsample.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp]
        L.f5h_op_text_upsample.restype = ctypes.c_int
    L.f5h_gemm_force_config.argtypes = [i32]
    L.f5h_gemm_force_config.restype = ctypes.c_int
    # test hooks: bound when present, so an older build loaded through F5H_LIB (one-box A/Bs) still loads
    if hasattr(L, "f5h_attn_force_safe"):
        L.f5h_attn_force_safe.argtypes = [i32]
        L.f5h_attn_force_safe.restype = ctypes.c_int
    if hasattr(L, "f5h_set_chain"):
        L.f5h_set_chain.argtypes = [vp, i32]
        L.f5h_set_chain.restype = ctypes.c_int
        L.f5h_chain_stats.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(i64)]
        L.f5h_chain_stats.restype = ctypes.c_int
    if hasattr(L, "f5h_set_ln_fold"):
        L.f5h_set_ln_fold.argtypes = [vp, i32]
        L.f5h_set_ln_fold.restype = ctypes.c_int
        L.f5h_ln_fold_stats.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i64)]
        L.f5h_ln_fold_stats.restype = ctypes.c_int
    if hasattr(L, "f5h_set_store_policy"):
        L.f5h_set_store_policy.argtypes = [vp, i32]
        L.f5h_set_store_policy.restype = ctypes.c_int
        L.f5h_store_policy_stats.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
        L.f5h_store_policy_stats.restype = ctypes.c_int
        L.f5h_store_policy_force.argtypes = [i32]
        L.f5h_store_policy_force.restype = ctypes.c_int
    if hasattr(L, "f5h_set_mx8_classes"):  # absent from an older build (has_mx8)
        L.f5h_set_mx8_classes.argtypes = [vp, i32]
        L.f5h_set_mx8_classes.restype = ctypes.c_int
        L.f5h_mx8_stats.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i64)]
        L.f5h_mx8_stats.restype = ctypes.c_int
        L.f5h_debug_mx8_quant_block.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8),
                                                ctypes.POINTER(ctypes.c_uint8)]
        L.f5h_debug_mx8_quant_block.restype = ctypes.c_int
        L.f5h_op_quant_mx8.argtypes = [vp, i64, i32, vp, vp, vp, vp, sz]
        L.f5h_op_quant_mx8.restype = ctypes.c_int
        L.f5h_op_ln_modulate_mx8.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz]
        L.f5h_op_ln_modulate_mx8.restype = ctypes.c_int
        L.f5h_op_gemm_mx8.argtypes = [vp, ctypes.POINTER(OpGemmArgs), vp, vp, vp, vp, vp, sz]
        L.f5h_op_gemm_mx8.restype = ctypes.c_int
    if hasattr(L, "f5h_chain_debug_spin_limit"):
        L.f5h_chain_debug_spin_limit.argtypes = [i64]
        L.f5h_chain_debug_spin_limit.restype = ctypes.c_int
    if hasattr(L, "f5h_debug_tile_live"):
        L.f5h_debug_tile_live.argtypes = [vp, i32, i32, i32, i32]
        L.f5h_debug_tile_live.restype = ctypes.c_int
    if hasattr(L, "f5h_debug_magic_div_sweep"):  # absent from an older build (F5H_LIB)
        L.f5h_debug_magic_div_sweep.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                ctypes.POINTER(ctypes.c_uint32)]
        L.f5h_debug_magic_div_sweep.restype = ctypes.c_int64
    if hasattr(L, "f5h_debug_step_modes"):  # absent from an older build (F5H_LIB)
        L.f5h_debug_step_modes.argtypes = [ctypes.POINTER(i32), i32, ctypes.POINTER(i32), i32]
        L.f5h_debug_step_modes.restype = ctypes.c_int
    L.f5h_vocos_create.argtypes = [ctypes.POINTER(VocosArch), ctypes.POINTER(Weight), i32, i32, ctypes.POINTER(vp)]
    L.f5h_vocos_create.restype = ctypes.c_int
    L.f5h_vocos_destroy.argtypes = [vp]
    L.f5h_vocos_destroy.restype = None
    L.f5h_vocos_workspace_size.argtypes = [vp, i32, i32]
    L.f5h_vocos_workspace_size.restype = sz
    L.f5h_vocos_decode.argtypes = [vp, vp, i32, i32, vp, vp, vp, sz]
    L.f5h_vocos_decode.restype = ctypes.c_int
    L.f5h_mel_create.argtypes = [ctypes.POINTER(MelArch), i32, ctypes.POINTER(vp)]
    L.f5h_mel_create.restype = ctypes.c_int
    L.f5h_mel_destroy.argtypes = [vp]
    L.f5h_mel_destroy.restype = None
    L.f5h_mel_workspace_size.argtypes = [vp, i32, i32]
    L.f5h_mel_workspace_size.restype = sz
    L.f5h_mel_forward.argtypes = [vp, vp, i32, i32, vp, vp, vp, sz]
    L.f5h_mel_forward.restype = ctypes.c_int
    if hasattr(L, "f5h_vocos_decode_ragged"):  # absent from an older build (has_ragged)
        L.f5h_vocos_ragged_workspace_size.argtypes = [vp, i32, i64]
        L.f5h_vocos_ragged_workspace_size.restype = sz
        L.f5h_vocos_decode_ragged.argtypes = [vp, vp, i32, vp, i64, i64, i64, ctypes.POINTER(i32), ctypes.POINTER(i32),
                                              vp, vp, sz]
        L.f5h_vocos_decode_ragged.restype = ctypes.c_int
        L.f5h_mel_ragged_workspace_size.argtypes = [vp, i32, i64]
        L.f5h_mel_ragged_workspace_size.restype = sz
        L.f5h_mel_forward_ragged.argtypes = [vp, vp, i32, vp, i64, ctypes.POINTER(i32), i32, vp, vp, sz]
        L.f5h_mel_forward_ragged.restype = ctypes.c_int
    if hasattr(L, "f5h_sample_ragged"):  # absent from an older build (has_ragged_sampler)
        L.f5h_workspace_size_ragged.argtypes = [vp, i32, i64, i32, i32, i32, i32, i32]
        L.f5h_workspace_size_ragged.restype = sz
        L.f5h_sample_ragged.argtypes = [vp, vp, ctypes.POINTER(RaggedArgs), i32, vp, sz]
        L.f5h_sample_ragged.restype = ctypes.c_int
        pi32 = ctypes.POINTER(i32)
        L.f5h_op_attention_ragged.argtypes = [vp, i32, i32, i32, i32, i32, pi32, vp, vp, vp, i32, vp, vp, sz]
        L.f5h_op_attention_ragged.restype = ctypes.c_int
        L.f5h_op_conv_pos_ragged.argtypes = [vp, i32, i32, i32, i32, i32, pi32, vp, vp, vp, i32, vp, i32, vp, vp, sz]
        L.f5h_op_conv_pos_ragged.restype = ctypes.c_int
        L.f5h_op_grn_ragged.argtypes = [vp, i32, i32, i32, i32, i32, pi32, vp, vp, vp, vp, vp, sz]
        L.f5h_op_grn_ragged.restype = ctypes.c_int
    if hasattr(L, "f5h_op_cfg_euler"):  # absent from an older build (has_glue_ops)
        for name, args in (
                ("f5h_op_mel_frames", [vp, i32, i32, i32, i32, vp, vp]),
                ("f5h_op_mel_frames_ragged", [vp, i32, i32, i32, i32, vp, i64, vp, vp, vp]),
                ("f5h_op_mel_mag", [vp, i64, i32, i32, i32, vp, vp]),
                ("f5h_op_mel_log", [vp, i32, i32, i32, vp, vp]),
                ("f5h_op_mel_log_ragged", [vp, i32, i32, i32, vp, vp, vp]),
                ("f5h_op_vocos_imcol", [vp, i32, i32, i32, i32, i32, vp, vp]),
                ("f5h_op_vocos_imcol_ragged", [vp, i32, i32, i32, i32, i32, vp, i64, i64, i64, vp, vp, vp]),
                ("f5h_op_vocos_spec", [vp, i64, i32, i32, vp]),
                ("f5h_op_vocos_ola", [vp, i32, i32, i32, i32, vp, vp, vp]),
                ("f5h_op_vocos_ola_ragged", [vp, i32, i32, i32, i32, vp, vp, vp, vp]),
                ("f5h_op_time_sinus", [vp, i32, i32, vp, vp]),
                ("f5h_op_rope_table", [vp, i32, vp]),
                ("f5h_op_text_embed", [vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
                ("f5h_op_build_ct", [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
                ("f5h_op_pack_y", [vp, i32, i32, i32, vp, vp]),
                ("f5h_op_masks", [vp, i32, i32, i32, i32, i32, vp, vp]),
                ("f5h_op_final_where_out", [vp, i32, i32, i32, vp, vp, vp, vp, vp]),
                ("f5h_op_copy_pred", [vp, i32, i32, i32, i32, i64, vp, vp, vp]),
                ("f5h_op_cfg_euler", [vp, ctypes.POINTER(OpStepArgs)]),
                ("f5h_op_cfg_rk", [vp, ctypes.POINTER(OpStepArgs)])):
            getattr(L, name).argtypes = args
            getattr(L, name).restype = ctypes.c_int
    L.f5h_last_error.argtypes = []
    L.f5h_last_error.restype = ctypes.c_char_p
    L.f5h_version.argtypes = []
    L.f5h_version.restype = ctypes.c_char_p
    _lib = L
    return L


def has_ode() -> bool:
    """False for an older build (F5H_LIB) without f5h_sample_ode: such a library samples with Euler only."""
    return hasattr(lib(), "f5h_sample_ode")


def has_dit_options() -> bool:
    """False for an older build (F5H_LIB) without f5h_op_text_upsample: such a library ignores the arch fields
    qk_norm / long_skip_connection / text_average_upsampling and the qk_norm fields of the GEMM op hook."""
    return hasattr(lib(), "f5h_op_text_upsample")


def has_mmdit() -> bool:
    """False for an older build (F5H_LIB) without f5h_op_attention_split: such a library has no MMDiT backbone, no
    split attention output and ignores the qkv_dst_len field of the GEMM op hook."""
    return hasattr(lib(), "f5h_op_attention_split")


def has_isolate() -> bool:
    """False for an older build (F5H_LIB) without f5h_op_attention_ranges: such a library has no isolated batches
    (use_batch_mask == 2) and no second key range in attention."""
    return hasattr(lib(), "f5h_op_attention_ranges")


def has_ragged() -> bool:
    """False for an older build (F5H_LIB) without f5h_vocos_decode_ragged: such a library has no ragged batch
    entry points (Vocos.decode_ragged, MelSpec.forward_ragged)."""
    return hasattr(lib(), "f5h_vocos_decode_ragged")


def has_ragged_sampler() -> bool:
    """False for an older build (F5H_LIB) without f5h_sample_ragged: such a library has no ragged sampling path
    (CFM.sample(ragged=True)), no ragged op hooks and ignores the seg_off field of the GEMM op hook."""
    return hasattr(lib(), "f5h_sample_ragged")


def has_mx8() -> bool:
    """False for an older build (F5H_LIB) without f5h_set_mx8_classes: such a library has no compute="mxfp8"."""
    return hasattr(lib(), "f5h_set_mx8_classes")


def has_glue_ops() -> bool:
    """False for an older build (F5H_LIB) without f5h_op_cfg_euler: such a library has no op hooks for the audio
    glue, prologue and ODE step kernels."""
    return hasattr(lib(), "f5h_op_cfg_euler")


def check(rc: int, what: str = "f5h"):
    if rc != 0:
        msg = lib().f5h_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {rc}): {msg}")


def host_ints(x, n: int, what: str) -> "list[int]":
    """Python ints of a host-side per-utterance argument (an int for all n, a list/tuple, or a CPU tensor).
    A device tensor raises: reading it would be a hidden synchronisation, so host values are required."""
    if torch.is_tensor(x):
        if x.device.type != "cpu":
            raise ValueError(f"{what} must be host values (ints, a list or a CPU tensor), not a tensor on {x.device}: "
                             "reading it back would synchronise the device")
        x = x.reshape(-1).tolist()
    elif isinstance(x, int):
        x = [x] * n
    vals = [int(v) for v in x]
    if len(vals) != n:
        raise ValueError(f"{what} has {len(vals)} entries for {n} utterances")
    return vals


def ptr(t) -> int | None:
    return None if t is None else t.data_ptr()


def stream_handle(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream
