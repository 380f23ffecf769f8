"""ctypes binding of libwae_hip.so (the C ABI declared in include/wae.h).

There is no CPU fallback: if the shared object is missing or a call fails, this raises.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WAE_LIB_PATH") or os.path.join(_HERE, "libwae_hip.so")   # WAE_LIB_PATH: A/B of two builds (tools/)

WAE_F32, WAE_BF16, WAE_F16 = 0, 1, 2
GLU_SAVE_Z, GLU_NO_OUT, GLU_WAVES4, GLU_CG2, GLU_PAIR, GLU_GENERIC = 2, 4, 8, 16, 32, 64
TM_INTERLEAVE, TM_ONE_WG = 1, 2
ERR_CLASS_ID, ERR_SPEAKER_ID, ERR_TARGET_ID, ERR_NOT_ONEHOT = 1, 2, 4, 8

c_i32, c_i64, c_f32, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


class GluDesc(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("dtype", "B", "T", "Rp", "Ccp", "Hp", "ktaps", "dilation", "flags")]


class ArDesc(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("dtype", "B", "T", "L", "R", "Rp", "G", "Hp", "S", "O", "Cc", "Ccp", "ktaps", "mode",
                                     "init_idx", "scalar_input")] + [("scale", c_f32), ("n_forced", c_i32), ("coop_generic", c_i32),
                                                                       ("resident_lds", c_i32), ("resident_regs", c_i32),
                                                                       ("t0", c_i32)]      # t0: trailing, so every positional construction means 0

    # include/wae.h: scalar_input = 2 is a scalar-input decoder that asks the cooperative entries for the constant-size scalar kernels.
    # Read and written here as a flag of its own: 0 unless asked for; a class-id descriptor (scalar_input 0) has no such request.
    @property
    def scalar_sized(self):
        return int(self.scalar_input == 2)

    @scalar_sized.setter
    def scalar_sized(self, on):
        if self.scalar_input:
            self.scalar_input = 2 if on else 1


class ArItem(ctypes.Structure):          # include/wae.h: wae_ar_item (device array element of wae_ar_generate_list)
    _fields_ = [("off", c_i64), ("T", c_i32), ("n_forced", c_i32), ("init_idx", c_i32), ("row", c_i32)]


class ArSpan(ctypes.Structure):          # include/wae.h: wae_ar_span (device array element of the wae_ar_generate*_spans entries)
    _fields_ = [("off", c_i64), ("ring", c_i64), ("T", c_i32), ("t0", c_i32), ("n_forced", c_i32), ("init_idx", c_i32), ("row", c_i32),
                ("reserved", c_i32)]


class GluSeg(ctypes.Structure):          # include/wae.h: wae_glu_seg (device array element of wae_glu_layer_fwd_list, wae_nll_segments)
    _fields_ = [(n, c_i32) for n in ("row_off", "T", "zb_row", "tile0")]


class VqSeg(ctypes.Structure):           # include/wae.h: wae_vq_seg (device array element of wae_vq_stats_segments)
    _fields_ = [(n, c_i32) for n in ("q_off", "Tq")]


VQ_MAX_SLICES = 8


class VqSliceRec(ctypes.Structure):      # include/wae.h: wae_vq_slice_rec (HOST array element of wae_vq_search_slices)
    _fields_ = [("emb", c_vp), ("d0", c_i32), ("D", c_i32), ("K", c_i32), ("c_loss", c_f32)]


class TmDesc(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("dtype", "B", "T", "M", "nsrc", "mode")] + [("alpha", c_f32), ("flags", c_i32)]


class TmCe(ctypes.Structure):            # include/wae.h: wae_tm_ce (modes 5 / 6 of the wide head)
    _fields_ = [("logits", c_vp), ("target", c_vp), ("nll", c_vp), ("lse", c_vp), ("lengths", c_vp), ("inv_count", c_f32),
                ("O", c_i32)]


class TnTile(ctypes.Structure):          # include/wae.h: wae_tn_tile (device array element)
    _fields_ = [("P", c_vp), ("Q", c_vp), ("onehot", c_vp), ("C", c_vp), ("p_stride", c_i64), ("q_stride", c_i64), ("ldc", c_i64),
                ("m_valid", c_i32), ("n_valid", c_i32), ("m0", c_i32), ("shift", c_i32), ("ones_col", c_i32), ("alpha", c_f32)]


class GluBwdDesc(ctypes.Structure):      # include/wae.h: wae_glu_bwd_desc
    _fields_ = [(n, c_i32) for n in ("dtype", "B", "T", "Rp", "Hp", "Sp", "ktaps", "dilation")] + [("alpha", c_f32)]


class TsJob(ctypes.Structure):           # include/wae.h: wae_ts_job (device array element)
    _fields_ = [("P", c_vp), ("Q", c_vp), ("C", c_vp), ("p_stride", c_i64), ("q_stride", c_i64), ("ldc", c_i64),
                ("m_valid", c_i32), ("n_valid", c_i32), ("shift", c_i32), ("ones_col", c_i32), ("alpha", c_f32), ("pad_", c_i32)]


class TqJob(ctypes.Structure):           # include/wae.h: wae_tq_job (device array element of wae_gemm_tn_static)
    _fields_ = [("P", c_vp), ("Q0", c_vp), ("Q1", c_vp), ("C0", c_vp), ("C1", c_vp), ("Cb", c_vp), ("p_stride", c_i64),
                ("q0_stride", c_i64), ("q1_stride", c_i64), ("ldc0", c_i64), ("ldc1", c_i64), ("m_valid", c_i32), ("n0_valid", c_i32),
                ("n1_valid", c_i32), ("shift", c_i32), ("ones_col", c_i32), ("kind", c_i32), ("alpha", c_f32), ("pad_", c_i32)]


TQ_TAPS, TQ_COND, TQ_OUTSKIP = 0, 1, 2


class TsSeg(ctypes.Structure):           # include/wae.h: wae_ts_seg
    _fields_ = [("job", c_i32), ("slab_begin", c_i32), ("slab_end", c_i32)]


class GatherJob(ctypes.Structure):       # include/wae.h: wae_gather_job (host array element)
    _fields_ = [("src", c_vp), ("map", c_vp), ("dst", c_vp), ("n", c_i64), ("src_stride", c_i64), ("dst_stride", c_i64),
                ("nbatch", c_i32), ("dtype", c_i32)]


class ScatterJob(ctypes.Structure):      # include/wae.h: wae_scatter_job (host array element)
    _fields_ = [("src", c_vp), ("map", c_vp), ("dst", c_vp), ("n", c_i64), ("src_stride", c_i64), ("dst_stride", c_i64),
                ("src_ld", c_i64), ("nbatch", c_i32), ("src_cols", c_i32), ("unique", c_i32), ("pad_", c_i32)]


MULTI_MAX = 16


class FinishRow(ctypes.Structure):       # include/wae.h: wae_finish_row (device array element of wae_grad_finish)
    _fields_ = [("off", c_i64), ("g_off", c_i64), ("base", c_i64), ("cols", c_i32), ("pat", c_i32)]


class HeadDesc(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ("dtype", "B", "T", "Ku", "Sp", "Op", "O")] + [("scale", c_f32)]


# the 16 arguments every wae_ar_generate* entry starts with: the descriptor, (dilations, ring_off, ring, ring_total, w_layers,
# layer_stride_bytes, w2_off_bytes), (bias2, zb, first_tab, first_bias, w_head, head_bias, c_up), c_dtype; the cooperative entries
# put C (and dist) behind the descriptor, the list entries (n_items, n_slots, items, next) / (C, n_items, n_teams, items, next, total),
# the scalar list entries dist in front of n_items
_AR = [ctypes.POINTER(ArDesc), c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_i64] + [c_vp] * 7 + [c_i32]

# name -> (restype, argtypes); mirrors include/wae.h one to one
SIGNATURES = {
    "wae_version": (ctypes.c_char_p, []),
    "wae_last_error": (ctypes.c_char_p, []),
    "wae_weight_norm_fwd": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "wae_weight_norm_bwd": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_vp]),
    "wae_weight_norm_bwd_range": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp]),
    "wae_pack_gather": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i64, c_i64, c_i32, c_vp]),
    "wae_unpack_scatter_add": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i64, c_i64, c_i32, c_i64, c_i32, c_vp]),
    "wae_pack_gather_multi": (c_i32, [ctypes.POINTER(GatherJob), c_i32, c_vp]),
    "wae_unpack_scatter_add_multi": (c_i32, [ctypes.POINTER(ScatterJob), c_i32, c_vp]),
    "wae_enc_conv_fwd": (c_i32, [c_vp, c_vp, c_vp, c_vp] + [c_i32] * 9 + [c_vp]),
    # x, w, bias, y, segs, nsegs, tiles, ntiles, et, in_pitch, out_pitch, Cin, Cout, k, stride, pad, relu, residual, stream
    "wae_enc_conv_fwd_list": (c_i32, [c_vp] * 5 + [c_i32, c_vp] + [c_i32] * 11 + [c_vp]),
    # x, w, bias, y, recs, nrecs, ntiles, et, in_pitch, out_pitch, Cin, Cout, k, stride, pad, relu, residual, stream
    "wae_enc_conv_fwd_ranges": (c_i32, [c_vp] * 5 + [c_i32] * 12 + [c_vp]),
    # the ranges entry's arguments, records wae_enc_ring (8 x int32) in the place of wae_enc_range
    "wae_enc_conv_fwd_rings": (c_i32, [c_vp] * 5 + [c_i32] * 12 + [c_vp]),
    "wae_vq_nearest": (c_i32, [c_vp] * 6 + [c_i32] * 4 + [c_f32, c_vp]),
    # lat, quant, idx, segs, nsegs, D, pitch, K, c_loss, first, sqerr, hist, item_stats, out, stream
    "wae_vq_stats_segments": (c_i32, [c_vp] * 4 + [c_i32] * 4 + [c_f32, c_i32] + [c_vp] * 5),
    "wae_upsample_stage_fwd": (c_i32, [c_vp, c_vp, c_vp] + [c_i32] * 7 + [c_vp]),
    # in, w, out, segs, nsegs, ntiles, in_pitch, out_pitch_or_rows, C, s, out_btc, Cp, dtype, stream
    "wae_upsample_stage_fwd_list": (c_i32, [c_vp] * 4 + [c_i32] * 9 + [c_vp]),
    # the list entry's arguments, records wae_ups_range in the place of wae_ups_seg
    "wae_upsample_stage_fwd_ranges": (c_i32, [c_vp] * 4 + [c_i32] * 9 + [c_vp]),
    # the ranges entry's arguments, records wae_ups_ring (8 x int32) in the place of wae_ups_range
    "wae_upsample_stage_fwd_rings": (c_i32, [c_vp] * 4 + [c_i32] * 9 + [c_vp]),
    # in, out, segs, nsegs, ntiles, in_pitch, C, Cp, dtype, stream
    "wae_to_btc_list": (c_i32, [c_vp] * 3 + [c_i32] * 6 + [c_vp]),
    "wae_gproj_fwd": (c_i32, [c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp] + [c_i32] * 6 + [c_vp, c_vp]),
    "wae_gproj_bwd": (c_i32, [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_i64] + [c_i32] * 7 + [c_vp]),
    "wae_gproj_bwd_consume": (c_i32, [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_i64] + [c_i32] * 7 + [c_vp]),
    # sums, counts, K, ce, ce_weight, vq_loss, vq_weight, hist, out, stream
    "wae_accum_stats": (c_i32, [c_vp, c_vp, c_i32, c_vp, ctypes.c_double, c_vp, ctypes.c_double, c_vp, c_vp, c_vp]),
    "wae_check_ids": (c_i32, [c_vp, c_i64, c_i32, c_i32, c_vp, c_i32, c_vp]),
    "wae_onehot_to_ids": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i64, c_i64, c_i64, c_vp, c_vp, c_i32, c_vp]),
    "wae_stream_delay": (c_i32, [ctypes.c_double, c_vp]),
    "wae_upsample_stage_bwd": (c_i32, [c_vp] * 5 + [c_i32] * 4 + [c_vp]),
    "wae_enc_conv_bwd": (c_i32, [c_vp] * 7 + [c_i32] * 9 + [c_vp]),
    # the list forms of the front end's backward (csrc/frontend_bwd_list.hip)
    # in, out, segs, nsegs, ntiles, pitch, rows, C, Cp, dtype, scale, stream
    "wae_from_btc_list": (c_i32, [c_vp] * 3 + [c_i32] * 7 + [c_f32, c_vp]),
    # dout, in, w, din, dw, segs, nsegs, ntiles, in_pitch, out_pitch, C, s, stream
    "wae_upsample_stage_bwd_list": (c_i32, [c_vp] * 6 + [c_i32] * 6 + [c_vp]),
    # x, w, y, dy, dx, dw, dbias, segs, nsegs, tiles, ntiles, et, in_pitch, out_pitch, Cin, Cout, k, stride, pad, relu, residual, stream
    "wae_enc_conv_bwd_list": (c_i32, [c_vp] * 8 + [c_i32, c_vp] + [c_i32] * 11 + [c_vp]),
    "wae_vq_bwd": (c_i32, [c_vp] * 6 + [c_i32] * 3 + [c_f32, c_f32, c_vp]),
    "wae_vq_slice": (c_i32, [c_vp] * 6 + [c_i32] * 6 + [c_f32, c_i32, c_vp]),
    "wae_vq_ema_update": (c_i32, [c_vp] * 6 + [c_i32] * 6 + [c_f32, c_vp]),
    "wae_vq_slice_bwd": (c_i32, [c_vp] * 6 + [c_i32] * 5 + [c_f32, c_f32, c_vp]),
    "wae_vq_search_slices_scratch": (c_i64, [ctypes.POINTER(VqSliceRec), c_i32]),
    # lat, recs_host, nslices, idx, quant, stats, scratch, B, Dtot, Tq, mode, stream
    "wae_vq_search_slices": (c_i32, [c_vp, ctypes.POINTER(VqSliceRec), c_i32, c_vp, c_vp, c_vp, c_vp] + [c_i32] * 4 + [c_vp]),
    "wae_first_conv_fwd": (c_i32, [c_vp] * 5 + [c_i64, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "wae_onehot_rows": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp]),
    "wae_softmax_bct_fwd": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "wae_softmax_bct_bwd": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "wae_bmm_f32": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, ctypes.c_float, c_vp]),
    "wae_glu_layer_fwd": (c_i32, [ctypes.POINTER(GluDesc), c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    "wae_glu_layer_fwd_drop": (c_i32, [ctypes.POINTER(GluDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    # d, segs, nsegs, ntiles, rows, x_in, x_out, c_up, u_out, u_stride, zb, zb_stride, w_packed, bias_out, stream
    "wae_glu_layer_fwd_list": (c_i32, [ctypes.POINTER(GluDesc), c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64,
                                       c_vp, c_vp, c_vp]),
    "wae_glu_list_tile": (c_i32, [c_i32]),
    # nll, segs, nsegs, rows, first, nll_sum, count, out, stream
    "wae_nll_segments": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "wae_dropout_fwd": (c_i32, [c_vp, c_vp, c_i64, ctypes.c_uint64, c_f32, c_i32, c_vp]),
    "wae_dropout_bwd": (c_i32, [c_vp, c_vp, c_vp, c_i64, ctypes.c_uint64, c_f32, c_f32, c_i32, c_vp]),
    "wae_glu_packed_bytes": (c_i64, [ctypes.POINTER(GluDesc)]),
    "wae_head_fwd": (c_i32, [ctypes.POINTER(HeadDesc)] + [c_vp] * 10),
    "wae_head_fwd_from_h0": (c_i32, [ctypes.POINTER(HeadDesc)] + [c_vp] * 9),
    "wae_head_bwd": (c_i32, [ctypes.POINTER(HeadDesc)] + [c_vp] * 7 + [c_f32] + [c_vp] * 5),
    "wae_head_bwd_packed_bytes": (c_i64, [ctypes.POINTER(HeadDesc)]),
    "wae_head_train_supported": (c_i32, [c_i32, c_i32, c_i32]),
    "wae_head_train_ws_bytes": (c_i64, [ctypes.POINTER(HeadDesc)]),
    # d, h0, w_tail, w_bwd_packed, bias, target, lengths, dy_factor, nll, lse, h1_save, dy, dh1, dskip, red_ws, loss, stream
    "wae_head_train_from_h0": (c_i32, [ctypes.POINTER(HeadDesc)] + [c_vp] * 6 + [c_f32] + [c_vp] * 9),
    "wae_gemm_tm": (c_i32, [ctypes.POINTER(TmDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "wae_gemm_tm_ce": (c_i32, [ctypes.POINTER(TmDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, ctypes.POINTER(TmCe), c_vp]),
    "wae_gemm_tn_tiles": (c_i32, [c_i32, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "wae_gemm_tn_tiles_det_floats": (c_i64, [c_i32, c_i32, c_i32, c_i32]),
    # dtype, tiles_dev, ntiles, B, T, splits, partials, partials_floats, ordered, stream
    "wae_gemm_tn_tiles_det": (c_i32, [c_i32, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_i64, c_i32, c_vp]),
    # the fixed-order forms of the small sums (include/wae.h): their twins' arguments and a partials buffer
    "wae_gproj_bwd_det_floats": (c_i64, [c_i32] * 4),
    "wae_gproj_bwd_det": (c_i32, [c_vp, c_vp, c_i64, c_i64, c_i64, c_vp, c_i64, c_vp, c_vp, c_i64, c_i64] + [c_i32] * 8 + [c_vp, c_i64, c_vp]),
    "wae_upsample_stage_bwd_det_floats": (c_i64, []),
    "wae_upsample_stage_bwd_det": (c_i32, [c_vp] * 6 + [c_i64] + [c_i32] * 4 + [c_vp]),
    "wae_upsample_stage_bwd_list_det_floats": (c_i64, []),
    "wae_upsample_stage_bwd_list_det": (c_i32, [c_vp] * 6 + [c_i32] * 6 + [c_vp, c_i64, c_vp]),
    "wae_vq_slice_bwd_det": (c_i32, [c_vp] * 6 + [c_i32] * 6 + [c_f32, c_f32, c_vp]),
    "wae_vq_bwd_det": (c_i32, [c_vp] * 6 + [c_i32] * 4 + [c_f32, c_f32, c_vp]),
    "wae_vq_loss_det": (c_i32, [c_vp] * 3 + [c_i32] * 5 + [c_f32, c_vp]),
    "wae_clip_adam_ema_det": (c_i32, [c_vp] * 5 + [c_i64, c_vp, c_i64, c_vp, c_i32] + [ctypes.c_double] * 7 + [c_vp]),
    "wae_glu_bwd_fused_supported": (c_i32, [c_i32, c_i32]),
    "wae_glu_bwd_fused_supported16": (c_i32, [c_i32, c_i32]),
    "wae_glu_bwd_fused": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "wae_glu_bwd_fused_dc": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp]),
    "wae_gemm_tn_stream": (c_i32, [c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_i32, c_i32, c_vp]),
    "wae_gemm_tn_static": (c_i32, [c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i64, c_vp]),
    "wae_sum_rows": (c_i32, [c_vp, c_i64, c_i64, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "wae_head_packed_bytes": (c_i64, [ctypes.POINTER(HeadDesc)]),
    "wae_dmol_loss_fwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_i32, c_vp]),
    "wae_dmol_sample": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_i32, c_vp]),
    "wae_mog_loss_fwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_i32, c_vp]),
    "wae_mog_sample": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "wae_clip_adam_ema": (c_i32, [c_vp] * 5 + [c_i64, c_vp, c_vp, c_i32] + [ctypes.c_double] * 7 + [c_vp]),
    "wae_clip_adam_ema_summed": (c_i32, [c_vp] * 5 + [c_i64, c_vp, c_vp, c_i32] + [ctypes.c_double] * 7 + [c_vp]),
    "wae_grad_finish": (c_i32, [c_vp] * 6 + [c_i32, c_i32, c_vp, c_vp]),
    "wae_ar_generate": (c_i32, _AR + [c_vp] * 5),
    "wae_ar_generate_scalar": (c_i32, _AR + [c_vp] * 3 + [c_f32, c_i32, c_vp, c_vp, c_vp]),
    "wae_ar_generate_scalar_mog": (c_i32, _AR + [c_vp] * 3 + [c_f32, c_vp, c_vp, c_vp]),
    "wae_ar_generate_list": (c_i32, _AR[:1] + [c_i32, c_i32, c_vp, c_vp] + _AR[1:] + [c_vp] * 5),
    "wae_ar_coop_msg_values": (c_i32, [ctypes.POINTER(ArDesc), c_i32]),
    "wae_ar_coop_acc_floats": (c_i64, [ctypes.POINTER(ArDesc)]),
    "wae_ar_generate_coop": (c_i32, _AR[:1] + [c_i32] + _AR[1:] + [c_vp] * 8),
    "wae_ar_generate_coop_fused": (c_i32, _AR[:1] + [c_i32] + _AR[1:] + [c_vp] * 9),
    "wae_ar_generate_coop_list": (c_i32, _AR[:1] + [c_i32, c_i32, c_i32, c_vp, c_vp, c_i64] + _AR[1:] + [c_vp] * 8),
    "wae_ar_generate_coop_scalar": (c_i32, _AR[:1] + [c_i32, c_i32] + _AR[1:] + [c_vp] * 3 + [c_f32, c_i32] + [c_vp] * 6),
    "wae_ar_generate_scalar_list": (c_i32, _AR[:1] + [c_i32, c_i32, c_i32, c_vp, c_vp] + _AR[1:] + [c_vp] * 3 + [c_f32, c_i32] + [c_vp] * 3),
    "wae_ar_generate_coop_scalar_list": (c_i32, _AR[:1] + [c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64] + _AR[1:] + [c_vp] * 3
                                         + [c_f32, c_i32] + [c_vp] * 6),
    # the span entries take their list twins' arguments (spans in place of items)
    "wae_ar_generate_spans": (c_i32, _AR[:1] + [c_i32, c_i32, c_vp, c_vp] + _AR[1:] + [c_vp] * 5),
    "wae_ar_generate_scalar_spans": (c_i32, _AR[:1] + [c_i32, c_i32, c_i32, c_vp, c_vp] + _AR[1:] + [c_vp] * 3 + [c_f32, c_i32] + [c_vp] * 3),
    "wae_ar_generate_coop_spans": (c_i32, _AR[:1] + [c_i32, c_i32, c_i32, c_vp, c_vp, c_i64] + _AR[1:] + [c_vp] * 8),
    "wae_ar_generate_coop_scalar_spans": (c_i32, _AR[:1] + [c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64] + _AR[1:] + [c_vp] * 3
                                          + [c_f32, c_i32] + [c_vp] * 6),
    "wae_ar_coop_ring_floats": (c_i64, [ctypes.POINTER(ArDesc), c_i32, c_i64]),
    "wae_ce_logits_fwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "wae_ce_logits_bwd": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "wae_weighted_mean": (c_i32, [c_vp, c_vp, c_i64, c_vp, c_vp]),
    "wae_masked_mean": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp]),
    "wae_to_btc": (c_i32, [c_vp, c_vp] + [c_i32] * 5 + [c_vp]),
    "wae_to_btc_masked": (c_i32, [c_vp, c_vp] + [c_i32] * 5 + [c_vp, c_f32, c_vp]),
    "wae_from_btc": (c_i32, [c_vp, c_vp] + [c_i32] * 5 + [c_vp]),
    "wae_from_btc_scaled": (c_i32, [c_vp, c_vp] + [c_i32] * 5 + [c_f32, c_vp]),
    "wae_act_fwd": (c_i32, [c_vp, c_i64, c_i32, c_f32, c_vp]),
    "wae_act_bwd": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_f32, c_vp]),
}

_lib = None


class WaeError(RuntimeError):
    pass


def build(force=False):
    """Compile csrc/*.hip for gfx950 into libwae_hip.so (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src, "clean"])
    subprocess.check_call(["make", "-C", src, "-j4"])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WaeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the hot path)")
        # torch first: its wheel carries its own libamdhip64, and libwae_hip.so must bind to THAT runtime -- loaded the other
        # way round, /opt/rocm's copy comes in as a second HIP runtime that does not know torch's allocations
        # (hipMemcpyAsync on a torch tensor then fails with "invalid value")
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        raise WaeError(f"{what} failed (rc={rc}): {lib().wae_last_error().decode()}")


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())
