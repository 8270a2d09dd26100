"""ctypes binding of libgda_hip.so (the C ABI declared in include/gda_hip.h).

The product path has no fallback: if the library is missing or a call fails this module
raises.

A call site reads like the prototype: ``call("gda_x", a, n, b, ..., stream())`` looks ``gda_x`` up, calls it and raises
``GdaError`` naming it on a non-zero status.  ``_SIGNATURES`` does the conversions: a tensor (or None) crosses as a raw
pointer through ``_P.from_param``, a Python number as the scalar type of its position, the stream -- always written
out, always last -- as the raw handle of torch's current stream.  ``scratch(size_fn_name, device, tag, *dims)`` is the
workspace query and the cached buffer in one.  Entry points that return a size or a count are plain ``lib().gda_x()``
calls; ``check`` and ``ptr`` remain for code that calls those by hand.
"""
import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_size_t, c_void_p

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libgda_hip.so")

class _P(c_void_p):
    """A pointer argument.  ``argtypes`` converts with ``from_param``, so a call site passes the tensor itself."""

    @classmethod
    def from_param(cls, obj):
        if isinstance(obj, torch.Tensor):
            return c_void_p(obj.data_ptr())
        if obj is None:
            return None
        if isinstance(obj, str):             # c_void_p would take it as a wide string; no entry point wants one
            raise TypeError("a str is not a pointer argument")
        return c_void_p.from_param(obj)      # an int address (ndarray.ctypes.data), a c_void_p, a ctypes array


_SIGNATURES = {
    "gda_abi_version": (c_int, []),
    "gda_status_string": (c_char_p, [c_int]),
    "gda_graph_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_build_csr_norm": (c_int, [_P, _P, _P, c_int64, c_int64, c_float, c_int, c_int, c_int,
                                   _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_build_csr_norm_map": (c_int, [_P, _P, _P, c_int64, c_int64, c_float, c_int, c_int, c_int,
                                       _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_gat_fwd_f32": (c_int, [_P, _P, c_int64, c_int64, _P, _P, _P, c_float, _P, _P, _P]),
    "gda_gat_bwd_f32": (c_int, [_P, _P, _P, _P, _P, c_int64, c_int64, _P, _P, _P, c_float, _P, _P,
                                _P, _P, _P, _P, _P]),
    "gda_faconv_fwd_f32": (c_int, [_P, _P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_float, _P, _P,
                                   c_int64, _P, _P]),
    "gda_faconv_bwd_f32": (c_int, [_P, _P, _P, _P, _P, _P, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, c_float,
                                   _P, c_int64, _P, _P, c_int64, _P, _P]),
    "gda_closs_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_closs_fwd_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, _P, _P, _P, _P, c_size_t, _P]),
    "gda_closs_bwd_f32": (c_int, [_P, c_int64, _P, _P, _P, c_int64, c_int64, _P, c_int64, _P]),
    "gda_colstats_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_weighted_moments_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, _P, _P, _P, c_size_t, _P]),
    "gda_std_mean_match_fwd_f32": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_std_mean_match_bwd_f32": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, _P, _P, c_int64, _P]),
    "gda_acdne_ppmi_workspace_bytes": (c_size_t, [c_int64]),
    "gda_acdne_ppmi_f32": (c_int, [_P, _P, _P, c_int64, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_acdne_xnei_f32": (c_int, [_P, c_int64, c_int64, _P, _P, _P, c_int64, _P, c_int64, _P]),
    "gda_acdne_prox_workspace_bytes": (c_size_t, [c_int64]),
    "gda_acdne_prox_f32": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, _P, _P, c_int64, c_int64, c_float, _P, _P,
                                   _P, c_size_t, _P]),
    "gda_acdne_heads_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "gda_acdne_heads_f32": (c_int, [_P, _P, c_int64, c_int64, c_int64, _P, _P, c_int64, _P, _P, _P, c_float, _P, _P, _P,
                                    _P, _P, c_size_t, _P]),
    "gda_acdne_predict_f32": (c_int, [_P, c_int64, c_int64, _P, _P, c_int64, _P, _P]),
    "gda_dmgnn_prox_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_dmgnn_prox_f32": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, _P, _P, c_int64, c_int64, c_float, _P, _P,
                                   _P, _P, c_size_t, _P]),
    "gda_dmgnn_heads_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "gda_dmgnn_heads_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_int64, _P, _P, c_int64, _P, _P, _P, c_float, _P, _P,
                                    _P, _P, _P, c_size_t, _P]),
    "gda_dmgnn_predict_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_dmgnn_predict_f32": (c_int, [_P, c_int64, c_int64, _P, _P, c_int64, _P, c_int64, _P, _P, c_size_t, _P]),
    "gda_asn_recon_chunks": (c_int, [c_int64]),
    "gda_asn_recon_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_asn_recon_f32": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, _P, c_float, c_float, _P, _P,
                                  c_int64, _P, c_size_t, _P]),
    "gda_asn_rows_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "gda_asn_kld_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, c_int64, ctypes.c_double, _P, _P, _P, _P, c_size_t,
                                _P]),
    "gda_asn_reparam_fwd_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, c_int64, _P, c_int, ctypes.c_uint64, _P,
                                        ctypes.c_uint32, _P, _P]),
    "gda_asn_reparam_bwd_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_int64, _P, _P]),
    "gda_asn_dropout_fwd_f32": (c_int, [_P, c_int64, c_float, ctypes.c_uint64, _P, ctypes.c_uint32, _P, _P, _P]),
    "gda_asn_mask_mul_f32": (c_int, [_P, _P, c_int64, _P, _P]),
    "gda_asn_diff_fwd_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, c_size_t, _P]),
    "gda_asn_diff_bwd_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P]),
    "gda_asn_ppmi_count": (c_int, [_P, c_int64, c_int64, _P, _P]),
    "gda_asn_ppmi_fill": (c_int, [_P, c_int64, c_int64, _P, c_int64, _P, _P, _P, _P, _P]),
    "gda_dgda_bits_workspace_bytes": (c_size_t, [c_int64]),
    "gda_dgda_manip_bits": (c_int, [_P, _P, _P, c_int64, c_float, c_float, ctypes.c_uint64, _P, ctypes.c_uint32, _P, _P,
                                    _P, _P, _P, c_size_t, _P]),
    "gda_dgda_pack_bits_f32": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_dgda_bitadj_gemm_f32": (c_int, [_P, c_int64, _P, _P, c_int64, c_int64, _P, _P, c_int64, _P]),
    "gda_dgda_recon_bits_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_dgda_recon_bits_f32": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, _P, _P, c_int64, _P, c_size_t, _P]),
    "gda_dgda_walks": (c_int, [_P, _P, c_int64, _P, c_int64, c_int64, ctypes.c_uint64, _P, ctypes.c_uint32, _P, _P]),
    "gda_jhgda_prox_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_jhgda_prox_f32": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, c_int64, _P, _P, c_int64, _P,
                                   c_int64, _P, c_size_t, _P]),
    "gda_jhgda_pool_rows_fwd_f32": (c_int, [_P, c_int64, c_int64, c_int64, _P, c_int64, _P, _P, _P]),
    "gda_jhgda_pool_rows_bwd_f32": (c_int, [_P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_int64, _P, c_int64,
                                            _P]),
    "gda_csr_to_coo": (c_int, [_P, _P, c_int64, c_int64, _P, _P, _P]),
    "gda_spmm_csr_f32": (c_int, [_P, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, _P]),
    "gda_spmm_csr_tout_f32": (c_int, [_P, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, _P]),
    "gda_spmm_csr_kstep_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_int, _P, c_int64, _P, c_int64,
                                       _P, _P, _P]),
    "gda_spmm_csr_interior_kstep_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_int64, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "gda_interior_max_rows": (c_int, []),
    "gda_interior_max_width": (c_int, []),
    "gda_interior_plan_bytes": (c_size_t, []),
    "gda_interior_kstep_lds_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_interior_plan_build": (c_int, [_P, _P, _P, _P, _P, c_size_t, _P, _P]),
    "gda_interior_kstep_lds_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_int64, c_int, c_int, _P, _P, _P, _P, _P,
                                           c_size_t, _P]),
    "gda_interior_kstep_lds_act_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_int64, c_int, _P, _P, _P, _P, _P,
                                               ctypes.c_float, ctypes.c_uint64, _P, ctypes.c_uint32, ctypes.c_uint32,
                                               _P, c_size_t, _P]),
    "gda_row_split_workspace_bytes": (c_size_t, [c_int64]),
    "gda_row_split_build": (c_int, [_P, c_int64, ctypes.c_int32, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_spmm_csr_split_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_int, _P, c_int64, _P, c_int64,
                                       _P, _P, _P, _P]),
    "gda_mmd_workspace_bytes": (c_size_t, [c_int, c_int64, c_int64]),
    "gda_mmd_fwd_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, _P, _P, c_int, c_int64, c_float,
                                c_int, c_float, _P, _P, _P, _P, c_size_t, _P]),
    "gda_mmd_bwd_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, _P, _P, c_int, c_int64, c_float,
                                c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_mmd_fwd_ex_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, _P, _P, c_int, c_int64, c_float, c_int, c_float,
                                   c_float, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_mmd_fwd_gather_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, _P, _P, c_int, c_int64, c_float, c_int, c_float,
                                       c_float, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_mmd_bwd_ex_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, _P, _P, c_int, c_int64, c_float, c_int,
                                   _P, _P, _P, c_float, _P, _P, _P, c_int64, _P, _P, _P, c_int64, _P,
                                   _P, c_size_t, _P]),
    "gda_mmd_fused_nseg": (c_int, [c_int, c_int64, c_int64, c_float, c_int]),
    "gda_mmd_fused_layout": (c_int, [c_int, c_int64, c_int64, _P, c_int]),
    "gda_mmd_fused_fwd_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, _P, _P, c_int, c_int64, c_float, c_int, c_float,
                                      c_float, _P, _P, _P, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "gda_mmd_fused_bwd_f32": (c_int, [_P, c_int, c_int, c_int64, c_int64, _P, c_float, _P,
                                      _P, _P, c_int64, _P, _P, _P, c_int64, _P, _P]),
    "gda_mmd_fused_bwd_mask_f32": (c_int, [_P, c_int, c_int, c_int64, c_int64, _P, c_float, _P,
                                           _P, _P, c_int64, _P, _P, _P, c_int64, _P, _P, c_float, _P, c_float, _P]),
    "gda_mmd_fused_fwd_act_cm_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, c_int64, _P, _P, c_int, c_int64, c_float, c_int,
                                             c_float, c_float, _P, _P, _P, _P, _P, _P, c_int, c_float, ctypes.c_uint64, _P,
                                             ctypes.c_uint32, _P, c_size_t, _P]),
    "gda_mmd_fused_bwd_act_cm_f32": (c_int, [_P, c_int, c_int, c_int64, c_int64, _P, c_float, _P, _P, c_int64, _P, _P, _P,
                                             c_int64, _P, _P, c_int64, c_float, ctypes.c_uint64, _P, ctypes.c_uint32, _P,
                                             c_float, _P]),
    "gda_copy_from_pinned": (c_int, [_P, _P, c_size_t, _P]),
    "gda_softmax_entropy_fwd_f32": (c_int, [_P, c_int64, c_int64, c_int, c_float, _P, _P, c_size_t, _P]),
    "gda_softmax_entropy_bwd_f32": (c_int, [_P, c_int64, c_int64, c_int, c_float, _P, _P, c_int64, _P]),
    "gda_mmd_chunked_plan": (c_int, [c_int, c_int64, c_int64, c_float, c_int, _P, c_int]),
    "gda_mmd_chunked_workspace_bytes": (c_size_t, [c_int, c_int64, c_int64]),
    "gda_mmd_chunked_fwd_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, _P, _P, c_int, c_int64, c_float, c_int, c_float,
                                        c_float, _P, _P, _P, c_int64, _P, _P, _P, c_int64, c_int, _P, c_size_t, _P]),
    "gda_mmd_fused_bwd_ld_f32": (c_int, [_P, c_int64, c_int, c_int, c_int64, c_int64, _P, c_float, _P,
                                         _P, _P, c_int64, _P, _P, _P, c_int64, _P, _P, c_float, _P, c_float, _P]),
    "gda_gemm_tall_fwd_ex_f32": (c_int, [c_int64, c_int64, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int,
                                         c_float, ctypes.c_uint64, _P, ctypes.c_uint32, ctypes.c_uint32, _P]),
    "gda_gemm_tall_wgrad_gather_f32": (c_int, [c_int64, c_int64, _P, c_int64, _P, c_int64, _P, _P, c_int64, _P, _P, c_size_t, _P]),
    "gda_gemm_nn_mask_f32": (c_int, [c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_float, _P]),
    "gda_gemm_act_cm_f32": (c_int, [c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, _P, c_int64, c_float,
                                    ctypes.c_uint64, _P, ctypes.c_uint32, _P]),
    "gda_gemm_act_cm_bwd_f32": (c_int, [c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_float, _P, _P, _P, c_size_t,
                                        _P]),
    "gda_gemm_skinny_act_cm_f32": (c_int, [c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, c_float,
                                           ctypes.c_uint64, _P, ctypes.c_uint32, _P]),
    "gda_grl_disc_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int]),
    "gda_grl_mlp_ce_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_lsgan_head_workspace_bytes": (c_size_t, [c_int64]),
    "gda_lsgan_head_fwd_f32": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, c_float, _P, _P, _P, c_size_t, _P]),
    "gda_lsgan_head_bwd_f32": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, c_float, _P, _P, c_int64, _P, _P,
                                       _P, c_size_t, _P]),
    "gda_grl_mlp_ce_fwd_f32": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P,
                                       c_float, ctypes.c_uint64, _P, ctypes.c_uint32, _P, _P, c_size_t, _P]),
    "gda_grl_mlp_ce_bwd_f32": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P,
                                       c_float, ctypes.c_uint64, _P, ctypes.c_uint32, _P, c_int, c_float, _P,
                                       _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_mlp_head_fwd_f32": (c_int, [c_int, _P, c_int64, c_int64, _P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P,
                                     c_float, ctypes.c_uint64, _P, ctypes.c_uint32, _P, _P, c_size_t, _P]),
    "gda_mlp_head_bwd_f32": (c_int, [c_int, _P, c_int64, c_int64, _P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P,
                                     c_float, ctypes.c_uint64, _P, ctypes.c_uint32, _P, c_int, c_float, _P,
                                     _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_grl_disc_ce_fwd_f32": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, c_int64, c_int,
                                        _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_grl_disc_ce_bwd_f32": (c_int, [_P, c_int64, c_int64, _P, c_int64, c_int64, c_int64, c_int,
                                        _P, _P, _P, _P, c_float, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_relu_dropout_fwd_f32": (c_int, [_P, _P, c_int64, c_float, ctypes.c_uint64, _P, ctypes.c_uint32, _P]),
    "gda_relu_dropout_bwd_f32": (c_int, [_P, _P, _P, c_int64, c_float, _P]),
    "gda_relu_dropout_tiled_fwd_f32": (c_int, [_P, c_int64, c_int64, _P, c_float, ctypes.c_uint64, _P, ctypes.c_uint32, _P]),
    "gda_gather_rows_f32": (c_int, [_P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P]),
    "gda_segment_mean_fwd_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, _P, c_int64, _P]),
    "gda_segment_mean_bwd_f32": (c_int, [_P, c_int64, _P, _P, c_int64, c_int64, _P, c_int64, _P]),
    "gda_sampler_create": (c_int, [_P, _P, c_int64, c_int64, ctypes.POINTER(c_void_p)]),
    "gda_sampler_destroy": (None, [_P]),
    "gda_sampler_set_threads": (c_int, [_P, c_int]),
    "gda_sampler_sample": (c_int, [_P, _P, c_int64, _P, c_int, ctypes.c_uint64,
                                   ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "gda_sampler_fetch": (c_int, [_P, _P, _P, _P]),
    "gda_sampler_csr_norm": (c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "gda_dsampler_graph_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_dsampler_build_graph": (c_int, [_P, _P, c_int64, c_int64, _P, _P, _P, _P, c_size_t, _P]),
    "gda_dsampler_caps": (c_int, [c_int64, _P, c_int, c_int64, c_int64, c_int64, _P, _P]),
    "gda_dsampler_workspace_bytes": (c_size_t, [c_int64, _P, c_int, c_int64, c_int64, c_int64]),
    "gda_dsampler_sample": (c_int, [_P, _P, c_int64, c_int64, c_int64, _P, c_int64, _P, c_int, ctypes.c_uint64,
                                    _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_event_create": (c_int, [_P]),
    "gda_event_destroy": (c_int, [_P]),
    "gda_event_record": (c_int, [_P, _P]),
    "gda_event_synchronize": (c_int, [_P]),
    "gda_stream_wait_event": (c_int, [_P, _P]),
    "gda_dsampler_batch": (c_int, [_P, _P, c_int64, c_int64, c_int64, _P, c_int64, _P, _P, c_int, ctypes.c_uint64,
                                   _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P, _P, _P, _P, c_size_t, _P]),
    "gda_dsampler_batch_ex": (c_int, [_P, _P, c_int64, c_int64, c_int64, _P, c_int64, _P, _P, c_int, ctypes.c_uint64,
                                      _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P, _P, _P, c_int64, _P,
                                      c_size_t, _P]),
    "gda_selection_csr_host": (c_int, [_P, c_int, c_int64, c_int64, c_int64, c_int64, _P, _P]),
    "gda_ppmi_build_host": (c_int, [_P, _P, c_int64, c_int64, c_int, c_int, ctypes.c_uint64,
                                    ctypes.POINTER(c_void_p)]),
    "gda_ppmi_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int]),
    "gda_ppmi_build": (c_int, [_P, _P, c_int64, c_int64, c_int, c_int, ctypes.c_uint64, _P, _P, _P, _P, _P,
                               c_size_t, _P]),
    "gda_edge_list_size": (c_int64, [_P]),
    "gda_edge_list_fetch": (c_int, [_P, _P, _P, _P]),
    "gda_edge_list_destroy": (None, [_P]),
    "gda_spmm_csr_axpby_f32": (c_int, [_P, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, c_float, c_float,
                                       _P, c_int64, c_float, _P, _P, _P]),
    "gda_kstep_max_rows": (c_int, []),
    "gda_kstep_plan_bytes": (c_size_t, [c_int]),
    "gda_kstep_plan_host": (c_int, [_P, _P, _P, c_int64, _P, c_size_t]),
    "gda_kstep_plan_host_ex": (c_int, [_P, _P, _P, c_int64, c_int, _P, c_size_t]),
    "gda_kstep_lds_f32": (c_int, [_P, c_int, c_int64, c_int64, c_int, _P, c_int64, c_int, _P, c_int64, c_int,
                                  _P, _P, _P, _P]),
    "gda_kstep_lds_colmajor_f32": (c_int, [_P, c_int, c_int64, c_int64, c_int, _P, c_int64, _P, c_int64, _P, _P, _P]),
    "gda_relu_dropout_pair_fwd_f32": (c_int, [_P, _P, c_int64, c_int64, c_float, ctypes.c_uint64, _P, ctypes.c_uint32,
                                              ctypes.c_uint32, _P]),
    "gda_relu_dropout_pair_workspace_bytes": (ctypes.c_size_t, [c_int64]),
    "gda_relu_dropout_pair_bwd_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_float, _P, _P, ctypes.c_size_t, _P]),
    "gda_stack2_f32": (c_int, [_P, _P, _P, c_int64, _P]),
    "gda_relu_dropout_bwd2_f32": (c_int, [_P, _P, _P, _P, c_int64, ctypes.c_float, _P]),
    "gda_colsum_workspace_bytes": (ctypes.c_size_t, [c_int64, c_int64]),
    "gda_colsum_f32": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, ctypes.c_size_t, _P]),
    "gda_softmax_nll_fwd_ex_f32": (c_int, [_P, c_int64, _P, c_int64, c_int, _P, _P, _P, ctypes.c_size_t, _P]),
    "gda_mixup_combine_workspace_bytes": (ctypes.c_size_t, [c_int64, c_int64]),
    "gda_mixup_combine_fwd_f32": (c_int, [_P, _P, _P, c_int, _P, _P, c_int64, c_int64, c_float, c_float, ctypes.c_uint64,
                                          _P, ctypes.c_uint32, ctypes.c_uint32, _P, _P, _P]),
    "gda_mixup_combine_bwd_f32": (c_int, [_P, _P, _P, _P, c_int, c_int64, c_int64, c_float, c_float, _P, _P, _P, _P, _P,
                                          ctypes.c_size_t, _P]),
    "gda_relu_dropout_fwd_cm_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, c_float, ctypes.c_uint64, _P,
                                           ctypes.c_uint32, _P]),
    "gda_relu_dropout_bwd_cm_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_int64, c_float, _P]),
    "gda_transpose_f32": (c_int, [_P, c_int64, _P, c_int64, c_int64, c_int64, _P]),
    "gda_wgan_critic_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int, c_int]),
    "gda_wgan_critic_f32": (c_int, [_P, c_int64, _P, c_int64, c_int, _P, _P, _P, c_int64, _P, _P, _P, _P, c_int,
                                    c_float, ctypes.c_uint64, _P, ctypes.c_uint32, c_float, _P, _P, _P, _P, _P,
                                    _P, c_size_t, _P]),
    "gda_wgan_critic_adam_f32": (c_int, [_P, c_int64, _P, c_int64, c_int, _P, _P, _P, c_int64, c_int,
                                         c_float, ctypes.c_uint64, _P, ctypes.c_uint32, c_float, _P, _P,
                                         c_float, c_float, c_float, c_float, c_float, _P, c_size_t, _P]),
    "gda_critic3_rows_per_trip": (c_int, []),
    "gda_critic3_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int]),
    "gda_critic3_update_f32": (c_int, [_P, c_int64, _P, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                       _P, c_size_t, _P]),
    "gda_critic3_update_adam_f32": (c_int, [_P, c_int64, _P, c_int64, c_int, _P, _P, c_float, c_float, c_float, c_float,
                                            c_float, _P, c_size_t, _P]),
    "gda_critic3_gap_f32": (c_int, [_P, c_int64, _P, c_int64, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_spectral_hinge_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_spectral_hinge_f32": (c_int, [_P, c_int64, c_int64, c_float, c_float, c_float, c_float, _P, _P, _P, c_size_t, _P]),
    "gda_laplacian_workspace_bytes": (c_size_t, [c_int64]),
    "gda_laplacian_fwd_f32": (c_int, [_P, _P, c_int64, c_int, _P, c_int64, _P, _P, _P, c_size_t, _P]),
    "gda_laplacian_bwd_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int, _P, c_int64, _P, _P, _P, c_int64, _P]),
    "gda_softmax_nll_workspace_bytes": (c_size_t, []),
    "gda_softmax_nll_fwd_f32": (c_int, [_P, c_int64, _P, c_int64, c_int, _P, _P, c_size_t, _P]),
    "gda_softmax_nll_bwd_f32": (c_int, [_P, c_int64, _P, c_int64, c_int, _P, _P, c_int64, _P]),
    "gda_softmax_nll_fwd_nv_f32": (c_int, [_P, c_int64, _P, c_int64, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "gda_softmax_nll_bwd_nv_f32": (c_int, [_P, c_int64, _P, c_int64, c_int, _P, _P, _P, c_int64, _P]),
    "gda_gemm_workspace_bytes": (c_size_t, [c_int, c_int64, c_int64, c_int64]),
    "gda_gemm_f32": (c_int, [c_int, c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64,
                             _P, c_size_t, _P]),
    "gda_gemm_ex_f32": (c_int, [c_int, c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P,
                                _P, c_size_t, _P]),
    "gda_gemm_skinny_workspace_bytes": (c_size_t, [c_int, c_int64, c_int64, c_int64]),
    "gda_gemm_skinny_f32": (c_int, [c_int, c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P,
                                    _P, c_size_t, _P]),
    "gda_gemm_tall_workspace_bytes": (c_size_t, [c_int, c_int64, c_int64, c_int64]),
    "gda_gemm_tall_f32": (c_int, [c_int, c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P,
                                  _P, c_size_t, _P]),
    "gda_attention_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_attention_fuse_fwd_f32": (c_int, [c_int, _P, _P, c_int64, c_int64, _P, _P, _P, c_int64, _P, _P]),
    "gda_attention_fuse_bwd_f32": (c_int, [c_int, _P, _P, c_int64, c_int64, _P, _P, _P, c_int64, _P, _P, _P, _P, c_size_t, _P]),
    "gda_adam_multi_f32": (c_int, [_P, c_int, c_float, c_float, c_float, c_float, c_float, _P]),
    "gda_adam_multi_ex_f32": (c_int, [_P, c_int, c_float, c_float, c_float, c_float, c_float, c_int, _P]),
    "gda_adam_multi_sum_f32": (c_int, [_P, _P, c_int, c_float, c_float, c_float, c_float, c_float, c_int, _P]),
    "gda_step_bump": (c_int, [_P, _P, c_int, _P]),
    "gda_rccl_load": (c_int, [ctypes.c_char_p]),
    "gda_comm_unique_id": (c_int, [_P, c_size_t]),
    "gda_comm_init_rank": (c_int, [_P, c_size_t, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "gda_comm_destroy": (c_int, [_P]),
    "gda_allreduce_f32": (c_int, [_P, c_int64, _P, _P]),
    "gda_allgather_f32": (c_int, [_P, _P, c_int64, _P, _P]),
    "gda_two_hop_host": (c_int, [_P, _P, c_int64, c_int64, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "gda_sepa_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "gda_sepa_stats_f32": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P]),
    "gda_sepa_group_sum_f32": (c_int, [_P, c_int64, _P, _P, c_int64, c_int64, c_int64, c_int, c_float, _P, _P, _P, _P,
                                       c_size_t, _P]),
    "gda_sepa_class_mean_bwd_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int64, c_int64, c_float, _P, _P]),
    "gda_sepa_mid_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int64, c_int64, _P, _P, _P, _P]),
    "gda_sepa_unbias_rows_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int64, c_int64, _P, _P]),
    "gda_sepa_row_weight_f32": (c_int, [_P, _P, c_int64, c_int64, _P, _P]),
    "gda_sepa_center_rows_bwd_f32": (c_int, [_P, _P, _P, _P, _P, _P, c_int64, c_int64, c_int64, _P, _P, _P]),
    "gda_sepa_unbias_rows_bwd_f32": (c_int, [_P, _P, _P, _P, _P, c_int64, c_int64, c_int64, _P, _P, _P, _P, c_size_t,
                                             _P]),
    "gda_sepa_mid_bwd_f32": (c_int, [_P, _P, _P, _P, _P, _P, c_float, c_int64, c_int64, c_int64, _P, _P, _P, _P]),
    "gda_sepa_dz_rows_f32": (c_int, [_P, _P, _P, _P, _P, _P, c_int64, c_int64, _P, _P]),
    "gda_sepa_proto_f32": (c_int, [_P, _P, c_int64, c_int64, c_float, c_float, c_float, _P, _P, _P, _P]),
    "gda_soga_ce_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_soga_smooth_ce_f32": (c_int, [_P, _P, c_int64, c_int64, c_float, _P, _P, _P, _P, c_size_t, _P]),
    "gda_soga_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    "gda_soga_adapt_f32": (c_int, [_P, c_int64, c_int64, _P, _P, _P, c_int64, c_int64, c_int64, c_float, c_float, _P, _P,
                                   c_int64, _P, _P, c_int64, _P, _P, _P, c_size_t, _P]),
    "gda_wgcn_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_wgcn_norm_f32": (c_int, [_P, _P, _P, _P, c_float, ctypes.c_uint64, _P, ctypes.c_uint32, _P, _P, _P, _P, _P, _P,
                                  _P, _P, c_size_t, _P]),
    "gda_wgcn_edge_grad_f32": (c_int, [_P, _P, _P, c_int64, _P, _P]),
    "gda_wgcn_norm_bwd_f32": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_gtrans_loss_workspace_bytes": (c_size_t, [c_int64]),
    "gda_gtrans_loss_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_float, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gda_gtrans_project_workspace_bytes": (c_size_t, [c_int64]),
    "gda_gtrans_project_f32": (c_int, [_P, c_int64, c_float, c_float, _P, c_size_t, _P]),
    "gda_cta_loss_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "gda_cta_model_loss_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int64, c_int64, c_float, c_float, _P, _P, _P, _P,
                                       c_size_t, _P]),
    "gda_cta_knn_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "gda_cta_knn_f32": (c_int, [_P, _P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, c_size_t, _P]),
    "gda_cta_tt_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "gda_cta_test_time_f32": (c_int, [_P, _P, _P, _P, _P, _P, c_int64, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P,
                                      _P, _P, c_size_t, _P]),
    "gda_kbl_pair_bce_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "gda_kbl_pair_bce_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, c_size_t, _P]),
    "gda_kbl_bridge_topk_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "gda_kbl_bridge_topk_f32": (c_int, [_P, _P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P, c_size_t, _P]),
    "gda_ata_gate_f32": (c_int, [_P, _P, c_int64, _P]),
    "gda_ata_gate_bwd_f32": (c_int, [_P, _P, _P, _P, c_int64, _P]),
    "gda_ata_sparsemax_f32": (c_int, [_P, c_int64, c_int64, _P, _P]),
    "gda_ata_sparsemax_bwd_f32": (c_int, [_P, _P, c_int64, c_int64, _P, _P]),
    "gda_ata_mix_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_int64, c_float, _P, _P, _P]),
    "gda_ata_mix_bwd_f32": (c_int, [_P, _P, _P, c_int64, c_int64, c_int64, c_float, _P, _P, _P, _P]),
    "gda_ata_head_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_ata_head_f32": (c_int, [_P, c_int64, c_int64, _P, _P, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, c_size_t,
                                 _P]),
    "gda_ata_vote_f32": (c_int, [_P, _P, c_int64, c_int64, c_int64, c_int64, _P, _P]),
    "gda_ata_memory_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_ata_memory_f32": (c_int, [_P, _P, c_int64, c_int64, c_int64, c_float, c_float, _P, _P, _P, c_size_t, _P]),
    "gda_pa_edge_stats_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "gda_pa_edge_stats_f64": (c_int, [_P, _P, _P, c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P,
                                      c_size_t, _P]),
    "gda_pa_softmax_sums_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_pa_softmax_sums_f64": (c_int, [_P, _P, _P, _P, c_int64, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, _P,
                                        c_size_t, _P]),
    "gda_pa_ce_workspace_bytes": (c_size_t, []),
    "gda_pa_ce_fwd_f32": (c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, _P, _P, c_size_t, _P]),
    "gda_pa_ce_bwd_f32": (c_int, [_P, _P, c_int64, c_int64, _P, c_int64, _P, _P, _P, _P]),
    "gda_pa_refresh_values_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int64, _P, _P, c_int64, c_float, c_float, c_int,
                                          _P]),
    "gda_collate_offsets": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P]),
    "gda_collate_nodes_f32": (c_int, [_P, c_int64, c_int64, _P, _P, _P, c_int64, _P, c_int64, _P, _P, _P, _P]),
    "gda_collate_edges": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, c_int64, c_int64, _P, _P]),
    "gda_collate_ppmi_f32": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, c_int64, c_int64, c_int, c_int64, _P,
                                     _P, _P]),
    "gda_collate_ppmi_csr_f32": (c_int, [_P, c_int64, c_int64, _P, _P, _P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, _P,
                                         c_int64, _P, _P, _P, c_int64, c_float, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gda_ppmi_build_ratio": (c_int, [_P, _P, c_int64, c_int64, c_int, c_int, ctypes.c_uint64, _P, _P, _P, _P, _P,
                                     c_size_t, _P]),
    "gda_collate_csr_offsets": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P]),
    "gda_collate_csr_f32": (c_int, [_P, c_int64, c_int64, _P, _P, _P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, _P,
                                    _P, _P, _P, _P, _P, _P, _P]),
    "gda_walk_smooth_host": (c_int, [_P, _P, c_int64, c_int64, c_int, ctypes.c_uint64, c_int,
                                     ctypes.POINTER(c_void_p)]),
    "gda_svd_lap_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int]),
    "gda_svd_lap_apply_f32": (c_int, [_P, _P, _P, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, _P, c_size_t, _P]),
    "gda_svd_lap_moments_f32": (c_int, [_P, _P, _P, c_int64, c_int64, _P, c_int64, _P, _P, _P, c_size_t, _P]),
    "gda_svd_gram_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_svd_gram_f32": (c_int, [_P, c_int64, c_int64, c_int64, _P, c_int64, _P, c_size_t, _P]),
    "gda_gmm_mstep_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "gda_gmm_mstep_f32": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, c_int64, _P, c_float, _P, _P, _P, _P, _P,
                                  c_size_t, _P]),
    "gda_gmm_factor_f32": (c_int, [_P, c_int64, c_int64, c_int64, _P, _P, _P, _P]),
    "gda_gmm_estep_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "gda_gmm_estep_f32": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P, _P, ctypes.c_double,
                                  _P, _P, c_size_t, _P]),
    "gda_kmeans_step_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "gda_kmeans_step_f32": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, _P, c_int, _P, _P, _P, _P, _P, c_size_t,
                                    _P]),
    "gda_gmm_label_sums_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "gda_gmm_label_sums_f32": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, _P, _P, _P, _P, c_size_t, _P]),
    "gda_gmm_relabel_f32": (c_int, [_P, c_int64, c_int64, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gda_lsa_cos_f32": (c_int, [_P, _P, c_int64, c_int64, _P, _P, _P, _P]),
    "gda_lsa_cost_f64": (c_int, [_P, c_int64, _P, _P, _P, _P]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

class AdamTensorStruct(ctypes.Structure):
    """``gda_adam_tensor`` of include/gda_hip.h."""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
                ("step", c_void_p), ("numel", c_int64)]


class WgcnPlanStruct(ctypes.Structure):
    """``gda_wgcn_plan`` of include/gda_hip.h."""
    _fields_ = [(k, c_int64) for k in ("n", "nnz", "m", "mu", "nseg", "t_nseg", "mean", "ec")] + \
               [(k, c_void_p) for k in ("rowptr", "colidx", "t_rowptr", "t_colidx", "t_to_fwd", "erow", "epos", "kidx",
                                        "pent", "gptr", "gidx", "pgrp", "seg_off", "row_seg", "t_seg_off", "t_row_seg")]


class RowSplitStruct(ctypes.Structure):
    """``gda_row_split`` of include/gda_hip.h."""
    _fields_ = [("threshold", ctypes.c_int32), ("n_long", ctypes.c_int32), ("n_chunks", ctypes.c_int32),
                ("long_rows", c_void_p), ("long_chunk_ptr", c_void_p), ("chunk_long", c_void_p),
                ("scratch", c_void_p), ("counts_dev", c_void_p)]


_lib = None


class GdaError(RuntimeError):
    pass


def lib():
    """The loaded library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GdaError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(pygda_amd has no CPU / eager fallback)")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


_DEBUG_SYNC = os.environ.get("PYGDA_AMD_DEBUG_SYNC") == "1"


def check(status, what):
    if _DEBUG_SYNC:                       # serialise and name every C-ABI call (debugging aid)
        import sys
        print("[gda] launched", what, file=sys.stderr, flush=True)
        torch.cuda.synchronize()
        print("[gda] done    ", what, file=sys.stderr, flush=True)
    if status != 0:
        msg = lib().gda_status_string(int(status)).decode()
        raise GdaError(f"{what} failed with status {status}: {msg}")


def call(name, *args):
    """Call the status-returning entry point ``name``; a non-zero status raises a GdaError that names it.  Pointer
    arguments are tensors (or None), scalars plain Python numbers: ``_SIGNATURES`` converts both.  The stream is an
    explicit argument -- ``stream()`` -- because the caller decides which stream is current."""
    check(getattr(lib(), name)(*args), name)


def ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


def stream():
    """The raw handle of torch's current stream on the current device.  (``torch.cuda.current_stream()`` builds a
    Stream object per call: ~10 us, a hundred times per eager training step.)"""
    return c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def require_gpu_tensor(t, name, dtype=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise GdaError(f"{name} must be a tensor on the MI355X device (got {getattr(t, 'device', type(t))}); "
                       "pygda_amd has no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise GdaError(f"{name} must have dtype {dtype}, got {t.dtype}")
    return t


_ws_cache = {}


def workspace(nbytes, device, tag):
    """A reusable byte scratch buffer per (device, tag, stream): kernels never allocate."""
    key = (str(device), tag, torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def scratch(size_fn_name, device, tag, *dims):
    """``(buffer, nbytes)``: the workspace that ``size_fn_name(*dims)`` asks for, from the cache entry ``tag``."""
    nbytes = getattr(lib(), size_fn_name)(*dims)
    return workspace(nbytes, device, tag), nbytes
