"""sparsify.me_amd -- ctypes front end of libsparsifyme.so (the gfx950 HIP back end).

This package is plumbing for tests and bench.py: it hands torch-owned device pointers to the
C ABI declared in include/sparsifyme.h.  There is NO CPU fallback here: if the HIP library is
missing or a call fails, the functions raise.  The C++ mirror of the reference's operator API
lives in include/sparsify.me/*.hxx; the function names below follow it
(sparsify, spmma, batched gemm -- reference include/sparsify.me/{sparsify,spmma,gemm}.hxx).

The directory name contains a dot, so import it through __graft_entry__.load_package(), which
registers it as module `sparsifyme_amd`.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPARSIFYME_LIB: another build of the library to load; default is the in-tree product library
LIB_PATH = os.environ.get("SPARSIFYME_LIB") or os.path.join(_HERE, "libsparsifyme.so")

PRUNE_TILE = 0
PRUNE_STRIP = 1
# include/sparsifyme.h: SM_STATUS_*
STATUS_SUCCESS, STATUS_INVALID_VALUE, STATUS_NOT_SUPPORTED, STATUS_LAUNCH_FAILED, STATUS_NO_DEVICE = 0, 1, 2, 3, 4

_lib = None

_c_size = ctypes.c_size_t
_c_ptr = ctypes.c_void_p
_c_f = ctypes.c_float
_c_i = ctypes.c_int

# name -> argtypes (restype is always int unless listed in _RET)
_SIGS = {
    "sm_device_check": [],
    "sm_sparsify_positional": [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_f, _c_ptr],
    "sm_sparsify_positional_f16": [_c_ptr, _c_ptr, _c_size, _c_size, _c_f, _c_ptr],
    "sm_sparsify_positional_f32": [_c_ptr, _c_ptr, _c_size, _c_size, _c_f, _c_ptr],
    "sm_sparsify_positional_f64": [_c_ptr, _c_ptr, _c_size, _c_size, _c_f, _c_ptr],
    "sm_prune24_f16": [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_i, _c_ptr],
    "sm_prune24_f32": [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_i, _c_ptr],
    "sm_prune24_check_f16": [_c_ptr, _c_size, _c_size, _c_size, _c_ptr, _c_ptr],
    "sm_prune24_check_f32": [_c_ptr, _c_size, _c_size, _c_size, _c_ptr, _c_ptr],
    "sm_compress24_size": [_c_size, _c_size, _c_size, _c_size, ctypes.POINTER(_c_size)],
    "sm_compress24_f16": [_c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr],
    "sm_compress24_f32": [_c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr],
    "sm_decompress24_f16": [_c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr],
    "sm_decompress24_f32": [_c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr],
    "sm_spmma_f16": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_f, _c_f, _c_ptr],
    "sm_spmma_f32": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_f, _c_f, _c_ptr],
    "sm_spmma_fused_f16": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size,
                           _c_f, _c_f, _c_ptr],
    "sm_spmma_fused_f32": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size,
                           _c_f, _c_f, _c_ptr],
    "sm_conv_spmma_workspace": [_c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, ctypes.POINTER(_c_size)],
    "sm_conv_spmma_f16": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_f, _c_f,
                          _c_ptr, _c_size, _c_ptr],
    "sm_conv_spmma_bf16": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_f, _c_f,
                           _c_ptr, _c_size, _c_ptr],
    "sm_gemm_rowmajor_f32_split": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_i,
                                   _c_ptr, _c_size, _c_f, _c_f, _c_ptr],
    "sm_spmma_f16_grouped": [_c_size, _c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_f, _c_f, _c_ptr],
    "sm_spmma_bf16_grouped": [_c_size, _c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_f, _c_f, _c_ptr],
    "sm_spmma_fused_f32_split_workspace": [_c_size, _c_size, _c_size, _c_size, _c_i, ctypes.POINTER(_c_size)],
    "sm_spmma_fused_f32_split": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_i,
                                 _c_ptr, _c_size, _c_f, _c_f, _c_ptr],
    "sm_spmma_fused_f16_grouped": [_c_size, _c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size,
                                   _c_size, _c_f, _c_f, _c_ptr],
    "sm_spmma_fused_bf16_grouped": [_c_size, _c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size,
                                    _c_size, _c_f, _c_f, _c_ptr],
    "sm_gemm_batched_f16": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_i, _c_i, _c_f, _c_f, _c_ptr],
    "sm_gemm_batched_f32": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_i, _c_i, _c_f, _c_f, _c_ptr],
    "sm_gemm_batched_f64": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_i, _c_i,
                            ctypes.c_double, ctypes.c_double, _c_ptr],
    "sm_gemm_rowmajor_f16": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size,
                             _c_size, _c_f, _c_f, _c_ptr],
    "sm_gemm_rowmajor_f32": [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size,
                             _c_size, _c_f, _c_f, _c_ptr],
    "sm_spmm_bell_f32": [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr, _c_size, _c_f, _c_f, _c_ptr],
    "sm_spmm_coo_f32": [_c_size, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_f, _c_f,
                        _c_ptr],
    "sm_spmm_bell_workspace_size": [_c_size, _c_size, ctypes.POINTER(_c_size)],
    "sm_spmm_bell_f32_ws": [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr, _c_size, _c_f, _c_f, _c_ptr,
                            _c_ptr],
    "sm_spmm_bell_batched_workspace_size": [_c_size, _c_size, _c_size, ctypes.POINTER(_c_size)],
    "sm_spmm_bell_batched_f32": [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr, _c_size, _c_size, _c_f,
                                 _c_f, _c_ptr, _c_ptr],
    "sm_spmm_coo_workspace_size": [_c_size, ctypes.POINTER(_c_size)],
    "sm_spmm_coo_packed_workspace_size": [_c_size, _c_size, ctypes.POINTER(_c_size)],
    "sm_spmm_coo_f32_packed": [_c_size, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_f, _c_f,
                               _c_ptr, _c_size, _c_ptr],
    "sm_spmm_coo_f32_ws": [_c_size, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_f, _c_f,
                           _c_ptr, _c_ptr],
    "sm_spmm_coo_fast_workspace_size": [_c_size, _c_size, _c_size, _c_size, ctypes.POINTER(_c_size)],
    "sm_spmm_coo_fast_flag": [_c_ptr, ctypes.POINTER(_c_i), _c_ptr],
    "sm_spmm_coo_fast_form": [_c_size, _c_size, _c_size, _c_size, _c_size, _c_f],
    "sm_spmm_coo_f32_fast": [_c_size, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_f, _c_f,
                             _c_ptr, _c_size, _c_ptr],
    "sm_fill_uniform_f16": [_c_ptr, _c_size, ctypes.c_uint64, _c_f, _c_f, _c_ptr],
    "sm_fill_uniform_f32": [_c_ptr, _c_size, ctypes.c_uint64, _c_f, _c_f, _c_ptr],
    "sm_copy_bytes": [_c_ptr, _c_ptr, _c_size, _c_ptr],
}
_SIGS["sm_prune24_compress24_f16"] = [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr, _c_i, _c_ptr]
_SIGS["sm_prune24_compress24_bf16"] = _SIGS["sm_prune24_compress24_f16"]
_SIGS["sm_prune24_spmma_f16"] = [_c_ptr, _c_ptr, _c_ptr, _c_ptr] + [_c_size] * 8 + [_c_i, _c_ptr, _c_f, _c_f, _c_ptr]
_SIGS["sm_prune24_spmma_bf16"] = _SIGS["sm_prune24_spmma_f16"]
_SIGS["sm_prune24_compress24_f32"] = _SIGS["sm_prune24_compress24_f16"]
_SIGS["sm_prune24_form"] = [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_i, ctypes.POINTER(_c_i), ctypes.POINTER(ctypes.c_uint)]
_SIGS["sm_prune24_check_form"] = [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, ctypes.POINTER(_c_i)]
_SIGS["sm_compress24_form"] = [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, ctypes.POINTER(_c_i)]
_SIGS["sm_decompress24_form"] = _SIGS["sm_compress24_form"]
_SIGS["sm_prune24_compress24_form"] = [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_size, _c_i, _c_size,
                                       ctypes.POINTER(_c_i), ctypes.POINTER(ctypes.c_uint)]
_SIGS["sm_conv_spmma_fused_f16"] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 10 + [_c_f, _c_f, _c_ptr]
_SIGS["sm_conv_spmma_fused_bf16"] = _SIGS["sm_conv_spmma_fused_f16"]
_SIGS["sm_conv_spmma_fused_plan"] = [_c_size] * 10 + [ctypes.c_uint, ctypes.POINTER(_c_i), ctypes.POINTER(ctypes.c_uint)]
_SIGS["sm_transpose"] = [_c_ptr, _c_ptr] + [_c_size] * 8 + [_c_ptr]
_SIGS["sm_conv_out_size"] = [_c_size, _c_size, _c_size, _c_size, _c_size, ctypes.POINTER(_c_size)]
_SIGS["sm_im2col_f16"] = [_c_ptr] + [_c_size] * 9 + [_c_ptr, _c_ptr]
_SIGS["sm_im2col_compress24_f16"] = [_c_ptr] + [_c_size] * 9 + [_c_ptr, _c_ptr]
for _name in ("sm_prune24", "sm_prune24_check", "sm_compress24", "sm_decompress24"):
    _SIGS[_name + "_i8"] = _SIGS[_name + "_f16"]
_SIGS["sm_spmma_fused_i8"] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 8 + [_c_i, _c_ptr]
_SIGS["sm_spmma_fused_i8_q"] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 8 + [_c_f, _c_ptr]
_SIGS["sm_transpose_i8"] = [_c_ptr, _c_ptr, _c_size, _c_size, _c_ptr]
_SIGS["sm_spmma_i8"] = [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_i, _c_ptr]
_SIGS["sm_spmma_i8_q"] = [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_size, _c_f, _c_ptr]
# bfloat16 forms: same signatures as their _f16 counterparts
for _name in ("sm_prune24", "sm_prune24_check", "sm_compress24", "sm_decompress24", "sm_spmma", "sm_spmma_fused",
              "sm_gemm_rowmajor", "sm_fill_uniform", "sm_im2col", "sm_im2col_compress24"):
    _SIGS[_name + "_bf16"] = _SIGS[_name + "_f16"]
_SIGS["sm_spmma_fused_f32_split_prepare"] = [_c_ptr, _c_size, _c_size, _c_size, _c_size, _c_i, _c_ptr, _c_size, _c_ptr]
_SIGS["sm_spmma_fused_f32_split_prepared"] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 8 + [_c_i, _c_size, _c_f, _c_f, _c_ptr]
_SIGS["sm_spmma_fused_workspace_size"] = [ctypes.POINTER(_c_size)]
_SIGS["sm_spmma_fused_workspace_state"] = [_c_ptr, ctypes.POINTER(_c_i), _c_ptr]
_SIGS["sm_spmma_fused_streamk_plan"] = [_c_size, _c_size, _c_size, _c_size, ctypes.POINTER(_c_i), ctypes.POINTER(ctypes.c_uint)]
_SIGS["sm_spmma_fused_form"] = [_c_size] * 9 + [_c_f, ctypes.c_uint, _c_size, ctypes.POINTER(_c_i)]
_SIGS["sm_gemm_rowmajor_f16_ws"] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 8 + [_c_f, _c_f, _c_ptr, _c_size, _c_ptr]
_SIGS["sm_gemm_rowmajor_bf16_ws"] = _SIGS["sm_gemm_rowmajor_f16_ws"]
_SIGS["sm_gemm_batched_f16_ws"] = [_c_ptr, _c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_i, _c_i, _c_f, _c_f, _c_ptr, _c_size, _c_ptr]
_SIGS["sm_spmma_fused_f16_ws"] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 8 + [_c_f, _c_f, _c_ptr, _c_size, _c_ptr]
_SIGS["sm_spmma_fused_bf16_ws"] = _SIGS["sm_spmma_fused_f16_ws"]
_SIGS["sm_spmma_fused_f16_grouped_ws"] = [_c_size, _c_ptr, _c_ptr, _c_ptr] + [_c_size] * 8 + [_c_f, _c_f, _c_ptr, _c_size, _c_ptr]
_SIGS["sm_spmma_fused_bf16_grouped_ws"] = _SIGS["sm_spmma_fused_f16_grouped_ws"]
# Blocked-ELL on the 16-bit matrix cores (spmm_bell16.hip)
_SIGS["sm_spmm_bell_f16"] = _SIGS["sm_spmm_bell_f32"]
_SIGS["sm_spmm_bell_bf16"] = _SIGS["sm_spmm_bell_f32"]
_SIGS["sm_spmm_bell_batched_f16"] = [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_ptr, _c_size, _c_size, _c_f, _c_f, _c_ptr]
_SIGS["sm_spmm_bell_batched_bf16"] = _SIGS["sm_spmm_bell_batched_f16"]
# OCP fp8 (e4m3 / e5m2) 2:4 path (spmma_fp8.hip)
_SIGS["sm_prune24_fp8"] = [_c_ptr, _c_ptr, _c_size, _c_size, _c_size, _c_i, _c_i, _c_ptr]
_SIGS["sm_prune24_check_fp8"] = _SIGS["sm_prune24_check_f16"]
_SIGS["sm_compress24_fp8"] = [_c_ptr, _c_size, _c_size, _c_size, _c_size, _c_size, _c_ptr, _c_i, _c_ptr]
_SIGS["sm_decompress24_fp8"] = _SIGS["sm_decompress24_f16"]
_SIGS["sm_spmma_fp8"] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 6 + [_c_i, _c_i, _c_i, _c_f, _c_f, _c_ptr, _c_ptr]
_SIGS["sm_spmma_fused_fp8"] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 8 + [_c_i, _c_i, _c_i, _c_f, _c_f, _c_ptr, _c_ptr]
# dense 1-byte GEMM (gemm_b8.hip): the signatures of the fused forms
_SIGS["sm_gemm_rowmajor_fp8"] = _SIGS["sm_spmma_fused_fp8"]
_SIGS["sm_gemm_rowmajor_i8"] = _SIGS["sm_spmma_fused_i8"]
_SIGS["sm_gemm_rowmajor_i8_q"] = _SIGS["sm_spmma_fused_i8_q"]
# fp8 quantisation of 16-bit operands (quant_fp8.hip)
for _sfx16 in ("f16", "bf16"):
    _SIGS["sm_quantize_rows_fp8_" + _sfx16] = [_c_ptr, _c_size, _c_size, _c_size, _c_ptr, _c_size, _c_ptr, _c_i, _c_ptr]
    _SIGS["sm_quantize_compress24_fp8_" + _sfx16] = [_c_ptr, _c_size, _c_size, _c_size, _c_ptr, _c_ptr, _c_i, _c_ptr]
    _SIGS["sm_quantize_transpose_fp8_" + _sfx16] = [_c_ptr, _c_size, _c_size, _c_size, _c_f, _c_ptr, _c_i, _c_ptr]
# bias / activation / residual epilogues of the 16-bit 2:4 matmul: the plain signature with a `const sm_epilogue_t*` before the stream
for _sfx16 in ("f16", "bf16"):
    _SIGS["sm_spmma_%s_ex" % _sfx16] = _SIGS["sm_spmma_f16"][:-1] + [_c_ptr, _c_ptr]
    _SIGS["sm_spmma_fused_%s_ex" % _sfx16] = _SIGS["sm_spmma_fused_f16"][:-1] + [_c_ptr, _c_ptr]
# the token-major 2:4 weight-sparse linear layer (linear24_f16.hip)
for _sfx16 in ("f16", "bf16"):
    _SIGS["sm_linear24_" + _sfx16] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 5 + [_c_f, _c_f, _c_ptr, _c_ptr]
# ... and its fp8 form (linear24_fp8.hip) with the host-side query of its dispatch rule
_SIGS["sm_linear24_fp8"] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 5 + [_c_i, _c_i, _c_i, _c_f, _c_f, _c_ptr, _c_ptr, _c_ptr, _c_ptr]
_SIGS["sm_linear24_fp8_form"] = [_c_size] * 4 + [ctypes.POINTER(_c_i)]
# the gated (gate/up) forms of both layers: one launch writes act(gate) * up
for _sfx16 in ("f16", "bf16"):
    _SIGS["sm_linear24_glu_" + _sfx16] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 5 + [_c_i, _c_ptr, _c_ptr]
_SIGS["sm_linear24_glu_fp8"] = [_c_ptr, _c_ptr, _c_ptr] + [_c_size] * 5 + [_c_i, _c_i, _c_i, _c_i, _c_ptr, _c_ptr, _c_ptr, _c_ptr]
_SIGS["sm_linear24_glu_form"] = [_c_size] * 4 + [ctypes.POINTER(_c_i)]
# the grouped (per-expert) forms: the plain signatures with (group_offsets, groups) in front of tokens
for _sfx16 in ("f16", "bf16", "fp8"):
    _SIGS["sm_linear24_grouped_" + _sfx16] = _SIGS["sm_linear24_" + _sfx16][:3] + [_c_ptr, _c_size] + _SIGS["sm_linear24_" + _sfx16][3:]
    _SIGS["sm_linear24_grouped_glu_" + _sfx16] = _SIGS["sm_linear24_glu_" + _sfx16][:3] + [_c_ptr, _c_size] + _SIGS["sm_linear24_glu_" + _sfx16][3:]
_SIGS["sm_linear24_grouped_form"] = [_c_size] * 5 + [ctypes.POINTER(_c_i)]
# ... with X gathered through a row index: (x_index, x_rows) directly after group_offsets
for _sfx16 in ("f16", "bf16", "fp8"):
    for _g in ("sm_linear24_grouped_", "sm_linear24_grouped_glu_"):
        _SIGS[_g + "gather_" + _sfx16] = _SIGS[_g + _sfx16][:4] + [_c_ptr, _c_size] + _SIGS[_g + _sfx16][4:]
# MoE routing (moe_route.hip) and combine (moe_combine.hip)
_SIGS["sm_moe_route_workspace_size"] = [_c_size] * 3 + [ctypes.POINTER(_c_size)]
_SIGS["sm_moe_route"] = [_c_ptr] + [_c_size] * 3 + [_c_ptr] * 5 + [_c_size, _c_ptr]
_SIGS["sm_moe_route_form"] = [_c_size] * 3 + [ctypes.POINTER(_c_i)]
for _sfx16 in ("f16", "bf16"):
    _SIGS["sm_moe_combine_" + _sfx16] = [_c_ptr] * 5 + [_c_size] * 6 + [_c_ptr]
_SIGS["sm_moe_combine_form"] = [_c_ptr] * 3 + [_c_size] * 3 + [ctypes.POINTER(_c_i)]
# MoE gate (moe_gate.hip): logits -> top_k ids and weights
for _sfx3 in ("f16", "bf16", "f32"):
    _SIGS["sm_moe_gate_" + _sfx3] = [_c_ptr] * 4 + [_c_size] * 4 + [_c_i, _c_i, _c_f, _c_ptr]
_SIGS["sm_moe_gate_form"] = [_c_size] * 3 + [ctypes.POINTER(_c_i)]
# residual add + RMSNorm with an optional fp8 output (rmsnorm.hip)
for _sfx16 in ("f16", "bf16"):
    _SIGS["sm_rmsnorm_" + _sfx16] = [_c_ptr] * 7 + [_c_size] * 6 + [_c_f, _c_i, _c_ptr]
_SIGS["sm_rmsnorm_form"] = [_c_size, ctypes.POINTER(_c_i)]
# paged-KV decode attention (attn_decode.hip)
for _sfx16 in ("f16", "bf16"):
    _SIGS["sm_attn_decode_" + _sfx16] = [_c_ptr] * 8 + [_c_size] * 13 + [_c_f, _c_ptr]
_SIGS["sm_attn_decode_workspace_size"] = [_c_size] * 5 + [ctypes.POINTER(_c_size)]
_SIGS["sm_attn_decode_form"] = [_c_size] * 6 + [ctypes.POINTER(_c_i)]
# RoPE + paged KV-cache append (rope_append.hip)
for _sfx16 in ("f16", "bf16"):
    _SIGS["sm_rope_append_" + _sfx16] = [_c_ptr] * 12 + [_c_size] * 19 + [_c_i, _c_ptr]
_SIGS["sm_rope_append_form"] = [_c_size] * 5 + [ctypes.POINTER(_c_i)]
# the fp8 paged KV cache: quantising append (rope_append_kv8.hip) and decode attention (attn_decode_kv8.hip)
for _sfx16 in ("f16", "bf16"):
    _SIGS["sm_rope_append_kv8_" + _sfx16] = [_c_ptr] * 14 + [_c_size] * 20 + [_c_i, _c_i, _c_ptr]
    _SIGS["sm_attn_decode_kv8_" + _sfx16] = [_c_ptr] * 10 + [_c_size] * 14 + [_c_f, _c_i, _c_ptr]
_RET = {"sm_version": ctypes.c_char_p, "sm_last_error": ctypes.c_char_p}

# every symbol include/sparsifyme.h declares (checked by tests/test_abi.py without a GPU)
EXPORTED_SYMBOLS = sorted(list(_SIGS) + list(_RET))


class SparsifymeError(RuntimeError):
    pass


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 into libsparsifyme.so (hipcc cross-compiles without a GPU)."""
    res = subprocess.run(["make", "-C", _HERE, "-j4"], capture_output=not verbose, text=True)
    if res.returncode != 0:
        raise SparsifymeError("building libsparsifyme.so failed:\n" + (res.stdout or "") + (res.stderr or ""))
    return LIB_PATH


def lib():
    """The loaded HIP library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SparsifymeError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback for the product path)")
        L = ctypes.CDLL(LIB_PATH)
        for name, args in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = ctypes.c_int
        for name, ret in _RET.items():
            fn = getattr(L, name)
            fn.argtypes = []
            fn.restype = ret
        _lib = L
    return _lib


def _check(status, what):
    if status != 0:
        msg = lib().sm_last_error().decode()
        raise SparsifymeError(f"{what} failed with status {status}: {msg}")


_torch = None
_SFX = None


def _t():
    global _torch, _SFX
    if _torch is None:
        import torch
        _torch = torch
        _SFX = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32", torch.float64: "f64", torch.int8: "i8"}
    return _torch


def _stream():
    return ctypes.c_void_p(_t().cuda.current_stream().cuda_stream)


def _dev(t):
    if not t.is_cuda:
        raise SparsifymeError("expected a device tensor (the product path has no host implementation)")
    return ctypes.c_void_p(t.data_ptr())


def _sfx(t):
    _t()
    return _SFX[t.dtype]


def graph_time_ms(fn, iters=20, replays=3):
    """Device time of one call of `fn` in ms: `iters` calls are captured into one hipGraph (so the
    host-side ctypes/launch cost is not on the clock) and the graph is replayed `replays` times
    between two HIP events on the capture stream's parent.  fn must only enqueue work on the
    current stream."""
    torch = _t()
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (iters * replays)


def version():
    return lib().sm_version().decode()


def device_check():
    _check(lib().sm_device_check(), "sm_device_check")


# ---- operators -------------------------------------------------------------------------------
def sparsify(weights, mask, m, n, sparsity_factor=0.5, blk_m=2, blk_n=2):
    """sparsifyme::sparsify<BLK_M,BLK_N> (sparsify.hxx:24-30): in place on `weights`
    (m*n elements) and `mask` (m*n int64/uint64)."""
    assert weights.numel() >= m * n and mask.numel() >= m * n and mask.element_size() == 8
    _check(lib().sm_sparsify_positional(_dev(weights), _dev(mask), m, n, weights.element_size(), blk_m, blk_n,
                                        float(sparsity_factor), _stream()), "sm_sparsify_positional")


def prune24(A_in, A_out, m, k, ld, alg=PRUNE_STRIP):
    fn = getattr(lib(), "sm_prune24_" + _sfx(A_in))
    _check(fn(_dev(A_in), _dev(A_out), m, k, ld, alg, _stream()), "sm_prune24")


def prune24_check(A, m, k, ld, d_valid):
    fn = getattr(lib(), "sm_prune24_check_" + _sfx(A))
    _check(fn(_dev(A), m, k, ld, _dev(d_valid), _stream()), "sm_prune24_check")


def compress24_size(m, k, elt_bytes, batch=1):
    out = ctypes.c_size_t(0)
    _check(lib().sm_compress24_size(m, k, elt_bytes, batch, ctypes.byref(out)), "sm_compress24_size")
    return out.value


def compress24(A, m, k, ld, batch, strideA, blob):
    fn = getattr(lib(), "sm_compress24_" + _sfx(A))
    _check(fn(_dev(A), m, k, ld, batch, strideA, _dev(blob), _stream()), "sm_compress24")


def prune24_compress24(A_in, A_out, m, k, ld, batch, strideA, blob, d_valid, alg=PRUNE_TILE):
    """prune -> check -> compress in one pass (spmma.hxx:82-104); A_out / blob / d_valid may be None."""
    fn = getattr(lib(), "sm_prune24_compress24_" + _sfx(A_in))
    opt = lambda t: _dev(t) if t is not None else None
    _check(fn(_dev(A_in), opt(A_out), m, k, ld, batch, strideA, opt(blob), opt(d_valid), alg, _stream()), "sm_prune24_compress24")


API_SPMMA_SEQUENCE = ("sm_prune24_compress24 (TILE prune out of place from the dense A + check flag + blob, one pass) -> "
                      "sm_spmma; the flag stays on the device (the reference reads it back and synchronises, spmma.hxx:89-92)")


def api_spmma_step(A, Apruned, B, C, blob, d_valid, m, n, k, batch):
    """One call of sparsifyme::spmma() as device work (reference spmma.hxx:82-113): TILE prune (A -> Apruned, the bytes of
    an in-place prune without destroying the bench's operand), check, compress, multiply."""
    prune24_compress24(A, Apruned, m, k, k, batch, m * k, blob, d_valid, PRUNE_TILE)
    spmma(blob, B, C, m, n, k, batch, 0)


def prune24_spmma(A_in, A_out, B, C, m, n, k, lda=None, batch=1, strideA=None, strideB=0, strideC=None, alg=PRUNE_TILE, d_valid=None,
                  alpha=1.0, beta=0.0, check=True):
    """sparsifyme::spmma()'s whole sequence in one kernel (spmma.hxx:82-113): prune A_in -> A_out (may be A_in), flag, multiply.
    Returns the status (check=False: SM_STATUS_NOT_SUPPORTED is returned, not raised, so that callers can fall back)."""
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    fn = getattr(lib(), "sm_prune24_spmma_" + _sfx(A_in))
    rc = fn(_dev(A_in), _dev(A_out), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, alg,
            _dev(d_valid) if d_valid is not None else None, alpha, beta, _stream())
    if check or rc not in (0, STATUS_NOT_SUPPORTED):
        _check(rc, "sm_prune24_spmma")
    return rc


def api_spmma_step_fused(A, Apruned, B, C, blob, d_valid, m, n, k, batch):
    """api_spmma_step without a blob wherever sm_prune24_spmma_* takes the shape (one kernel for n <= 128, k % 64 == 0, m % 4 == 0; since round 6
    the prune + flag pass followed by the exact fused kernel on the pruned operand elsewhere), the blob pair where it does not."""
    if prune24_spmma(A, Apruned, B, C, m, n, k, batch=batch, d_valid=d_valid, check=False) == STATUS_NOT_SUPPORTED:
        api_spmma_step(A, Apruned, B, C, blob, d_valid, m, n, k, batch)


def decompress24(blob, m, k, ld, batch, strideA, A):
    fn = getattr(lib(), "sm_decompress24_" + _sfx(A))
    _check(fn(_dev(blob), m, k, ld, batch, strideA, _dev(A), _stream()), "sm_decompress24")


# ---- which kernel a prune / check / compress / decompress / one-pass call runs (include/sparsifyme.h: sm_*_form) ----
# names of SM_PRUNE24_FORM_*, SM_COMPRESS24_FORM_*, SM_DECOMPRESS24_FORM_* and SM_PRUNE24_COMPRESS24_FORM_*, in order
PRUNE24_FORMS = ("invalid", "empty", "strip_scalar", "strip_vec", "strip_flat_scalar", "strip_flat_vec", "tile2", "span", "element_scalar",
                 "element_vec")
COMPRESS24_FORMS = ("invalid", "empty", "flat", "rowspan", "general_scalar", "general_vec")
DECOMPRESS24_FORMS = ("invalid", "empty", "scalar", "vec")
PRUNE24_COMPRESS24_FORMS = ("invalid", "empty", "not_supported", "fallback_tall_span", "fallback_tall", "fallback_per_batch", "onepass_tile",
                            "onepass_tile_noblob", "onepass_strip")


def _addr(x):
    """An operand of a form query as an address: None, an int (a dummy address: the queries never dereference) or a tensor."""
    if x is None or isinstance(x, int):
        return x
    return x.data_ptr()


def prune24_form(A_in, A_out, m, k, ld, elt_bytes, alg=PRUNE_STRIP, with_span_rows=False):
    """The name (PRUNE24_FORMS) of the kernel class prune24 runs for this call -- sm_prune24_form; operands: tensors or addresses.
    with_span_rows: (name, rows per span of the span form or 0)."""
    form, rows = _c_i(-1), ctypes.c_uint(0)
    _check(lib().sm_prune24_form(_addr(A_in), _addr(A_out), m, k, ld, elt_bytes, alg, ctypes.byref(form), ctypes.byref(rows)), "sm_prune24_form")
    return (PRUNE24_FORMS[form.value], rows.value) if with_span_rows else PRUNE24_FORMS[form.value]


def prune24_check_form(A, d_valid, m, k, ld, elt_bytes):
    form = _c_i(-1)
    _check(lib().sm_prune24_check_form(_addr(A), _addr(d_valid), m, k, ld, elt_bytes, ctypes.byref(form)), "sm_prune24_check_form")
    return PRUNE24_FORMS[form.value]


def compress24_form(A, blob, m, k, ld, batch, strideA, elt_bytes):
    form = _c_i(-1)
    _check(lib().sm_compress24_form(_addr(A), _addr(blob), m, k, ld, batch, strideA, elt_bytes, ctypes.byref(form)), "sm_compress24_form")
    return COMPRESS24_FORMS[form.value]


def decompress24_form(blob, A, m, k, ld, batch, strideA, elt_bytes):
    form = _c_i(-1)
    _check(lib().sm_decompress24_form(_addr(blob), _addr(A), m, k, ld, batch, strideA, elt_bytes, ctypes.byref(form)), "sm_decompress24_form")
    return DECOMPRESS24_FORMS[form.value]


def prune24_compress24_form(A_in, A_out, m, k, ld, batch, strideA, blob, elt_bytes, alg=PRUNE_TILE, cus=0):
    """(name in PRUNE24_COMPRESS24_FORMS, plan) of a prune24_compress24 call -- sm_prune24_compress24_form.  plan: dict(flat, lpr_log2, nj,
    grid, capped) for the one-pass kernel, dict(matrices) for the three-launch fallback, {} otherwise.  cus = 0: this device's CU count."""
    form, plan = _c_i(-1), (ctypes.c_uint * 6)()
    _check(lib().sm_prune24_compress24_form(_addr(A_in), _addr(A_out), m, k, ld, batch, strideA, _addr(blob), elt_bytes, alg, cus,
                                            ctypes.byref(form), plan), "sm_prune24_compress24_form")
    name = PRUNE24_COMPRESS24_FORMS[form.value]
    if name.startswith("onepass"):
        return name, dict(flat=bool(plan[0]), lpr_log2=plan[1], nj=plan[2], grid=plan[3], capped=bool(plan[4]))
    if name.startswith("fallback"):
        return name, dict(matrices=plan[5])
    return name, {}


BIAS_COL, BIAS_ROW = 0, 1
ACT_NONE, ACT_RELU, ACT_CLIPPED_RELU, ACT_LEAKY_RELU, ACT_HARDSWISH = 0, 1, 2, 3, 4
_BIAS_DIMS = {"col": BIAS_COL, "row": BIAS_ROW}
_ACTS = {"none": ACT_NONE, "relu": ACT_RELU, "clipped_relu": ACT_CLIPPED_RELU, "relu6": ACT_CLIPPED_RELU, "leaky_relu": ACT_LEAKY_RELU,
         "hardswish": ACT_HARDSWISH}


class EpilogueStruct(ctypes.Structure):
    """sm_epilogue_t (include/sparsifyme.h)"""
    _fields_ = [("bias", _c_ptr), ("bias_dim", _c_i), ("act", _c_i), ("act_arg", _c_f), ("R", _c_ptr), ("strideR", _c_size)]


class Epilogue:
    """What spmma(..., epilogue=) / spmma_fused(..., epilogue=) apply in the matmul's store:
    D = act(alpha * A.B + beta * residual + bias), fp32 until the one final rounding (sm_epilogue_t, include/sparsifyme.h).
    bias: float32 device vector (bias_dim "col": n entries, "row": m entries) or None; act: "none", "relu", "clipped_relu"
    ("relu6": clipped with act_arg 6), "leaky_relu", "hardswish", or an ACT_* number; residual: a device tensor of D's dtype with D's
    layout (None: D itself when beta != 0, what beta means without an epilogue); stride_residual: its batch stride (default m * n)."""

    def __init__(self, bias=None, bias_dim="col", act="none", act_arg=0.0, residual=None, stride_residual=None):
        if bias is not None and bias.dtype != _t().float32:
            raise SparsifymeError(f"Epilogue: bias is float32, not {bias.dtype}")
        if isinstance(bias_dim, str):
            if bias_dim not in _BIAS_DIMS:
                raise SparsifymeError(f"Epilogue: bias_dim is 'col' or 'row', not {bias_dim!r}")
            bias_dim = _BIAS_DIMS[bias_dim]
        if isinstance(act, str):
            if act not in _ACTS:
                raise SparsifymeError(f"Epilogue: unknown activation {act!r} (one of {sorted(_ACTS)})")
            if act == "relu6" and not act_arg:
                act_arg = 6.0
            act = _ACTS[act]
        self.bias, self.bias_dim, self.act, self.act_arg = bias, int(bias_dim), int(act), float(act_arg)
        self.residual, self.stride_residual = residual, stride_residual

    def struct_for(self, D, strideD, beta):
        """The C struct for a call that writes D (dtype checks first, then the pointers)."""
        if self.residual is not None and self.residual.dtype != D.dtype:
            raise SparsifymeError(f"Epilogue: residual is {self.residual.dtype}, the output is {D.dtype}")
        st = EpilogueStruct()
        st.bias = _dev(self.bias) if self.bias is not None else None
        st.bias_dim, st.act, st.act_arg = self.bias_dim, self.act, self.act_arg
        if self.residual is not None:
            st.R = _dev(self.residual)
            st.strideR = strideD if self.stride_residual is None else self.stride_residual
        elif beta != 0.0:
            st.R, st.strideR = _dev(D), strideD
        else:
            st.R, st.strideR = None, 0
        return st


def spmma(blob, B, C, m, n, k, batch=1, strideB=0, strideC=None, alpha=1.0, beta=0.0, epilogue=None):
    """The matmul step of sparsifyme::spmma (spmma.hxx:112-113) on a compressed blob; epilogue: an Epilogue (sm_spmma_*_ex)."""
    if strideC is None:
        strideC = m * n
    if epilogue is not None:
        st = epilogue.struct_for(C, strideC, float(beta))
        fn = getattr(lib(), "sm_spmma_%s_ex" % _sfx(B))
        _check(fn(_dev(blob), _dev(B), _dev(C), m, n, k, batch, strideB, strideC, float(alpha), float(beta), ctypes.addressof(st), _stream()),
               "sm_spmma_ex")
        return
    fn = getattr(lib(), "sm_spmma_" + _sfx(B))
    _check(fn(_dev(blob), _dev(B), _dev(C), m, n, k, batch, strideB, strideC, float(alpha), float(beta), _stream()),
           "sm_spmma")


def _opt(t):
    """the device address of an optional tensor"""
    return _dev(t) if t is not None else None


def _linear24_16(X, Y, what):
    """what the eight linear24* wrappers share: the 16-bit layers' dtype check ..."""
    torch = _t()
    if X.dtype not in (torch.float16, torch.bfloat16) or Y.dtype != X.dtype:
        raise SparsifymeError(f"{what}: X and Y are both float16 or both bfloat16, not {X.dtype} and {Y.dtype}")


def _linear24_8(X, Y, w_dtype, w_scale, x_scale, what):
    """... the fp8 layers' (fmt_w, fmt_x, out_type) from the dtypes and their two optional scale addresses ..."""
    fx = fp8_format(X.dtype)
    fw = fx if w_dtype is None else fp8_format(w_dtype)
    ot = _fp8_out_type(Y)
    for name, v in (("w_scale", w_scale), ("x_scale", x_scale)):
        if v is not None and v.dtype != _t().float32:
            raise SparsifymeError(f"{what}: {name} is float32, not {v.dtype}")
    return fw, fx, ot, _opt(w_scale), _opt(x_scale)


def _linear24_ld(ldx, ldy, in_features, width):
    """... the leading dimensions' defaults (width: out_features, or hidden) ..."""
    return in_features if ldx is None else ldx, width if ldy is None else ldy


def _linear24_epilogue(epilogue, Y, beta):
    """... and (struct, its address) of an optional Epilogue: the caller holds the struct until the call has returned."""
    if epilogue is None:
        return None, None
    st = epilogue.struct_for(Y, 0, float(beta))
    return st, ctypes.addressof(st)


def linear24(blob, X, Y, tokens, out_features, in_features, ldx=None, ldy=None, alpha=1.0, beta=0.0, epilogue=None):
    """Y[tokens][out] = act(alpha * X[tokens][in] . W^T + beta * R + bias) with W[out][in] the 2:4 blob of
    compress24(W, m=out_features, k=in_features) (sm_linear24_*): token-major in and out, one launch.  epilogue: an Epilogue read in
    Y's coordinates (bias_dim "col": one value per out feature, "row": one per token; residual of Y's shape and ldy)."""
    _linear24_16(X, Y, "linear24")
    ldx, ldy = _linear24_ld(ldx, ldy, in_features, out_features)
    st, ep = _linear24_epilogue(epilogue, Y, beta)
    fn = getattr(lib(), "sm_linear24_" + _sfx(X))
    _check(fn(_dev(blob), _dev(X), _dev(Y), tokens, out_features, in_features, ldx, ldy, float(alpha), float(beta), ep,
              _stream()), "sm_linear24")


# include/sparsifyme.h: SM_LINEAR24_FORM_* (index = value)
LINEAR24_FORMS = ("not_taken", "empty", "decode", "tile64", "tile128x64", "tile128")


def linear24_fp8(blob, X, Y, tokens, out_features, in_features, w_dtype=None, ldx=None, ldy=None, alpha=1.0, beta=0.0, w_scale=None,
                 x_scale=None, epilogue=None):
    """Y[tokens][out] = act((alpha * w_scale[o]) * x_scale[t] * (X[tokens][in] . W^T) + beta * R + bias) with W[out][in] the fp8 2:4 blob
    of compress24_fp8 / quantize_compress24_fp8 and X fp8 tokens (sm_linear24_fp8): token-major in and out, one launch.  The formats
    come from the dtypes (w_dtype: W's fp8 dtype, the blob does not carry it; None = X's), the output type from Y's (float32 / float16 /
    bfloat16).  w_scale / x_scale: float32 device vectors or None.  epilogue: an Epilogue read in Y's coordinates, as linear24 reads it."""
    fw, fx, ot, ws, xs = _linear24_8(X, Y, w_dtype, w_scale, x_scale, "linear24_fp8")
    ldx, ldy = _linear24_ld(ldx, ldy, in_features, out_features)
    st, ep = _linear24_epilogue(epilogue, Y, beta)
    _check(lib().sm_linear24_fp8(_dev(blob), _dev(X), _dev(Y), tokens, out_features, in_features, ldx, ldy, fw, fx, ot, float(alpha), float(beta),
                                 ws, xs, ep, _stream()), "sm_linear24_fp8")


def linear24_fp8_form(tokens, out_features, in_features, cus=0):
    """The name (LINEAR24_FORMS) of the form linear24_fp8 runs for this shape -- sm_linear24_fp8_form, the rule the entry point itself
    switches on.  cus=0: this device's compute units; another value: host-only."""
    form = _c_i(-1)
    _check(lib().sm_linear24_fp8_form(tokens, out_features, in_features, cus, ctypes.byref(form)), "sm_linear24_fp8_form")
    return LINEAR24_FORMS[form.value]


# include/sparsifyme.h: SM_GLU_ACT_*
GLU_ACTS = {"none": 0, "relu": 1, "silu": 2}


def _glu_act(act, what):
    if act not in GLU_ACTS:
        raise SparsifymeError(f"{what}: act is one of {sorted(GLU_ACTS)}, not {act!r}")
    return GLU_ACTS[act]


def _glu_bias(bias, what):
    if bias is not None and bias.dtype != _t().float32:
        raise SparsifymeError(f"{what}: bias is float32, not {bias.dtype}")
    return _opt(bias)


def linear24_glu(blob, X, Y, tokens, hidden, in_features, act="silu", bias=None, ldx=None, ldy=None):
    """Y[tokens][hidden] = act(g) * u, g = X . W[:hidden]^T + bias[:hidden], u = X . W[hidden:]^T + bias[hidden:], with W[2 hidden][in]
    the 2:4 blob of compress24(W, m=2 * hidden, k=in_features): a fused gate/up projection and its gate in one launch
    (sm_linear24_glu_*).  act: "silu" (SwiGLU), "relu" (ReGLU) or "none" (bilinear); bias: 2 * hidden float32 values or None."""
    _linear24_16(X, Y, "linear24_glu")
    a, b = _glu_act(act, "linear24_glu"), _glu_bias(bias, "linear24_glu")
    ldx, ldy = _linear24_ld(ldx, ldy, in_features, hidden)
    fn = getattr(lib(), "sm_linear24_glu_" + _sfx(X))
    _check(fn(_dev(blob), _dev(X), _dev(Y), tokens, hidden, in_features, ldx, ldy, a, b, _stream()), "sm_linear24_glu")


def linear24_glu_fp8(blob, X, Y, tokens, hidden, in_features, act="silu", w_dtype=None, w_scale=None, x_scale=None, bias=None, ldx=None,
                     ldy=None):
    """linear24_glu on fp8 operands (sm_linear24_glu_fp8): g and u are (w_scale[row] * x_scale[t]) * acc + bias[row] with row = h and
    hidden + h.  The formats come from the dtypes as in linear24_fp8; w_scale: 2 * hidden float32 values, x_scale: tokens, or None."""
    fw, fx, ot, ws, xs = _linear24_8(X, Y, w_dtype, w_scale, x_scale, "linear24_glu_fp8")
    a, b = _glu_act(act, "linear24_glu_fp8"), _glu_bias(bias, "linear24_glu_fp8")
    ldx, ldy = _linear24_ld(ldx, ldy, in_features, hidden)
    _check(lib().sm_linear24_glu_fp8(_dev(blob), _dev(X), _dev(Y), tokens, hidden, in_features, ldx, ldy, fw, fx, ot, a,
                                     ws, xs, b, _stream()), "sm_linear24_glu_fp8")


def linear24_glu_form(tokens, hidden, in_features, cus=0):
    """The name (LINEAR24_FORMS) of the form the gated layers run for this shape -- sm_linear24_glu_form, by definition the plain rule
    on 2 * hidden rows.  linear24_glu_fp8 asks with this device's compute units (cus=0), linear24_glu with cus=256."""
    form = _c_i(-1)
    _check(lib().sm_linear24_glu_form(tokens, hidden, in_features, cus, ctypes.byref(form)), "sm_linear24_glu_form")
    return LINEAR24_FORMS[form.value]


# include/sparsifyme.h: SM_LINEAR24_MAX_GROUPS
LINEAR24_MAX_GROUPS = 1024


def _group_offsets(group_offsets, what):
    if group_offsets.dtype != _t().int32:
        raise SparsifymeError(f"{what}: group_offsets is int32, not {group_offsets.dtype}")
    return _dev(group_offsets)


def _x_index(x_index, x_rows, what):
    """(x_index, x_rows) of the gathered forms as ctypes arguments, [] without x_index; x_rows=None is not guessed (X's buffer may hold
    guard rows)."""
    if x_index is None:
        return []
    if x_index.dtype != _t().int32:
        raise SparsifymeError(f"{what}: x_index is int32, not {x_index.dtype}")
    if x_rows is None:
        raise SparsifymeError(f"{what}: x_rows (the rows of X) is required with x_index")
    return [_dev(x_index), x_rows]


def linear24_grouped(blob, X, Y, group_offsets, groups, tokens, out_features, in_features, ldx=None, ldy=None, alpha=1.0, beta=0.0,
                     epilogue=None, x_index=None, x_rows=None):
    """linear24 per expert in one launch (sm_linear24_grouped_*): blob is that of the stacked W[groups * out][in], the tokens of X
    and Y are sorted by expert, and group_offsets (groups + 1 int32 values on the device, never copied to the host) says where each
    expert's rows begin.  A "col" bias holds groups * out values, expert-major; a "row" bias and the residual are in Y's rows.
    x_index (tokens int32 values on the device) with x_rows: the gathered form (sm_linear24_grouped_gather_*), row t of Y reads row
    x_index[t] of X's x_rows rows; the same for the three grouped wrappers below."""
    _linear24_16(X, Y, "linear24_grouped")
    off = _group_offsets(group_offsets, "linear24_grouped")
    ldx, ldy = _linear24_ld(ldx, ldy, in_features, out_features)
    st, ep = _linear24_epilogue(epilogue, Y, beta)
    gather = _x_index(x_index, x_rows, "linear24_grouped")
    fn = getattr(lib(), "sm_linear24_grouped_" + ("gather_" if gather else "") + _sfx(X))
    _check(fn(_dev(blob), _dev(X), _dev(Y), off, *gather, groups, tokens, out_features, in_features, ldx, ldy, float(alpha), float(beta), ep,
              _stream()), "sm_linear24_grouped")


def linear24_grouped_fp8(blob, X, Y, group_offsets, groups, tokens, out_features, in_features, w_dtype=None, ldx=None, ldy=None, alpha=1.0,
                         beta=0.0, w_scale=None, x_scale=None, epilogue=None, x_index=None, x_rows=None):
    """linear24_fp8 per expert in one launch (sm_linear24_grouped_fp8); w_scale: groups * out float32 values, expert-major; x_scale:
    tokens values in Y's rows (gathered: x_rows values in X's rows)."""
    fw, fx, ot, ws, xs = _linear24_8(X, Y, w_dtype, w_scale, x_scale, "linear24_grouped_fp8")
    off = _group_offsets(group_offsets, "linear24_grouped_fp8")
    ldx, ldy = _linear24_ld(ldx, ldy, in_features, out_features)
    st, ep = _linear24_epilogue(epilogue, Y, beta)
    gather = _x_index(x_index, x_rows, "linear24_grouped_fp8")
    fn = lib().sm_linear24_grouped_gather_fp8 if gather else lib().sm_linear24_grouped_fp8
    _check(fn(_dev(blob), _dev(X), _dev(Y), off, *gather, groups, tokens, out_features, in_features, ldx, ldy, fw, fx, ot,
              float(alpha), float(beta), ws, xs, ep, _stream()), "sm_linear24_grouped_fp8")


def linear24_grouped_glu(blob, X, Y, group_offsets, groups, tokens, hidden, in_features, act="silu", bias=None, ldx=None, ldy=None,
                         x_index=None, x_rows=None):
    """linear24_glu per expert in one launch (sm_linear24_grouped_glu_*): blob is that of W[groups][2 hidden][in], each expert's gate
    rows then its up rows; bias: groups * 2 * hidden float32 values in the same order, or None."""
    _linear24_16(X, Y, "linear24_grouped_glu")
    a, b = _glu_act(act, "linear24_grouped_glu"), _glu_bias(bias, "linear24_grouped_glu")
    off = _group_offsets(group_offsets, "linear24_grouped_glu")
    ldx, ldy = _linear24_ld(ldx, ldy, in_features, hidden)
    gather = _x_index(x_index, x_rows, "linear24_grouped_glu")
    fn = getattr(lib(), "sm_linear24_grouped_glu_" + ("gather_" if gather else "") + _sfx(X))
    _check(fn(_dev(blob), _dev(X), _dev(Y), off, *gather, groups, tokens, hidden, in_features, ldx, ldy, a, b, _stream()), "sm_linear24_grouped_glu")


def linear24_grouped_glu_fp8(blob, X, Y, group_offsets, groups, tokens, hidden, in_features, act="silu", w_dtype=None, w_scale=None,
                             x_scale=None, bias=None, ldx=None, ldy=None, x_index=None, x_rows=None):
    """linear24_glu_fp8 per expert in one launch (sm_linear24_grouped_glu_fp8); w_scale and bias: groups * 2 * hidden float32 values."""
    fw, fx, ot, ws, xs = _linear24_8(X, Y, w_dtype, w_scale, x_scale, "linear24_grouped_glu_fp8")
    a, b = _glu_act(act, "linear24_grouped_glu_fp8"), _glu_bias(bias, "linear24_grouped_glu_fp8")
    off = _group_offsets(group_offsets, "linear24_grouped_glu_fp8")
    ldx, ldy = _linear24_ld(ldx, ldy, in_features, hidden)
    gather = _x_index(x_index, x_rows, "linear24_grouped_glu_fp8")
    fn = lib().sm_linear24_grouped_glu_gather_fp8 if gather else lib().sm_linear24_grouped_glu_fp8
    _check(fn(_dev(blob), _dev(X), _dev(Y), off, *gather, groups, tokens, hidden, in_features, ldx, ldy, fw, fx, ot, a,
              ws, xs, b, _stream()), "sm_linear24_grouped_glu_fp8")


def linear24_grouped_form(tokens, groups, out_features, in_features, cus=0):
    """The name (LINEAR24_FORMS) of the form the grouped layers run -- sm_linear24_grouped_form; never "decode".  The gated layers ask
    with out_features = 2 * hidden; the fp8 layers with this device's compute units (cus=0), the 16-bit layers with cus=256."""
    form = _c_i(-1)
    _check(lib().sm_linear24_grouped_form(tokens, groups, out_features, in_features, cus, ctypes.byref(form)), "sm_linear24_grouped_form")
    return LINEAR24_FORMS[form.value]


# include/sparsifyme.h: SM_MOE_ROUTE_FORM_*, SM_MOE_COMBINE_FORM_* (index = value), the SINGLE limit and the MULTI chunk
MOE_ROUTE_FORMS = ("invalid", "empty", "single", "multi")
MOE_COMBINE_FORMS = ("invalid", "empty", "scalar", "vec")
MOE_ROUTE_SINGLE_MAX_PAIRS = 4096
MOE_ROUTE_CHUNK = 4096


def moe_route_form(tokens, top_k, groups):
    """The name (MOE_ROUTE_FORMS) of the form moe_route runs -- sm_moe_route_form, the rule the entry point switches on.  Host only."""
    form = _c_i(-1)
    _check(lib().sm_moe_route_form(tokens, top_k, groups, ctypes.byref(form)), "sm_moe_route_form")
    return MOE_ROUTE_FORMS[form.value]


def moe_route_workspace_size(tokens, top_k, groups):
    """Bytes of workspace moe_route needs (0 for the single form).  Host only."""
    n = _c_size(0)
    _check(lib().sm_moe_route_workspace_size(tokens, top_k, groups, ctypes.byref(n)), "sm_moe_route_workspace_size")
    return n.value


def moe_route(expert_ids, tokens, top_k, groups, group_offsets, sorted_token, sorted_pair, pair_pos, workspace=None):
    """The router's ids (int32 [tokens * top_k]) to group_offsets [groups + 1], sorted_token / sorted_pair [P] and pair_pos [P], all int32
    on the device: a stable counting sort by expert, ids outside [0, groups) dropped (sm_moe_route).  workspace: a device tensor of at
    least moe_route_workspace_size bytes, or None where that is 0."""
    for name, v in (("expert_ids", expert_ids), ("group_offsets", group_offsets), ("sorted_token", sorted_token), ("sorted_pair", sorted_pair),
                    ("pair_pos", pair_pos)):
        if v.dtype != _t().int32:
            raise SparsifymeError(f"moe_route: {name} is int32, not {v.dtype}")
    ws = _dev(workspace) if workspace is not None else None
    nb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    _check(lib().sm_moe_route(_dev(expert_ids), tokens, top_k, groups, _dev(group_offsets), _dev(sorted_token), _dev(sorted_pair), _dev(pair_pos),
                              ws, nb, _stream()), "sm_moe_route")


def moe_combine(Yp, pair_pos, out, tokens, top_k, hidden, rows_p, weights=None, residual=None, ldp=None, ldo=None):
    """out[t] = round(residual[t] + sum_j weights[t top_k + j] * Yp[pair_pos[t top_k + j]]) in fp32, j ascending, multiply and add not
    contracted, one rounding (sm_moe_combine_*): Yp and out both float16 or both bfloat16; weights float32 or None; residual of out's
    type and ldo (out itself: in place) or None; pairs with pair_pos < 0 or >= rows_p are skipped."""
    torch = _t()
    if Yp.dtype not in (torch.float16, torch.bfloat16) or out.dtype != Yp.dtype or (residual is not None and residual.dtype != Yp.dtype):
        raise SparsifymeError(f"moe_combine: Yp, out and residual are all float16 or all bfloat16, not {Yp.dtype} and {out.dtype}")
    if pair_pos.dtype != torch.int32 or (weights is not None and weights.dtype != torch.float32):
        raise SparsifymeError("moe_combine: pair_pos is int32 and weights float32")
    ldp = hidden if ldp is None else ldp
    ldo = hidden if ldo is None else ldo
    fn = getattr(lib(), "sm_moe_combine_" + _sfx(Yp))
    _check(fn(_dev(Yp), _dev(pair_pos), _dev(weights) if weights is not None else None, _dev(residual) if residual is not None else None,
              _dev(out), tokens, top_k, hidden, rows_p, ldp, ldo, _stream()), "sm_moe_combine")


def moe_combine_form(Yp, residual, out, hidden, ldp, ldo):
    """The name (MOE_COMBINE_FORMS) of the form moe_combine runs -- sm_moe_combine_form; Yp / residual / out: tensors, addresses or None."""
    ptr = lambda v: None if v is None else ctypes.c_void_p(v if isinstance(v, int) else v.data_ptr())
    form = _c_i(-1)
    _check(lib().sm_moe_combine_form(ptr(Yp), ptr(residual), ptr(out), hidden, ldp, ldo, ctypes.byref(form)), "sm_moe_combine_form")
    return MOE_COMBINE_FORMS[form.value]


# include/sparsifyme.h: SM_MOE_GATE_FORM_* (index = value), SM_MOE_SCORE_*, SM_MOE_GATE_MAX_TOP_K
MOE_GATE_FORMS = ("invalid", "empty", "lane1", "lane2", "lane4", "lane8", "lane16")
MOE_SCORE_SOFTMAX, MOE_SCORE_SIGMOID = 0, 1
MOE_GATE_MAX_TOP_K = 32
_MOE_SCORES = {"softmax": MOE_SCORE_SOFTMAX, "sigmoid": MOE_SCORE_SIGMOID}


def moe_gate_form(tokens, experts, top_k):
    """The name (MOE_GATE_FORMS) of the form moe_gate runs -- sm_moe_gate_form, the rule the entry points switch on.  Host only."""
    form = _c_i(-1)
    _check(lib().sm_moe_gate_form(tokens, experts, top_k, ctypes.byref(form)), "sm_moe_gate_form")
    return MOE_GATE_FORMS[form.value]


def moe_gate(logits, topk_ids, topk_weights, tokens, experts, top_k, scoring="softmax", renormalize=True, scale=1.0, select_bias=None, ld=None):
    """The router's logits [tokens][experts] (row pitch ld; float16, bfloat16 or float32) to topk_ids (int32) and topk_weights (float32),
    both [tokens * top_k] in pair order: descending key, equal keys in ascending expert index; softmax or sigmoid weights in fp32,
    renormalised over the top_k or not, times scale (sm_moe_gate_*).  scoring: "softmax" / "sigmoid" or a MOE_SCORE_* value.
    select_bias: float32 [experts] added to the sigmoid scores for the selection only, or None."""
    torch = _t()
    if logits.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise SparsifymeError(f"moe_gate: logits are float16, bfloat16 or float32, not {logits.dtype}")
    if topk_ids.dtype != torch.int32 or topk_weights.dtype != torch.float32 or (select_bias is not None and select_bias.dtype != torch.float32):
        raise SparsifymeError("moe_gate: topk_ids is int32, topk_weights and select_bias float32")
    ld = experts if ld is None else ld
    fn = getattr(lib(), "sm_moe_gate_" + _sfx(logits))
    _check(fn(_dev(logits), _dev(select_bias) if select_bias is not None else None, _dev(topk_ids), _dev(topk_weights), tokens, experts, top_k, ld,
              _MOE_SCORES.get(scoring, scoring), 1 if renormalize else 0, float(scale), _stream()), "sm_moe_gate")


def spmma_fused_i8(A, B, C, m, n, k, lda=None, batch=1, strideA=None, strideB=0, strideC=None, accumulate=False, scale=None):
    """int8 prune + compress + matmul in one kernel; C int32 (scale None) or int8 requantised with `scale`."""
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    if scale is None:
        _check(lib().sm_spmma_fused_i8(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC,
                                       1 if accumulate else 0, _stream()), "sm_spmma_fused_i8")
    else:
        _check(lib().sm_spmma_fused_i8_q(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, float(scale),
                                         _stream()), "sm_spmma_fused_i8_q")


def transpose_i8(src, dst, rows, cols):
    _check(lib().sm_transpose_i8(_dev(src), _dev(dst), rows, cols, _stream()), "sm_transpose_i8")


def spmma_i8(blob, B, C, m, n, k, batch=1, strideB=0, strideC=None, accumulate=False):
    """int8 2:4 product: B [n][k] int8 (k-contiguous per output column), C int32."""
    strideC = m * n if strideC is None else strideC
    if C.dtype == _t().int8:
        raise SparsifymeError("spmma_i8 writes int32; use spmma_i8_q for a requantised int8 result")
    _check(lib().sm_spmma_i8(_dev(blob), _dev(B), _dev(C), m, n, k, batch, strideB, strideC, 1 if accumulate else 0, _stream()),
           "sm_spmma_i8")


def spmma_i8_q(blob, B, C, m, n, k, scale, batch=1, strideB=0, strideC=None):
    """int8 2:4 product requantised to int8: C = saturate(rne(scale * acc))."""
    strideC = m * n if strideC is None else strideC
    _check(lib().sm_spmma_i8_q(_dev(blob), _dev(B), _dev(C), m, n, k, batch, strideB, strideC, float(scale), _stream()),
           "sm_spmma_i8_q")


# ---- OCP fp8 (include/sparsifyme.h: SM_FP8_*, SM_OUT_*) ----------------------------------------
FP8_E4M3, FP8_E5M2 = 0, 1
OUT_F32, OUT_F16, OUT_BF16 = 0, 1, 2


def fp8_format(dtype):
    """SM_FP8_* of a torch dtype: float8_e4m3fn or float8_e5m2 (the OCP encodings; the fnuz ones are refused)."""
    torch = _t()
    fmts = {torch.float8_e4m3fn: FP8_E4M3, torch.float8_e5m2: FP8_E5M2}
    if dtype not in fmts:
        raise SparsifymeError(f"expected torch.float8_e4m3fn or torch.float8_e5m2, not {dtype}")
    return fmts[dtype]


def _fp8_out_type(C):
    torch = _t()
    outs = {torch.float32: OUT_F32, torch.float16: OUT_F16, torch.bfloat16: OUT_BF16}
    if C.dtype not in outs:
        raise SparsifymeError(f"fp8 spmma writes float32, float16 or bfloat16, not {C.dtype}")
    return outs[C.dtype]


def prune24_fp8(A_in, A_out, m, k, ld, alg=PRUNE_STRIP):
    """2:4 prune of an fp8 matrix: the fp16 rule on its exact fp16 image, mapped back (dropped bytes become 0x00)."""
    fmt = fp8_format(A_in.dtype)
    if A_out.dtype != A_in.dtype:
        raise SparsifymeError("prune24_fp8: A_in and A_out differ in dtype")
    _check(lib().sm_prune24_fp8(_dev(A_in), _dev(A_out), m, k, ld, alg, fmt, _stream()), "sm_prune24_fp8")


def prune24_check_fp8(A, m, k, ld, d_valid):
    fp8_format(A.dtype)
    _check(lib().sm_prune24_check_fp8(_dev(A), m, k, ld, _dev(d_valid), _stream()), "sm_prune24_check_fp8")


def compress24_fp8(A, m, k, ld, batch, strideA, blob):
    """blob: compress24_size(m, k, 1, batch) bytes."""
    _check(lib().sm_compress24_fp8(_dev(A), m, k, ld, batch, strideA, _dev(blob), fp8_format(A.dtype), _stream()), "sm_compress24_fp8")


def decompress24_fp8(blob, m, k, ld, batch, strideA, A):
    fp8_format(A.dtype)
    _check(lib().sm_decompress24_fp8(_dev(blob), m, k, ld, batch, strideA, _dev(A), _stream()), "sm_decompress24_fp8")


def spmma_fp8(blob, B, C, m, n, k, batch=1, strideB=0, strideC=None, alpha=1.0, beta=0.0, row_scale=None, a_dtype=None):
    """fp8 2:4 product: C = alpha * row_scale[i] * (A_2:4 . B) + beta * C.  B [n][k] fp8 (k-contiguous per output column);
    C float32 / float16 / bfloat16; row_scale None or m float32 on the device.  a_dtype: A's fp8 dtype (the blob does not
    carry it); None = B's."""
    strideC = m * n if strideC is None else strideC
    fa = fp8_format(B.dtype if a_dtype is None else a_dtype)
    ot = _fp8_out_type(C)
    rs = _dev(row_scale) if row_scale is not None else None
    _check(lib().sm_spmma_fp8(_dev(blob), _dev(B), _dev(C), m, n, k, batch, strideB, strideC, fa, fp8_format(B.dtype), ot, float(alpha),
                              float(beta), rs, _stream()), "sm_spmma_fp8")


def spmma_fused_fp8(A, B, C, m, n, k, lda=None, batch=1, strideA=None, strideB=0, strideC=None, alpha=1.0, beta=0.0, row_scale=None):
    """prune (STRIP) + compress + spmma_fp8 in one kernel from the dense fp8 A; the same C bit for bit."""
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    ot = _fp8_out_type(C)
    rs = _dev(row_scale) if row_scale is not None else None
    _check(lib().sm_spmma_fused_fp8(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, fp8_format(A.dtype),
                                    fp8_format(B.dtype), ot, float(alpha), float(beta), rs, _stream()), "sm_spmma_fused_fp8")


def gemm_rowmajor_fp8(A, B, C, m, n, k, lda=None, batch=1, strideA=None, strideB=0, strideC=None, alpha=1.0, beta=0.0, row_scale=None):
    """dense fp8 GEMM: C = alpha * row_scale[i] * (A . B) + beta * C.  A row-major m x k fp8, B [n][k] fp8 (formats from their
    dtypes), C float32 / float16 / bfloat16 (the output type from its dtype); the dense denominator of spmma_fp8."""
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    fa, fb = fp8_format(A.dtype), fp8_format(B.dtype)
    ot = _fp8_out_type(C)
    rs = _dev(row_scale) if row_scale is not None else None
    _check(lib().sm_gemm_rowmajor_fp8(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, fa, fb, ot, float(alpha),
                                      float(beta), rs, _stream()), "sm_gemm_rowmajor_fp8")


def _quant_src_sfx(A, what):
    torch = _t()
    if A.dtype not in (torch.float16, torch.bfloat16):
        raise SparsifymeError(f"{what}: the source is float16 or bfloat16, not {A.dtype}")
    return _sfx(A)


def _quant_row_scale(row_scale, what):
    if row_scale.dtype != _t().float32:
        raise SparsifymeError(f"{what}: row_scale is float32, not {row_scale.dtype}")
    return _dev(row_scale)


def quantize_rows_fp8(A, Q, row_scale, rows, k, lda=None, ldq=None):
    """Per-row quantisation of a float16 / bfloat16 A (rows x k) to fp8 (the format of Q's dtype): Q rows x k bytes and
    row_scale[rows] = amax / FMAX, what spmma_fp8 / gemm_rowmajor_fp8 take as row_scale."""
    sfx = _quant_src_sfx(A, "quantize_rows_fp8")
    fmt = fp8_format(Q.dtype)
    rs = _quant_row_scale(row_scale, "quantize_rows_fp8")
    fn = getattr(lib(), "sm_quantize_rows_fp8_" + sfx)
    _check(fn(_dev(A), rows, k, k if lda is None else lda, _dev(Q), k if ldq is None else ldq, rs, fmt, _stream()), "sm_quantize_rows_fp8")


# include/sparsifyme.h: SM_RMSNORM_FORM_* (index = value), SM_RMSNORM_LANES_MAX_HIDDEN, SM_RMSNORM_MAX_HIDDEN
RMSNORM_FORMS = ("invalid", "empty", "lanes", "block")
RMSNORM_LANES_MAX_HIDDEN = 512
RMSNORM_MAX_HIDDEN = 16384


def rmsnorm_form(hidden):
    """The name (RMSNORM_FORMS) of the form rmsnorm runs -- sm_rmsnorm_form, the rule the entry points switch on.  Host only."""
    form = _c_i(-1)
    _check(lib().sm_rmsnorm_form(hidden, ctypes.byref(form)), "sm_rmsnorm_form")
    return RMSNORM_FORMS[form.value]


def _rows2d(t, what, name):
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise SparsifymeError(f"{what}: {name} is [tokens][hidden] with contiguous rows (any row pitch)")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def rmsnorm(h, delta=None, gamma=None, eps=1e-6, out=None, res_out=None, fp8=None):
    """Residual add + RMSNorm in one launch (sm_rmsnorm_*): s = h + delta rounded to h's dtype (float16 / bfloat16), written to res_out
    (None: not written; h itself: the in-place update); n = s * (1 / sqrt(mean(s^2) + eps)) * gamma, fp32 to the operation, rounded once.
    h, delta, res_out, out: [tokens][hidden] with contiguous rows, any row pitch; gamma: [hidden] in h's dtype, or None (= 1).
    fp8: None -- returns n (in `out`, allocated when None); an fp8 dtype or a pair (Q, row_scale) -- also quantises n per row by the
    rule of quantize_rows_fp8 and returns (out or None, Q, row_scale): n itself is written only when `out` is given."""
    torch = _t()
    sfx = _quant_src_sfx(h, "rmsnorm")
    tokens, hidden = h.shape if h.dim() == 2 else (0, 0)
    ldh = _rows2d(h, "rmsnorm", "h")
    for name, t in (("delta", delta), ("out", out), ("res_out", res_out)):
        if t is not None and (t.dtype != h.dtype or tuple(t.shape) != (tokens, hidden)):
            raise SparsifymeError(f"rmsnorm: {name} has h's dtype and shape")
    if gamma is not None and (gamma.dtype != h.dtype or tuple(gamma.shape) != (hidden,) or not gamma.is_contiguous()):
        raise SparsifymeError("rmsnorm: gamma is a contiguous [hidden] tensor of h's dtype")
    if res_out is not None and _rows2d(res_out, "rmsnorm", "res_out") != ldh:
        raise SparsifymeError("rmsnorm: res_out has h's row pitch")
    Q = rs = None
    if fp8 is not None:
        if isinstance(fp8, torch.dtype):
            fp8_format(fp8)
            Q = torch.empty((tokens, hidden), dtype=fp8, device=h.device)
            rs = torch.empty(tokens, dtype=torch.float32, device=h.device)
        else:
            Q, rs = fp8
        if tuple(Q.shape) != (tokens, hidden) or tuple(rs.shape) != (tokens,) or not rs.is_contiguous():
            raise SparsifymeError("rmsnorm: Q is [tokens][hidden] fp8, row_scale a contiguous float32 [tokens]")
    elif out is None:
        out = torch.empty((tokens, hidden), dtype=h.dtype, device=h.device)
    ptr = lambda t: _dev(t) if t is not None else None
    fn = getattr(lib(), "sm_rmsnorm_" + sfx)
    _check(fn(_dev(h), ptr(delta), ptr(gamma), ptr(res_out), ptr(out), ptr(Q), _quant_row_scale(rs, "rmsnorm") if rs is not None else None, tokens, hidden,
              ldh, _rows2d(delta, "rmsnorm", "delta") if delta is not None else 0, _rows2d(out, "rmsnorm", "out") if out is not None else 0,
              _rows2d(Q, "rmsnorm", "Q") if Q is not None else 0, float(eps), fp8_format(Q.dtype) if Q is not None else 0, _stream()), "sm_rmsnorm")
    return out if fp8 is None else (out, Q, rs)


# include/sparsifyme.h: SM_ATTN_DECODE_FORM_* (index = value), SM_ATTN_DECODE_CHUNK and the limits
ATTN_DECODE_FORMS = ("invalid", "empty", "direct", "split")
ATTN_DECODE_CHUNK = 256
ATTN_DECODE_HEAD_DIMS = (64, 128)
ATTN_DECODE_PAGE_SIZES = (16, 32, 64, 128)
ATTN_DECODE_MAX_GROUP = 16
ATTN_DECODE_MAX_CONTEXT = 2 ** 31 - 1


def _pitch(t, d, least):
    """the stride of dimension d, or -- one entry, its stride says nothing -- at least the extent"""
    return t.stride(d) if t.shape[d] > 1 else max(t.stride(d), least)


def _heads3(what, name, t, dtype, shape):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or (shape[2] > 1 and t.stride(2) != 1) or (shape[1] > 1 and t.stride(1) != shape[2]):
        raise SparsifymeError(f"{what}: {name} is [rows][heads][head_dim] = {list(shape)} of one dtype with contiguous heads (any row pitch)")


def _paged_cache(what, k_cache, v_cache, block_table, dtype, kv_heads, head_dim):
    """The paged KV cache as attn_decode and rope_append take it (csrc/paged_kv.h), checked; returns (num_pages, page_size, max_pages, seqs,
    ldkv, page_stride, ldbt)."""
    if k_cache.dim() != 4 or tuple(v_cache.shape) != tuple(k_cache.shape) or k_cache.dtype != dtype or v_cache.dtype != dtype or \
            tuple(k_cache.shape[2:]) != (kv_heads, head_dim) or v_cache.stride() != k_cache.stride():
        raise SparsifymeError(f"{what}: the caches are [num_pages][page_size][kv_heads][head_dim] of q's dtype, one shape and the same strides")
    if (head_dim > 1 and k_cache.stride(3) != 1) or (kv_heads > 1 and k_cache.stride(2) != head_dim):
        raise SparsifymeError(f"{what}: a cache token is [kv_heads][head_dim], contiguous")
    if block_table.dim() != 2 or block_table.dtype != _t().int32 or (block_table.shape[1] > 1 and block_table.stride(1) != 1):
        raise SparsifymeError(f"{what}: block_table is int32 [seqs][max_pages] with contiguous rows")
    num_pages, page_size = k_cache.shape[:2]
    seqs, max_pages = block_table.shape
    ldkv = _pitch(k_cache, 1, kv_heads * head_dim)
    return num_pages, page_size, max_pages, seqs, ldkv, _pitch(k_cache, 0, page_size * ldkv), _pitch(block_table, 0, max_pages)


def attn_decode_form(seqs, q_heads, kv_heads, head_dim, page_size, max_pages):
    """The name (ATTN_DECODE_FORMS) of the form attn_decode runs -- sm_attn_decode_form, the rule the entry points switch on.  Host only."""
    form = _c_i(-1)
    _check(lib().sm_attn_decode_form(seqs, q_heads, kv_heads, head_dim, page_size, max_pages, ctypes.byref(form)), "sm_attn_decode_form")
    return ATTN_DECODE_FORMS[form.value]


def attn_decode_workspace_size(seqs, q_heads, head_dim, page_size, max_pages):
    """Bytes of workspace attn_decode needs (0 in the direct form) -- sm_attn_decode_workspace_size.  Host only."""
    out = ctypes.c_size_t(0)
    _check(lib().sm_attn_decode_workspace_size(seqs, q_heads, head_dim, page_size, max_pages, ctypes.byref(out)), "sm_attn_decode_workspace_size")
    return out.value


def attn_decode(q, k_cache, v_cache, block_table, seq_lens, scale=None, out=None, lse=None, workspace=None):
    """Single-query attention over a paged KV cache (sm_attn_decode_*).  q: [seqs][q_heads][head_dim] float16 / bfloat16 with contiguous
    heads (any row pitch: a column slice of a fused QKV output); k_cache, v_cache: [num_pages][page_size][kv_heads][head_dim] of q's dtype
    with contiguous heads (any token and page pitch); block_table: int32 [seqs][max_pages] (any row pitch), seq_lens: int32 [seqs], both on
    the device.  scale: head_dim ** -0.5 when None.  out: [seqs][q_heads][head_dim] (allocated when None); lse: a contiguous float32
    [seqs][q_heads], or None; workspace: a uint8 tensor of attn_decode_workspace_size bytes (allocated when None and the form is split).
    Returns out."""
    torch = _t()
    what = "attn_decode"
    sfx = _quant_src_sfx(q, what)
    if q.dim() != 3 or seq_lens.dim() != 1:
        raise SparsifymeError(f"{what}: q is [seqs][q_heads][head_dim], seq_lens [seqs]")
    seqs, q_heads, head_dim = q.shape
    kv_heads = k_cache.shape[2] if k_cache.dim() == 4 else 0
    num_pages, page_size, max_pages, table_seqs, ldkv, page_stride, ldbt = _paged_cache(what, k_cache, v_cache, block_table, q.dtype, kv_heads, head_dim)
    if table_seqs != seqs or seq_lens.dtype != torch.int32 or seq_lens.shape[0] != seqs or not seq_lens.is_contiguous():
        raise SparsifymeError(f"{what}: block_table is [seqs][max_pages], seq_lens a contiguous int32 [seqs]")
    if out is None:
        out = torch.empty((seqs, q_heads, head_dim), dtype=q.dtype, device=q.device)
    for name, t in (("q", q), ("out", out)):
        _heads3(what, name, t, q.dtype, (seqs, q_heads, head_dim))
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != (seqs, q_heads) or not lse.is_contiguous()):
        raise SparsifymeError(f"{what}: lse is a contiguous float32 [seqs][q_heads]")
    ldq, ldo = _pitch(q, 0, q_heads * head_dim), _pitch(out, 0, q_heads * head_dim)
    need = attn_decode_workspace_size(seqs, q_heads, head_dim, page_size, max_pages)
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
    ws_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    fn = getattr(lib(), "sm_attn_decode_" + sfx)
    _check(fn(_dev(q), _dev(k_cache), _dev(v_cache), _dev(block_table), _dev(seq_lens), _dev(out), _dev(lse) if lse is not None else None,
              _dev(workspace) if workspace is not None else None, ws_bytes, seqs, q_heads, kv_heads, head_dim, num_pages, page_size, max_pages,
              ldq, ldkv, page_stride, ldbt, ldo, float(head_dim ** -0.5 if scale is None else scale), _stream()), "sm_attn_decode")
    return out


# include/sparsifyme.h: SM_ROPE_APPEND_FORM_* (index = value), SM_ROPE_*, SM_ROPE_APPEND_* limits and the BLOCK / WAVE threshold
ROPE_APPEND_FORMS = ("invalid", "empty", "block", "wave")
ROPE_NEOX, ROPE_INTERLEAVED = 0, 1
ROPE_APPEND_MAX_HEAD_DIM = 256
ROPE_APPEND_ROT_DIM_MULTIPLE = 16
ROPE_APPEND_BLOCK_MAX_TOKENS = 32768
_ROPE_STYLES = {"neox": ROPE_NEOX, "interleaved": ROPE_INTERLEAVED, ROPE_NEOX: ROPE_NEOX, ROPE_INTERLEAVED: ROPE_INTERLEAVED}


def rope_append_form(tokens, q_heads, kv_heads, head_dim, rot_dim):
    """The name (ROPE_APPEND_FORMS) of the form rope_append runs -- sm_rope_append_form, the rule the entry points switch on.  Host only."""
    form = _c_i(-1)
    _check(lib().sm_rope_append_form(tokens, q_heads, kv_heads, head_dim, rot_dim, ctypes.byref(form)), "sm_rope_append_form")
    return ROPE_APPEND_FORMS[form.value]


def rope_table(max_pos, rot_dim, base=10000.0, device=None):
    """The plain RoPE table rope_append reads: float32 [max_pos][rot_dim], row p = cos(p * theta_j) for j < rot_dim / 2, then sin(p * theta_j),
    theta_j = base ** (-2 j / rot_dim); evaluated in float64 on the host and rounded once to float32.  A set-up op, once per model: a scaled
    (linear, NTK, YaRN, llama-3) table is the caller's to build in the same layout."""
    import numpy as np
    torch = _t()
    if rot_dim % 2 != 0 or rot_dim < 0 or max_pos < 0:
        raise SparsifymeError("rope_table: rot_dim is even, max_pos and rot_dim are not negative")
    half = rot_dim // 2
    theta = np.float64(base) ** (-2.0 * np.arange(half, dtype=np.float64) / max(rot_dim, 1))
    ang = np.arange(max_pos, dtype=np.float64)[:, None] * theta[None, :]
    t = torch.from_numpy(np.concatenate([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32))
    return t if device is None else t.to(device)


def rope_append(q, k, v, cs, block_table=None, k_cache=None, v_cache=None, positions=None, token_seq=None, seq_lens=None, rot_dim=None, style="neox",
                q_out=None, k_out=None):
    """RoPE on every Q and K head and the append of K and V to the paged cache, in one launch (sm_rope_append_*).  q: [tokens][q_heads][head_dim],
    k, v: [tokens][kv_heads][head_dim], float16 / bfloat16 with contiguous heads (any row pitch: column slices of a fused QKV output); cs: the
    float32 table [max_pos][rot_dim] (rope_table; any row pitch), or None with rot_dim 0; rot_dim: cs.shape[1] when None.  k_cache, v_cache:
    [num_pages][page_size][kv_heads][head_dim] in attn_decode's layout with block_table int32 [seqs][max_pages], or all three None (then k_out is
    required).  positions, token_seq: int32 [tokens] or None; seq_lens: int32 [seqs] or None -- positions None takes seq_lens[s] - 1, token_seq
    None takes token i as sequence i (the decode step).  style: "neox" or "interleaved".  q_out: None means in place (q itself); k_out: None means
    not written, k itself is the in-place update.  Returns q_out."""
    torch = _t()
    what = "rope_append"
    sfx = _quant_src_sfx(q, what)
    if style not in _ROPE_STYLES:
        raise SparsifymeError(f"{what}: style is 'neox' or 'interleaved'")
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise SparsifymeError(f"{what}: q is [tokens][q_heads][head_dim], k and v are [tokens][kv_heads][head_dim]")
    tokens, q_heads, head_dim = q.shape
    kv_heads = k.shape[1]
    if tuple(k.shape) != (tokens, kv_heads, head_dim) or tuple(v.shape) != tuple(k.shape) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise SparsifymeError(f"{what}: k and v are [tokens][kv_heads][head_dim] of q's dtype")
    if q_out is None:
        q_out = q
    for name, t, heads in (("q", q, q_heads), ("k", k, kv_heads), ("v", v, kv_heads), ("q_out", q_out, q_heads), ("k_out", k_out, kv_heads)):
        if t is not None:
            _heads3(what, name, t, q.dtype, (tokens, heads, head_dim))
    if cs is None:
        if rot_dim not in (None, 0):
            raise SparsifymeError(f"{what}: rot_dim > 0 needs the table cs")
        rot_dim, max_pos, ldcs = 0, 0, 0
    else:
        if cs.dim() != 2 or cs.dtype != torch.float32 or (cs.shape[1] > 1 and cs.stride(1) != 1):
            raise SparsifymeError(f"{what}: cs is float32 [max_pos][rot_dim] with contiguous rows (any row pitch)")
        max_pos = cs.shape[0]
        rot_dim = cs.shape[1] if rot_dim is None else rot_dim
        if rot_dim > cs.shape[1]:
            raise SparsifymeError(f"{what}: rot_dim exceeds the table's row")
        ldcs = cs.stride(0) if max_pos > 1 else max(cs.stride(0), cs.shape[1])
    row = lambda t, heads: _pitch(t, 0, heads * head_dim)
    num_pages = page_size = max_pages = ldkv = page_stride = ldbt = 0
    seqs = None
    if (k_cache is None) != (v_cache is None) or (k_cache is None) != (block_table is None):
        raise SparsifymeError(f"{what}: k_cache, v_cache and block_table are given together, or not at all")
    if k_cache is not None:
        num_pages, page_size, max_pages, seqs, ldkv, page_stride, ldbt = _paged_cache(what, k_cache, v_cache, block_table, q.dtype, kv_heads, head_dim)
    for name, t in (("positions", positions), ("token_seq", token_seq)):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (tokens,) or not t.is_contiguous()):
            raise SparsifymeError(f"{what}: {name} is a contiguous int32 [tokens]")
    if seq_lens is not None:
        if seq_lens.dtype != torch.int32 or seq_lens.dim() != 1 or not seq_lens.is_contiguous() or (seqs is not None and seq_lens.shape[0] != seqs):
            raise SparsifymeError(f"{what}: seq_lens is a contiguous int32 [seqs]")
        seqs = seq_lens.shape[0]
    if seqs is None:
        seqs = tokens                  # no cache and no lengths: the sequence ids address nothing
    ptr = lambda t: _dev(t) if t is not None else None
    fn = getattr(lib(), "sm_rope_append_" + sfx)
    _check(fn(_dev(q), _dev(k), _dev(v), _dev(q_out), ptr(k_out), ptr(k_cache), ptr(v_cache), ptr(cs) if rot_dim else None, ptr(positions), ptr(token_seq),
              ptr(seq_lens), ptr(block_table), tokens, seqs, q_heads, kv_heads, head_dim, rot_dim, max_pos, num_pages, page_size, max_pages,
              row(q, q_heads), row(k, kv_heads), row(v, kv_heads), row(q_out, q_heads), row(k_out, kv_heads) if k_out is not None else 0, ldkv, page_stride,
              ldcs, ldbt, _ROPE_STYLES[style], _stream()), "sm_rope_append")
    return q_out


def _paged_cache8(what, k_cache, v_cache, k_scale, v_scale, block_table, kv_heads, head_dim):
    """The fp8 paged KV cache as attn_decode_kv8 and rope_append_kv8 take it (csrc/paged_kv.h), checked: the byte tensors through _paged_cache
    in their own fp8 dtype, the scales float32 [num_pages][kv_heads][page_size] with contiguous heads (any page pitch).  Returns _paged_cache's
    tuple, then scale_page_stride and fmt."""
    fmt = fp8_format(k_cache.dtype)
    geo = _paged_cache(what, k_cache, v_cache, block_table, k_cache.dtype, kv_heads, head_dim)
    num_pages, page_size = geo[0], geo[1]
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if t.dtype != _t().float32 or tuple(t.shape) != (num_pages, kv_heads, page_size) or (page_size > 1 and t.stride(2) != 1) or \
                (kv_heads > 1 and t.stride(1) != page_size) or t.stride() != k_scale.stride():
            raise SparsifymeError(f"{what}: {name} is float32 [num_pages][kv_heads][page_size] with contiguous heads, both at the same strides")
    return geo + (_pitch(k_scale, 0, kv_heads * page_size), fmt)


def rope_append_kv8(q, k, v, cs, block_table, k_cache, v_cache, k_scale, v_scale, positions=None, token_seq=None, seq_lens=None, rot_dim=None,
                    style="neox", q_out=None, k_out=None):
    """rope_append with the append going to the fp8 cache (sm_rope_append_kv8_*): k_cache, v_cache are float8_e4m3fn or float8_e5m2
    [num_pages][page_size][kv_heads][head_dim] (one dtype for both), k_scale, v_scale float32 [num_pages][kv_heads][page_size]; each
    appended K head (rotated, rounded to q's dtype) and V head is one row of quantize_rows_fp8: its bytes go to the token's cache row, its
    row_scale to [page][head][slot].  All four and block_table are required; everything else as rope_append.  Returns q_out."""
    torch = _t()
    what = "rope_append_kv8"
    sfx = _quant_src_sfx(q, what)
    if style not in _ROPE_STYLES:
        raise SparsifymeError(f"{what}: style is 'neox' or 'interleaved'")
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise SparsifymeError(f"{what}: q is [tokens][q_heads][head_dim], k and v are [tokens][kv_heads][head_dim]")
    tokens, q_heads, head_dim = q.shape
    kv_heads = k.shape[1]
    if tuple(k.shape) != (tokens, kv_heads, head_dim) or tuple(v.shape) != tuple(k.shape) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise SparsifymeError(f"{what}: k and v are [tokens][kv_heads][head_dim] of q's dtype")
    if q_out is None:
        q_out = q
    for name, t, heads in (("q", q, q_heads), ("k", k, kv_heads), ("v", v, kv_heads), ("q_out", q_out, q_heads), ("k_out", k_out, kv_heads)):
        if t is not None:
            _heads3(what, name, t, q.dtype, (tokens, heads, head_dim))
    if cs is None:
        if rot_dim not in (None, 0):
            raise SparsifymeError(f"{what}: rot_dim > 0 needs the table cs")
        rot_dim, max_pos, ldcs = 0, 0, 0
    else:
        if cs.dim() != 2 or cs.dtype != torch.float32 or (cs.shape[1] > 1 and cs.stride(1) != 1):
            raise SparsifymeError(f"{what}: cs is float32 [max_pos][rot_dim] with contiguous rows (any row pitch)")
        max_pos = cs.shape[0]
        rot_dim = cs.shape[1] if rot_dim is None else rot_dim
        if rot_dim > cs.shape[1]:
            raise SparsifymeError(f"{what}: rot_dim exceeds the table's row")
        ldcs = cs.stride(0) if max_pos > 1 else max(cs.stride(0), cs.shape[1])
    row = lambda t, heads: _pitch(t, 0, heads * head_dim)
    num_pages, page_size, max_pages, seqs, ldkv, page_stride, ldbt, sps, fmt = _paged_cache8(what, k_cache, v_cache, k_scale, v_scale, block_table, kv_heads, head_dim)
    for name, t in (("positions", positions), ("token_seq", token_seq)):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (tokens,) or not t.is_contiguous()):
            raise SparsifymeError(f"{what}: {name} is a contiguous int32 [tokens]")
    if seq_lens is not None and (seq_lens.dtype != torch.int32 or seq_lens.dim() != 1 or not seq_lens.is_contiguous() or seq_lens.shape[0] != seqs):
        raise SparsifymeError(f"{what}: seq_lens is a contiguous int32 [seqs]")
    ptr = lambda t: _dev(t) if t is not None else None
    fn = getattr(lib(), "sm_rope_append_kv8_" + sfx)
    _check(fn(_dev(q), _dev(k), _dev(v), _dev(q_out), ptr(k_out), _dev(k_cache), _dev(v_cache), _dev(k_scale), _dev(v_scale), ptr(cs) if rot_dim else None,
              ptr(positions), ptr(token_seq), ptr(seq_lens), _dev(block_table), tokens, seqs, q_heads, kv_heads, head_dim, rot_dim, max_pos, num_pages, page_size,
              max_pages, row(q, q_heads), row(k, kv_heads), row(v, kv_heads), row(q_out, q_heads), row(k_out, kv_heads) if k_out is not None else 0, ldkv,
              page_stride, sps, ldcs, ldbt, _ROPE_STYLES[style], fmt, _stream()), "sm_rope_append_kv8")
    return q_out


def attn_decode_kv8(q, k_cache, v_cache, k_scale, v_scale, block_table, seq_lens, scale=None, out=None, lse=None, workspace=None):
    """attn_decode over the fp8 cache (sm_attn_decode_kv8_*): k_cache, v_cache float8_e4m3fn or float8_e5m2 [num_pages][page_size][kv_heads]
    [head_dim] (one dtype for both), k_scale, v_scale float32 [num_pages][kv_heads][page_size]; q, out, lse, scale and workspace as
    attn_decode (attn_decode_form and attn_decode_workspace_size serve this call too).  Returns out."""
    torch = _t()
    what = "attn_decode_kv8"
    sfx = _quant_src_sfx(q, what)
    if q.dim() != 3 or seq_lens.dim() != 1:
        raise SparsifymeError(f"{what}: q is [seqs][q_heads][head_dim], seq_lens [seqs]")
    seqs, q_heads, head_dim = q.shape
    kv_heads = k_cache.shape[2] if k_cache.dim() == 4 else 0
    num_pages, page_size, max_pages, table_seqs, ldkv, page_stride, ldbt, sps, fmt = _paged_cache8(what, k_cache, v_cache, k_scale, v_scale, block_table, kv_heads,
                                                                                                   head_dim)
    if table_seqs != seqs or seq_lens.dtype != torch.int32 or seq_lens.shape[0] != seqs or not seq_lens.is_contiguous():
        raise SparsifymeError(f"{what}: block_table is [seqs][max_pages], seq_lens a contiguous int32 [seqs]")
    if out is None:
        out = torch.empty((seqs, q_heads, head_dim), dtype=q.dtype, device=q.device)
    for name, t in (("q", q), ("out", out)):
        _heads3(what, name, t, q.dtype, (seqs, q_heads, head_dim))
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != (seqs, q_heads) or not lse.is_contiguous()):
        raise SparsifymeError(f"{what}: lse is a contiguous float32 [seqs][q_heads]")
    ldq, ldo = _pitch(q, 0, q_heads * head_dim), _pitch(out, 0, q_heads * head_dim)
    need = attn_decode_workspace_size(seqs, q_heads, head_dim, page_size, max_pages)
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=q.device)
    ws_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    fn = getattr(lib(), "sm_attn_decode_kv8_" + sfx)
    _check(fn(_dev(q), _dev(k_cache), _dev(v_cache), _dev(k_scale), _dev(v_scale), _dev(block_table), _dev(seq_lens), _dev(out),
              _dev(lse) if lse is not None else None, _dev(workspace) if workspace is not None else None, ws_bytes, seqs, q_heads, kv_heads, head_dim,
              num_pages, page_size, max_pages, ldq, ldkv, page_stride, sps, ldbt, ldo, float(head_dim ** -0.5 if scale is None else scale), fmt, _stream()),
           "sm_attn_decode_kv8")
    return out


def quantize_compress24_fp8(A, blob, row_scale, rows, k, fmt_dtype, lda=None):
    """quantize_rows_fp8 + compress24_fp8 in one pass over A: blob of compress24_size(rows, k, 1, 1) bytes (fmt_dtype: the fp8
    dtype, the blob does not carry it) and row_scale[rows]."""
    sfx = _quant_src_sfx(A, "quantize_compress24_fp8")
    fmt = fp8_format(fmt_dtype)
    rs = _quant_row_scale(row_scale, "quantize_compress24_fp8")
    fn = getattr(lib(), "sm_quantize_compress24_fp8_" + sfx)
    _check(fn(_dev(A), rows, k, k if lda is None else lda, _dev(blob), rs, fmt, _stream()), "sm_quantize_compress24_fp8")


def quantize_transpose_fp8(B, Bt, k, n, inv_scale, ldb=None):
    """Row-major k x n float16 / bfloat16 B -> Bt [n][k] fp8 (the format of Bt's dtype), q = rne(clamp(b * inv_scale))."""
    sfx = _quant_src_sfx(B, "quantize_transpose_fp8")
    fmt = fp8_format(Bt.dtype)
    fn = getattr(lib(), "sm_quantize_transpose_fp8_" + sfx)
    _check(fn(_dev(B), k, n, n if ldb is None else ldb, float(inv_scale), _dev(Bt), fmt, _stream()), "sm_quantize_transpose_fp8")


def gemm_rowmajor_i8(A, B, C, m, n, k, lda=None, batch=1, strideA=None, strideB=0, strideC=None, accumulate=False):
    """dense int8 GEMM: C (int32) = A . B (+ C when accumulate); A row-major m x k int8, B [n][k] int8."""
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    if C.dtype != _t().int32:
        raise SparsifymeError("gemm_rowmajor_i8 writes int32; use gemm_rowmajor_i8_q for a requantised int8 result")
    _check(lib().sm_gemm_rowmajor_i8(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, 1 if accumulate else 0,
                                     _stream()), "sm_gemm_rowmajor_i8")


def gemm_rowmajor_i8_q(A, B, C, m, n, k, scale, lda=None, batch=1, strideA=None, strideB=0, strideC=None):
    """dense int8 GEMM requantised to int8: C = saturate(rne(scale * acc))."""
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    if C.dtype != _t().int8:
        raise SparsifymeError("gemm_rowmajor_i8_q writes int8")
    _check(lib().sm_gemm_rowmajor_i8_q(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, float(scale), _stream()),
           "sm_gemm_rowmajor_i8_q")


def spmma_fused_workspace_size():
    out = _c_size(0)
    _check(lib().sm_spmma_fused_workspace_size(ctypes.byref(out)), "sm_spmma_fused_workspace_size")
    return out.value


def spmma_fused_streamk_plan(rows, n, k, problems=1):
    """(takes, plan): whether the workspace entry points run the stream-K form on `problems` problems of rows x n x k, and its
    decomposition as a dict (tg, wg, groups_full, tgl, wgl, slots, units, cut, cutl) -- sm_spmma_fused_streamk_plan."""
    takes = _c_i(0)
    buf = (ctypes.c_uint * 32)()   # the entry point writes plan[0 .. 24] (include/sparsifyme.h: >= 25 unsigned)
    _check(lib().sm_spmma_fused_streamk_plan(rows, n, k, problems, ctypes.byref(takes), buf), "sm_spmma_fused_streamk_plan")
    v = list(buf)
    return bool(takes.value), dict(tg=v[0], wg=v[1], groups_full=v[2], tgl=v[3], wgl=v[4], slots=v[5], units=v[6], cut=v[7:16], cutl=v[16:25])


# include/sparsifyme.h: SM_FUSED_FORM_* (index = value) and SM_FUSED_FLAG_*
FUSED_FORMS = ("not_taken", "empty", "thin", "span", "streamk", "big", "direct64", "direct128", "direct128_nt", "astat", "widep", "wide", "wide_nt")
FUSED_FLAG_A_ALIGNED, FUSED_FLAG_B_ALIGNED, FUSED_FLAG_C_ALIGNED, FUSED_FLAG_WORKSPACE, FUSED_FLAG_EPILOGUE = 1, 2, 4, 8, 16


def spmma_fused_form(m, n, k, lda=None, batch=1, count=1, strideA=None, strideB=0, strideC=None, beta=0.0, a_aligned=True, b_aligned=True,
                     c_aligned=True, workspace=False, epilogue=False, cus=0):
    """The name (FUSED_FORMS) of the kernel form spmma_fused / spmma_fused_grouped run for this launch -- sm_spmma_fused_form, the
    rule the entry points themselves switch on.  cus=0: this device's compute units; another value: host-only."""
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    flags = ((FUSED_FLAG_A_ALIGNED if a_aligned else 0) | (FUSED_FLAG_B_ALIGNED if b_aligned else 0) | (FUSED_FLAG_C_ALIGNED if c_aligned else 0) |
             (FUSED_FLAG_WORKSPACE if workspace else 0) | (FUSED_FLAG_EPILOGUE if epilogue else 0))
    form = _c_i(-1)
    _check(lib().sm_spmma_fused_form(m, n, k, lda, batch, count, strideA, strideB, strideC, float(beta), flags, cus, ctypes.byref(form)),
           "sm_spmma_fused_form")
    return FUSED_FORMS[form.value]


def streamk_whole_panels(plan, panels, nkt):
    """The row panels (0 .. panels - 1) that lie inside ONE slot range of `plan` (their tiles equal the no-workspace result bit for bit)."""
    cuts = set()
    for g in range(plan["groups_full"]):
        cuts.update(g * plan["tg"] * nkt + c for c in plan["cut"][:plan["wg"] + 1])
    base = plan["groups_full"] * plan["tg"] * nkt
    cuts.update(base + c for c in plan["cutl"][:plan["wgl"] + 1])
    return [t for t in range(panels) if not any(t * nkt < u < (t + 1) * nkt for u in cuts)]


def spmma_fused_workspace_state(ws):
    """0 = the workspace's flag page is clean; 1 = a stream-K fix-up timed out (that launch's C is invalid); 2 = flags raised without a recorded
    timeout.  Blocks on the current stream (sm_spmma_fused_workspace_state); after 1 / 2 zero the first 4096 bytes before the next call."""
    st = _c_i(-1)
    _check(lib().sm_spmma_fused_workspace_state(_dev(ws), ctypes.byref(st), _stream()), "sm_spmma_fused_workspace_state")
    return st.value


def spmma_fused_workspace():
    """A zeroed workspace for the `workspace=` argument of spmma_fused / spmma_fused_grouped (the stream-K form; one per concurrent call)."""
    return _t().zeros(spmma_fused_workspace_size(), dtype=_t().uint8, device="cuda")


def spmma_fused(A, B, C, m, n, k, lda=None, batch=1, strideA=None, strideB=0, strideC=None, alpha=1.0, beta=0.0, workspace=None,
                epilogue=None):
    """Fused prune(STRIP) + compress + 2:4 matmul straight from the dense A (no blob).  workspace (spmma_fused_workspace()): the
    library may run the stream-K form where whole-tile rounds leave CUs idle.  epilogue: an Epilogue (sm_spmma_fused_*_ex; not with a
    workspace)."""
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    if epilogue is not None:
        if workspace is not None:
            raise SparsifymeError("spmma_fused: the workspace (stream-K) form takes no epilogue")
        st = epilogue.struct_for(C, strideC, float(beta))
        fn = getattr(lib(), "sm_spmma_fused_%s_ex" % _sfx(A))
        _check(fn(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, float(alpha), float(beta), ctypes.addressof(st),
                  _stream()), "sm_spmma_fused_ex")
        return
    if workspace is not None:
        fn = getattr(lib(), "sm_spmma_fused_%s_ws" % _sfx(A))
        _check(fn(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, float(alpha), float(beta), _dev(workspace),
                  workspace.numel() * workspace.element_size(), _stream()), "sm_spmma_fused_ws")
        return
    fn = getattr(lib(), "sm_spmma_fused_" + _sfx(A))
    _check(fn(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, float(alpha), float(beta), _stream()),
           "sm_spmma_fused")


def spmma_grouped(blobs, Bs, Cs, m, n, k, batch=1, strideB=0, strideC=None, alpha=1.0, beta=0.0):
    """The matmul step on len(blobs) same-shape compressed operands in one grid per 8 (sm_spmma_*_grouped): the same C as that many
    spmma() calls."""
    if not (len(blobs) == len(Bs) == len(Cs)):
        raise SparsifymeError("spmma_grouped: operand lists differ in length")
    if not blobs:
        return
    if strideC is None:
        strideC = m * n
    fn = getattr(lib(), "sm_spmma_%s_grouped" % _sfx(Bs[0]))
    _check(fn(len(blobs), _ptr_table(blobs), _ptr_table(Bs), _ptr_table(Cs), m, n, k, batch, strideB, strideC, float(alpha), float(beta),
              _stream()), "sm_spmma_grouped")


def spmma_fused_f32_split_workspace(n, k, batch=1, strideB=0, planes=3):
    out = _c_size(0)
    _check(lib().sm_spmma_fused_f32_split_workspace(n, k, batch, strideB, planes, ctypes.byref(out)), "sm_spmma_fused_f32_split_workspace")
    return out.value


def spmma_fused_f32_split(A, B, C, m, n, k, workspace, lda=None, batch=1, strideA=None, strideB=0, strideC=None, planes=3, alpha=1.0,
                          beta=0.0, check=True, dense=False):
    """fp32 2:4 product on the sparse matrix instruction through exact bfloat16 splits (sm_spmma_fused_f32_split); `workspace`:
    a uint8 tensor of spmma_fused_f32_split_workspace(...) bytes.  Returns the status (check=False: NOT_SUPPORTED is returned)."""
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    fn = lib().sm_gemm_rowmajor_f32_split if dense else lib().sm_spmma_fused_f32_split  # dense: every element of A multiplied
    rc = fn(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, planes, _dev(workspace),
            workspace.numel() * workspace.element_size(), float(alpha), float(beta), _stream())
    if check or rc not in (0, STATUS_NOT_SUPPORTED):
        _check(rc, "sm_spmma_fused_f32_split")
    return rc


def spmma_fused_f32_split_prepare(B, n, k, workspace, batch=1, strideB=0, planes=3):
    """Split B (fp32, k x n) into its bfloat16 planes once (weights that stay the same across calls): sm_spmma_fused_f32_split_prepare."""
    _check(lib().sm_spmma_fused_f32_split_prepare(_dev(B), n, k, batch, strideB, planes, _dev(workspace), workspace.numel() * workspace.element_size(), _stream()),
           "sm_spmma_fused_f32_split_prepare")


def spmma_fused_f32_split_prepared(A, workspace, C, m, n, k, lda=None, batch=1, strideA=None, strideB=0, strideC=None, planes=3, alpha=1.0, beta=0.0, check=True):
    """The split-form product from prepared planes of B (spmma_fused_f32_split_prepare): same C as spmma_fused_f32_split, no per-call pass over B."""
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    rc = lib().sm_spmma_fused_f32_split_prepared(_dev(A), _dev(workspace), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, planes,
                                                 workspace.numel() * workspace.element_size(), float(alpha), float(beta), _stream())
    if check or rc not in (0, STATUS_NOT_SUPPORTED):
        _check(rc, "sm_spmma_fused_f32_split_prepared")
    return rc


def _ptr_table(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[_dev(t).value for t in tensors])
    return arr


def spmma_fused_grouped(As, Bs, Cs, m, n, k, lda=None, batch=1, strideA=None, strideB=0, strideC=None, alpha=1.0, beta=0.0, workspace=None):
    """len(As) same-shape problems in one grid per 8 (sm_spmma_fused_*_grouped): the same C as len(As) spmma_fused calls."""
    if not (len(As) == len(Bs) == len(Cs)):
        raise SparsifymeError("spmma_fused_grouped: operand lists differ in length")
    if not As:
        return
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    if workspace is not None:
        fn = getattr(lib(), "sm_spmma_fused_%s_grouped_ws" % _sfx(As[0]))
        _check(fn(len(As), _ptr_table(As), _ptr_table(Bs), _ptr_table(Cs), m, n, k, lda, batch, strideA, strideB, strideC,
                  float(alpha), float(beta), _dev(workspace), workspace.numel() * workspace.element_size(), _stream()), "sm_spmma_fused_grouped_ws")
        return
    fn = getattr(lib(), "sm_spmma_fused_%s_grouped" % _sfx(As[0]))
    _check(fn(len(As), _ptr_table(As), _ptr_table(Bs), _ptr_table(Cs), m, n, k, lda, batch, strideA, strideB, strideC,
              float(alpha), float(beta), _stream()), "sm_spmma_fused_grouped")


def transpose(src, dst, rows, cols, ld_in=None, ld_out=None, batch=1, stride_in=None, stride_out=None):
    """dst[b][c][r] = src[b][r][c] (row-major, out of place): the transposed operands of sparsifyme::spmma."""
    ld_in = cols if ld_in is None else ld_in
    ld_out = rows if ld_out is None else ld_out
    stride_in = rows * ld_in if stride_in is None else stride_in
    stride_out = cols * ld_out if stride_out is None else stride_out
    _check(lib().sm_transpose(_dev(src), _dev(dst), rows, cols, ld_in, ld_out, src.element_size(), batch, stride_in, stride_out,
                              _stream()), "sm_transpose")


def conv_out_size(size, kernel, stride=1, pad=0, dilation=1):
    out = ctypes.c_size_t(0)
    _check(lib().sm_conv_out_size(size, kernel, stride, pad, dilation, ctypes.byref(out)), "sm_conv_out_size")
    return out.value


def im2col(X, N, C, H, W, kh, kw, stride, pad, dilation, out, compress=False):
    """NCHW activations -> the matmul operand A [N][L][C*kh*kw] (compress=False) or its 2:4 blob (compress=True)."""
    fn = getattr(lib(), ("sm_im2col_compress24_" if compress else "sm_im2col_") + _sfx(X))
    _check(fn(_dev(X), N, C, H, W, kh, kw, stride, pad, dilation, _dev(out), _stream()), "sm_im2col")


def conv_spmma_fused(X, B, C, N, Cin, H, W, kh, kw, stride, pad, dilation, n_out, alpha=1.0, beta=0.0):
    """Implicit-GEMM 2:4 convolution matmul straight from NCHW activations (no dense A, no blob)."""
    fn = getattr(lib(), "sm_conv_spmma_fused_" + _sfx(X))
    _check(fn(_dev(X), _dev(B), _dev(C), N, Cin, H, W, kh, kw, stride, pad, dilation, n_out, float(alpha), float(beta), _stream()),
           "sm_conv_spmma_fused")


# include/sparsifyme.h: SM_CONV_FORM_* (index = value), SM_CONV_FLAG_* and the words of the plan
CONV_FORMS = ("not_taken", "empty", "v16", "small4", "large4")
CONV_FLAG_X_ALIGNED16, CONV_FLAG_X_ALIGNED4, CONV_FLAG_B_ALIGNED16 = 1, 2, 4
CONV_PLAN_FIELDS = ("bn", "RI", "pitch", "padl", "rpi", "nch", "a_n", "patch_bytes", "lds", "tiles_m", "tiles_n")


def conv_spmma_fused_plan(N, Cin, H, W, kh, kw, stride, pad, dilation, n_out, x_align=16, b_aligned=True):
    """(form, plan): the name (CONV_FORMS) of the kernel class conv_spmma_fused runs for this layer and the stage plan it is launched
    with as a dict (CONV_PLAN_FIELDS) -- sm_conv_spmma_fused_plan, the rule the entry points themselves switch on.  x_align: the
    largest of 16, 4, 2 that divides X's address.  Host-only."""
    flags = ((CONV_FLAG_X_ALIGNED16 | CONV_FLAG_X_ALIGNED4) if x_align % 16 == 0 else CONV_FLAG_X_ALIGNED4 if x_align % 4 == 0 else 0) | \
            (CONV_FLAG_B_ALIGNED16 if b_aligned else 0)
    form = _c_i(-1)
    buf = (ctypes.c_uint * len(CONV_PLAN_FIELDS))()
    _check(lib().sm_conv_spmma_fused_plan(N, Cin, H, W, kh, kw, stride, pad, dilation, n_out, flags, ctypes.byref(form), buf),
           "sm_conv_spmma_fused_plan")
    return CONV_FORMS[form.value], dict(zip(CONV_PLAN_FIELDS, list(buf)))


def conv_spmma_workspace(N, Cin, H, W, kh, kw, stride, pad, dilation):
    out = _c_size(0)
    _check(lib().sm_conv_spmma_workspace(N, Cin, H, W, kh, kw, stride, pad, dilation, ctypes.byref(out)), "sm_conv_spmma_workspace")
    return out.value


def conv_spmma(X, B, C, N, Cin, H, W, kh, kw, stride, pad, dilation, n_out, workspace=None, alpha=1.0, beta=0.0):
    """The convolution-layer 2:4 product by the faster route (implicit GEMM, or im2col-to-blob + matmul for small-spatial long-K layers)."""
    fn = getattr(lib(), "sm_conv_spmma_" + _sfx(X))
    wb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    _check(fn(_dev(X), _dev(B), _dev(C), N, Cin, H, W, kh, kw, stride, pad, dilation, n_out, float(alpha), float(beta),
              _dev(workspace) if workspace is not None else None, wb, _stream()), "sm_conv_spmma")


def _bell_sfx(values):
    torch = _t()
    sfx = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}.get(values.dtype)
    if sfx is None:
        raise SparsifymeError(f"spmm_bell: values must be float16, bfloat16 or float32, not {values.dtype}")
    return sfx


def spmm_bell(values, column_indices, B, C, rows, cols, block_size, ell_cols, n, alpha=1.0, beta=0.0):
    """sparsifyme::batched::spmm for one Blocked-ELL A (spmm.hxx:57-67,107-110): C (rows x n, column-major) = alpha * A * B + beta * C.
    values [rows][ell_cols] and B / C in fp16, bf16 (the 16-bit matrix-core kernel) or fp32 (the fp32 route, with its workspace
    allocated here); column_indices int64 / uint64 [ceil(rows/block_size)][ell_cols/block_size]."""
    sfx = _bell_sfx(values)
    if sfx in ("f16", "bf16"):
        fn = getattr(lib(), "sm_spmm_bell_" + sfx)
        _check(fn(_dev(values), _dev(column_indices), rows, cols, block_size, ell_cols, _dev(B), _dev(C), n, float(alpha), float(beta),
                  _stream()), "sm_spmm_bell_" + sfx)
        return
    nb = _c_size(0)
    _check(lib().sm_spmm_bell_workspace_size(rows, cols, ctypes.byref(nb)), "sm_spmm_bell_workspace_size")
    ws = _t().empty(max(nb.value, 1), dtype=_t().uint8, device=values.device)
    _check(lib().sm_spmm_bell_f32_ws(_dev(values), _dev(column_indices), rows, cols, block_size, ell_cols, _dev(B), _dev(C), n, float(alpha),
                                     float(beta), _dev(ws), _stream()), "sm_spmm_bell_f32_ws")


def spmm_bell_batched(values_list, indices_list, B, C_list, rows, cols, block_size, ell_cols, n, alpha=1.0, beta=0.0):
    """All batches of sparsifyme::batched::spmm in one submission: one A (values, indices) and one C per entry, B shared.
    fp16 / bf16: sm_spmm_bell_batched_{f16,bf16} (no workspace); fp32: sm_spmm_bell_batched_f32 with its workspace allocated here."""
    if not (len(values_list) == len(indices_list) == len(C_list)):
        raise SparsifymeError("spmm_bell_batched: operand lists differ in length")
    if not values_list:
        return
    sfx = _bell_sfx(values_list[0])
    pv, pi, pc = _ptr_table(values_list), _ptr_table(indices_list), _ptr_table(C_list)
    batch = len(values_list)
    if sfx in ("f16", "bf16"):
        fn = getattr(lib(), "sm_spmm_bell_batched_" + sfx)
        _check(fn(pv, pi, rows, cols, block_size, ell_cols, _dev(B), pc, n, batch, float(alpha), float(beta), _stream()),
               "sm_spmm_bell_batched_" + sfx)
        return
    nb = _c_size(0)
    _check(lib().sm_spmm_bell_batched_workspace_size(rows, cols, batch, ctypes.byref(nb)), "sm_spmm_bell_batched_workspace_size")
    ws = _t().empty(max(nb.value, 1), dtype=_t().uint8, device=values_list[0].device)
    _check(lib().sm_spmm_bell_batched_f32(pv, pi, rows, cols, block_size, ell_cols, _dev(B), pc, n, batch, float(alpha), float(beta),
                                          _dev(ws), _stream()), "sm_spmm_bell_batched_f32")


def gemm_batched(A_ptrs, B_ptrs, C_ptrs, m, n, k, batch, dtype_suffix, alpha=1.0, beta=0.0, ta=0, tb=0, workspace=None):
    """sparsifyme::batched::gemm (gemm.hxx:25-36): column-major, device pointer arrays (int64 tensors)."""
    if workspace is not None and dtype_suffix == "f16":
        _check(lib().sm_gemm_batched_f16_ws(_dev(A_ptrs), _dev(B_ptrs), _dev(C_ptrs), m, n, k, batch, ta, tb, alpha, beta, _dev(workspace),
                                            workspace.numel() * workspace.element_size(), _stream()), "sm_gemm_batched_ws")
        return
    fn = getattr(lib(), "sm_gemm_batched_" + dtype_suffix)
    _check(fn(_dev(A_ptrs), _dev(B_ptrs), _dev(C_ptrs), m, n, k, batch, ta, tb, alpha, beta, _stream()),
           "sm_gemm_batched")


def gemm_rowmajor(A, B, C, m, n, k, lda=None, batch=1, strideA=None, strideB=0, strideC=None, alpha=1.0, beta=0.0, workspace=None):
    lda = k if lda is None else lda
    strideA = m * lda if strideA is None else strideA
    strideC = m * n if strideC is None else strideC
    if workspace is not None and _sfx(A) in ("f16", "bf16"):
        fn = getattr(lib(), "sm_gemm_rowmajor_%s_ws" % _sfx(A))
        _check(fn(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, float(alpha), float(beta), _dev(workspace),
                  workspace.numel() * workspace.element_size(), _stream()), "sm_gemm_rowmajor_ws")
        return
    fn = getattr(lib(), "sm_gemm_rowmajor_" + _sfx(A))
    _check(fn(_dev(A), _dev(B), _dev(C), m, n, k, lda, batch, strideA, strideB, strideC, float(alpha), float(beta),
              _stream()), "sm_gemm_rowmajor")


def copy_bytes(src, dst):
    """Streaming device-to-device copy of src's bytes into dst (bandwidth yardstick of bench.py)."""
    nbytes = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() < nbytes:
        raise SparsifymeError("copy_bytes: destination smaller than the source")
    _check(lib().sm_copy_bytes(_dev(src), _dev(dst), nbytes, _stream()), "sm_copy_bytes")


def fill_uniform(out, seed, lo=0.0, hi=1.0):
    fn = getattr(lib(), "sm_fill_uniform_" + _sfx(out))
    _check(fn(_dev(out), out.numel(), seed, float(lo), float(hi), _stream()), "sm_fill_uniform")
