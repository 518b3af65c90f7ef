// gvl_limits.h -- the batch limits that size arrays in kernel argument structs (gvl_internal.h) AND bound the host-only launch plans (gvl_attn_plan.h, gvl_prefill_plan.h,
// gvl_decode_plan.h), and the padded head dim that the attention kernels, the towers and the operator checks (gvl_op_check.h) agree on.
// No HIP header: any C++17 compiler reads it.
#pragma once

constexpr int GVL_MAX_DECODE_BATCH = 16;  // sequences decoded together: the weight stream is read ONCE for all of them;
                                          // = the 16 columns of the MFMA B operand of the skinny decode GEMM (gvl_decode.hip)
constexpr int GVL_MAX_VALU_BATCH = 4;     // the round-1 VALU GEMV (fallback for K % 256 != 0 geometries) holds B vectors in LDS: 1, 2 or 4
constexpr int GVL_MAX_PREFILL_BATCH = 8;  // most sequences whose rows share one pass of the prefill GEMMs (gvl_debug_set prefill_group picks 1 .. 8; default 4)

inline int pad_head(int dr) { return dr <= 64 ? 64 : (dr <= 96 ? 96 : (dr <= 128 ? 128 : -1)); }   // the head dim a kernel runs a real head dim on; -1: none
