// Prototypes of every kernel bindings.hip launches.  The kernels are
// extern "C", so a launch through a prototype that disagrees with the
// definition would link and run with misread arguments.  bindings.hip and
// every .hip file that defines one of these include this header: a definition
// that drifts from its declaration is a compile error ("conflicting types").
#pragma once

#include "common.h"

#define SW_KERNEL extern "C" __global__ void

// ---- elemwise.hip ----
SW_KERNEL rmsnorm_fwd_kernel(const ushort* x, const ushort* w, ushort* y,
                             ushort* residual, int hidden, float eps);
SW_KERNEL rope_fwd_kernel(ushort* q, ushort* k, const float* cos_sin,
                          const int* positions, int Hq, int Hk, int D);
SW_KERNEL rope_scatter_kernel(const ushort* qkv, long long ld, ushort* q_out,
                              ushort* k_out, const float* cos_sin,
                              const int* positions, int Hq, int Hk, int D, int S);
SW_KERNEL rope_scatter_packed_kernel(const ushort* qkv, long long ld,
                                     ushort* q_out, ushort* k_out,
                                     const float* cos_sin, const int* positions,
                                     int Hq, int Hk, int D, int S, int B,
                                     const int* skip, const int* base,
                                     const int* owner, long long Tp);
SW_KERNEL transpose_v_kernel(const ushort* qkv, long long ld, long long v_off,
                             ushort* vt, int B, int S, int Hk, int D);
SW_KERNEL transpose_v_packed_kernel(const ushort* qkv, long long ld,
                                    long long v_off, ushort* vt, int B, int S,
                                    int Hk, int D, const int* skip,
                                    const int* base, const int* owner,
                                    long long Tp);
SW_KERNEL rope_kv_append_kernel(const ushort* qkv, long long ld, ushort* q_out,
                                ushort* kcache, ushort* vcache,
                                const float* cos_sin, const int* positions,
                                const int* slot, int Hq, int Hk, int D);
SW_KERNEL swiglu_fwd_kernel(const ushort* gateup, ushort* y, long long rows,
                            int inter);
SW_KERNEL add_bf16_kernel(const ushort* a, const ushort* b, ushort* y,
                          long long n8);

// ---- sampling.hip ----
SW_KERNEL argmax_rows_kernel(const ushort* logits, int* out, int vocab);
SW_KERNEL target_logprob_kernel(const ushort* logits, const int* targets,
                                float* out, int vocab);

// ---- gemm.hip, gemm_pipe.hip, gemm_asm.hip: C[M,N] = A[M,K] @ B[N,K]^T ----
SW_KERNEL gemm_bt_bf16_kernel(const ushort* A, const ushort* B, ushort* C,
                              int M, int N, int K);
SW_KERNEL gemm_bt_bf16_256_kernel(const ushort* A, const ushort* B, ushort* C,
                                  int M, int N, int K);
SW_KERNEL gemm_bt_bf16_8ph_v14_kernel(const ushort* A, const ushort* B,
                                      ushort* C, int M, int N, int K);
SW_KERNEL gemm_bt_bf16_asm4_kernel(const ushort* A, const ushort* B, ushort* C,
                                   int M, int N, int K);
SW_KERNEL gemm_bt_bf16_asm7_kernel(const ushort* A, const ushort* B, ushort* C,
                                   int M, int N, int K);

// ---- gemm.hip: decode GEMV family ----
SW_KERNEL gemv_bt_bf16_v2_m1(const ushort* A, const ushort* B, ushort* C,
                             int M, int N, int K);
SW_KERNEL gemv_bt_bf16_v2_m2(const ushort* A, const ushort* B, ushort* C,
                             int M, int N, int K);
SW_KERNEL gemv_bt_bf16_v2_m4(const ushort* A, const ushort* B, ushort* C,
                             int M, int N, int K);
SW_KERNEL gemv_bt_bf16_v2_m8(const ushort* A, const ushort* B, ushort* C,
                             int M, int N, int K);
SW_KERNEL gemv_bt_bf16_v2_m16(const ushort* A, const ushort* B, ushort* C,
                              int M, int N, int K);
SW_KERNEL gemv_bt_bf16_v3_m1(const ushort* A, const ushort* B, ushort* C,
                             int M, int N, int K);
SW_KERNEL gemv_bt_bf16_v3w_m1(const ushort* A, const ushort* B, ushort* C,
                              int M, int N, int K);
SW_KERNEL swiglu_gemv_bt_bf16_m1(const ushort* GU, const ushort* B, ushort* C,
                                 int M, int N, int K);
SW_KERNEL gemv_bt_fp8w_m1(const ushort* X, const unsigned char* Bq,
                          const float* Bs, ushort* C, int M, int N, int K);
SW_KERNEL gemv_bt_fp8w_m2(const ushort* X, const unsigned char* Bq,
                          const float* Bs, ushort* C, int M, int N, int K);
SW_KERNEL gemv_bt_fp8w_m4(const ushort* X, const unsigned char* Bq,
                          const float* Bs, ushort* C, int M, int N, int K);
SW_KERNEL gemv_bt_fp8w_m8(const ushort* X, const unsigned char* Bq,
                          const float* Bs, ushort* C, int M, int N, int K);
SW_KERNEL gemv_bt_mxfp8w_m1(const ushort* X, const unsigned char* Bq,
                            const unsigned char* Bs, ushort* C, int M, int N,
                            int K);
SW_KERNEL gemv_bt_mxfp8w_m2(const ushort* X, const unsigned char* Bq,
                            const unsigned char* Bs, ushort* C, int M, int N,
                            int K);
SW_KERNEL gemv_bt_mxfp8w_m4(const ushort* X, const unsigned char* Bq,
                            const unsigned char* Bs, ushort* C, int M, int N,
                            int K);
SW_KERNEL gemv_bt_mxfp8w_m8(const ushort* X, const unsigned char* Bq,
                            const unsigned char* Bs, ushort* C, int M, int N,
                            int K);
SW_KERNEL gemv_norm_bt_bf16_m1(const ushort* x, const ushort* res_in,
                               const ushort* normw, const ushort* B, ushort* C,
                               ushort* res_out, int M, int N, int K, float eps);
SW_KERNEL gemv_norm_bt_bf16_m2(const ushort* x, const ushort* res_in,
                               const ushort* normw, const ushort* B, ushort* C,
                               ushort* res_out, int M, int N, int K, float eps);
SW_KERNEL gemv_norm_bt_bf16_m4(const ushort* x, const ushort* res_in,
                               const ushort* normw, const ushort* B, ushort* C,
                               ushort* res_out, int M, int N, int K, float eps);
SW_KERNEL gemv_norm_bt_bf16_m8(const ushort* x, const ushort* res_in,
                               const ushort* normw, const ushort* B, ushort* C,
                               ushort* res_out, int M, int N, int K, float eps);
SW_KERNEL gemv_norm_bt_bf16_m16(const ushort* x, const ushort* res_in,
                                const ushort* normw, const ushort* B, ushort* C,
                                ushort* res_out, int M, int N, int K, float eps);

// ---- moe.hip ----
SW_KERNEL grouped_gemm_bt_bf16_kernel(const ushort* A, const ushort* W,
                                      ushort* C, const int* tile_expert,
                                      const int* tile_m0, const int* seg_ends,
                                      int N, int K, int tiles_n);
SW_KERNEL moe_combine_kernel(const ushort* down, const int* pos,
                             const float* weight, ushort* out, int H, int k);

// ---- fp8.hip ----
SW_KERNEL quant_fp8_rowwise_kernel(const ushort* x, unsigned char* q,
                                   float* scales, int K);
SW_KERNEL gemm_bt_fp8_kernel(const unsigned char* A, const float* a_s,
                             const unsigned char* B, const float* b_s,
                             ushort* C, int M, int N, int K);
SW_KERNEL quant_mxfp8_kernel(const ushort* x, unsigned char* q,
                             unsigned char* scales, int K);
SW_KERNEL gemm_bt_mxfp8_kernel(const unsigned char* A, const unsigned char* As,
                               const unsigned char* B, const unsigned char* Bs,
                               ushort* C, int M, int N, int K);
SW_KERNEL gemm_bt_mxfp8_256_kernel(const unsigned char* A,
                                   const unsigned char* As,
                                   const unsigned char* B,
                                   const unsigned char* Bs, ushort* C, int M,
                                   int N, int K);

// ---- attention.hip, attention_v2.hip, attention_v5.hip: prefill ----
SW_KERNEL attn_fwd_bf16_kernel(const ushort* Q, const ushort* K,
                               const ushort* VT, ushort* O, int B, int H,
                               int Hk, int S, float scale);
SW_KERNEL attn_fwd_v2_kernel(const ushort* Q, const ushort* K, const ushort* VT,
                             ushort* OT, int B, int H, int Hk, int S,
                             float scale);
SW_KERNEL attn_fwd_v3_kernel(const ushort* Q, const ushort* K, const ushort* VT,
                             ushort* OT, int B, int H, int Hk, int S,
                             float scale);
SW_KERNEL attn_fwd_v5_kernel(const ushort* Q, const ushort* K, const ushort* VT,
                             ushort* OT, int B, int H, int Hk, int S,
                             float scale);
SW_KERNEL attn_fwd_v5_packed_kernel(const ushort* Q, const ushort* K,
                                    const ushort* VT, ushort* OT, int B, int H,
                                    int Hk, int S, float scale, const int* skip,
                                    const int* base, int Tp);
SW_KERNEL attn_fwd_v5_packed_rm_kernel(const ushort* Q, const ushort* K,
                                       const ushort* VT, ushort* O, int B,
                                       int H, int Hk, int S, float scale,
                                       const int* skip, const int* base,
                                       int Tp);
SW_KERNEL attn_fwd_v5_packed_rm_qkv_kernel(const ushort* Q, const ushort* K,
                                           const ushort* qkv, long long ld,
                                           long long v_off, long long Tq,
                                           ushort* O, int B, int H, int Hk,
                                           int S, float scale, const int* skip,
                                           const int* base, const int* owner,
                                           int Tp);

// ---- decode_attention.hip, paged_prefill_attention.hip ----
SW_KERNEL paged_decode_attn_partial_kernel(const ushort* Q, const ushort* Kcache,
                                           const ushort* Vcache, float* partials,
                                           const int* block_table,
                                           const int* ctx_lens, int H, int Hk,
                                           int max_pages, float scale);
SW_KERNEL paged_decode_attn_merge_kernel(const float* partials, ushort* O,
                                         int H);
SW_KERNEL paged_prefill_attn_kernel(const ushort* Q, const ushort* Kcache,
                                    const ushort* Vcache, ushort* O,
                                    const int* block_table, const int* ctx_lens,
                                    const int* q_lens, int Sq, int H, int Hk,
                                    int max_pages, float scale);

#undef SW_KERNEL
