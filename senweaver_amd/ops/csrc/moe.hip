// Grouped GEMM for MoE (Mixtral-style) on gfx950.
//
// After top-k routing, tokens are sorted by expert into A_sorted and each
// expert e owns rows [seg_starts[e], seg_starts[e+1]).  One launch computes
// every expert's C_seg = A_seg @ W_e^T: the host builds a flat tile map of
// (expert, m_tile) pairs (so no idle blocks for empty experts — router
// imbalance costs nothing extra), and each 256-thread block runs the same
// 128x128 glds-double-buffered MFMA pipeline as the dense GEMM, with
// per-row store masking at segment boundaries.
//
// W: [E, N, K] bf16 row-major.  A_sorted: [T_pad, N? no: K].  C: [T_pad, N].

#include "common.h"
#include "kernels.h"
#include "tile_gemm.h"

extern "C" __global__ void __launch_bounds__(256, 2)
grouped_gemm_bt_bf16_kernel(const ushort* __restrict__ A,  // [T_pad, K] sorted by expert
                            const ushort* __restrict__ W,  // [E, N, K]
                            ushort* __restrict__ C,        // [T_pad, N]
                            const int* __restrict__ tile_expert,  // [n_mtiles]
                            const int* __restrict__ tile_m0,      // [n_mtiles] row of tile start
                            const int* __restrict__ seg_ends,     // [E]
                            int N, int K, int tiles_n) {
  const int mt = blockIdx.x / tiles_n;
  const int tile_n = blockIdx.x % tiles_n;
  const int e = tile_expert[mt];
  const int m0 = tile_m0[mt];
  const int seg_end = seg_ends[e];
  // the dense 128-tile pipeline (tile_gemm.h): tile origin from the tile
  // map, no XCD remap, stores of rows >= seg_end masked
  gemm_bt_bf16_body<128, true>(A + (long long)m0 * K,
                               W + ((long long)e * N + (long long)tile_n * 128) * K,
                               C, (long long)m0, (long long)tile_n * 128, N, K,
                               seg_end);
}

// ---------------------------------------------------------------------------
// Routed-FFN combine: out[t] = sum_j w[pos(t,j)] * down[pos(t,j)]  (bf16).
// pos = inverse routing permutation [T, k] (each token's k rows in the
// expert-sorted layout), so every output row is a private k-way sum — no
// atomics, one pass, replacing zeros + f32 index_add_ + cast (three torch
// kernels, ~6% of the Mixtral step).
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
moe_combine_kernel(const ushort* __restrict__ down, const int* __restrict__ pos,
                   const float* __restrict__ weight, ushort* __restrict__ out,
                   int H, int k) {
  const long long t = blockIdx.x;
  const int nvec = H / 8;
  // per-token row indices + weights are wave-uniform scalars
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int j = 0; j < k; ++j) {
      const int p = pos[t * k + j];
      const float w = weight[p];
      bf16x8 v = *reinterpret_cast<const bf16x8*>(down + (long long)p * H + i * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += w * bf2f(v.v[e]);
    }
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.v[e] = f2bf(acc[e]);
    *reinterpret_cast<bf16x8*>(out + t * H + i * 8) = o;
  }
}
