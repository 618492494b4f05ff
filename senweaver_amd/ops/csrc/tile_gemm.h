// Shared device code of the single-barrier tiled GEMMs (gemm.hip, moe.hip,
// fp8.hip): "stage the next K-tile by global_load_lds, run MFMA on the
// current one, __syncthreads".
//
// A staged tile row is 128 bytes in every kernel (64 bf16 or 128 fp8) = 8
// chunks of 16 bytes, so one staging helper and one swizzle serve them all.
// The tile is square: TILE rows staged by 2 * TILE threads (128 / 256 or
// 256 / 512), waves in a 2 x (TILE / 64) grid, each owning TILE/2 x 64 of C.
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define TILE_ROW_BYTES 128
#define ROW_CHUNKS 8  // 16-byte chunks per tile row

// XCD-aware bijective remap of the flat workgroup id: neighboring tiles
// (sharing A/B panels) land on the same XCD's L2 (8 XCDs, private 4 MiB L2s).
__device__ __forceinline__ int xcd_remap(int wgid, int nwg) {
  const int q = nwg / 8, r = nwg % 8;
  const int xcd = wgid % 8, pos = wgid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}

// Stage THREADS/2 rows x 128 bytes from src (tile origin &X[row0*ld + k0],
// leading dimension ld in elements of T) into the lane-linear LDS tile.
template <int THREADS, typename T>
__device__ __forceinline__ void stage_tile_glds(
    const T* __restrict__ src, long long ld, T* lds_tile, int tid) {
  // THREADS/2 rows x 8 chunks staged by THREADS threads -> 4 glds each.
  // Linear slot s holds global chunk (row = s/8, c = (s%8) ^ (row&7)):
  // inverse-swizzled source + swizzled read = same involution (rule 21).
  // The swizzle sits on the SOURCE address because glds writes lane-linear:
  // lane destination = wave-uniform base + lane*16, so the base must
  // include this wave's 64-chunk sub-block, not just the iteration offset.
  constexpr int CHUNK = 16 / sizeof(T);  // elements per 16-byte chunk
  const int wave_chunk = tid & ~63;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = i * THREADS + tid;
    const int row = s >> 3;
    const int c = (s & 7) ^ (row & 7);
    const T* g = src + (long long)row * ld + c * CHUNK;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)g,
        (__attribute__((address_space(3))) unsigned int*)(lds_tile + (long long)(i * THREADS + wave_chunk) * CHUNK),
        16, 0, 0);
  }
}

// ---- swizzled fragment reads of logical (row, chunk) ----
// bf16: one ds_read_b128 (8 bf16 of chunk c)
__device__ __forceinline__ short8 read_frag(const ushort* lds_tile, int row, int c) {
  const int slot = row * ROW_CHUNKS + (c ^ (row & 7));
  return *reinterpret_cast<const short8*>(lds_tile + slot * 8);
}

// fp8: 8 bytes at byte_off of the row
__device__ __forceinline__ long read_fp8_frag(const unsigned char* lds_tile, int row,
                                              int byte_off) {
  const int c = byte_off >> 4;
  const int phys = (c ^ (row & 7)) * 16 + (byte_off & 15);
  return *reinterpret_cast<const long*>(lds_tile + row * TILE_ROW_BYTES + phys);
}

// MX: two 16-B chunks (c0, c0+2), one from each 32-element scale block
__device__ __forceinline__ i32x8 read_mx_frag(const unsigned char* lds_tile,
                                              int row, int c0) {
  i32x8 out;
  const int p0 = (c0 ^ (row & 7)) * 16;
  const int p1 = ((c0 + 2) ^ (row & 7)) * 16;
  *reinterpret_cast<int4*>(&out) = *reinterpret_cast<const int4*>(lds_tile + row * TILE_ROW_BYTES + p0);
  *(reinterpret_cast<int4*>(&out) + 1) = *reinterpret_cast<const int4*>(lds_tile + row * TILE_ROW_BYTES + p1);
  return out;
}

// ---------------------------------------------------------------------------
// bf16 v_mfma_f32_16x16x32_bf16 body: one TILE x TILE tile of
// C = A @ B^T from Atile = &A[row0*K], Btile = &B[col0*K], BK = 64.
// Each wave owns TILE/2 x 64 = (TILE/32) x 4 fragments.  MASK drops the
// stores of rows >= row_end (grouped GEMM segment tails); the dense kernels
// compile no row compare.
// ---------------------------------------------------------------------------
template <int TILE, bool MASK>
static __device__ __forceinline__ void gemm_bt_bf16_body(
    const ushort* __restrict__ Atile, const ushort* __restrict__ Btile,
    ushort* __restrict__ C, long long row0, long long col0, int N, int K,
    long long row_end) {
  constexpr int THREADS = 2 * TILE;
  constexpr int BK = 64;
  constexpr int MI = TILE / 32;        // m-fragments per wave
  constexpr int WN = TILE / 64;        // waves along n (2 along m)

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int wm = wid / WN;
  const int wn = wid % WN;

  __shared__ __attribute__((aligned(16))) ushort lds[2][2][TILE * BK];  // [buf][A/B]

  f32x4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int m_base = wm * (TILE / 2);  // within tile
  const int n_base = wn * 64;
  const int frag_row = lane & 15;      // m or n within 16
  const int frag_kgrp = lane >> 4;     // k-group 0..3 (8 bf16 each)

  const int ntiles = K / BK;
  // Prologue: stage tile 0 into buffer 0
  stage_tile_glds<THREADS>(Atile, K, lds[0][0], tid);
  stage_tile_glds<THREADS>(Btile, K, lds[0][1], tid);
  __syncthreads();

  int buf = 0;
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) {
      stage_tile_glds<THREADS>(Atile + (long long)(t + 1) * BK, K, lds[buf ^ 1][0], tid);
      stage_tile_glds<THREADS>(Btile + (long long)(t + 1) * BK, K, lds[buf ^ 1][1], tid);
    }
    const ushort* Al = lds[buf][0];
    const ushort* Bl = lds[buf][1];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {  // two K=32 MFMA steps per BK=64
      short8 af[MI], bf[4];
      const int c = kk * 4 + frag_kgrp;  // logical chunk of this lane's 8 bf16
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        af[mi] = read_frag(Al, m_base + mi * 16 + frag_row, c);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        bf[ni] = read_frag(Bl, n_base + ni * 16 + frag_row, c);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();  // drains the in-flight glds (vmcnt 0) + barrier
    buf ^= 1;
  }

  // ---- Epilogue: C[m][n], C-fragment map row=(lane>>4)*4+e, col=lane&15 ----
  const long long c_row0 = row0 + m_base + (lane >> 4) * 4;
  const long long c_col0 = col0 + n_base + (lane & 15);
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long row = c_row0 + mi * 16 + e;
      if (MASK && row >= row_end) continue;
      ushort* crow = C + row * N;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        crow[c_col0 + ni * 16] = f2bf(acc[mi][ni][e]);
    }
  }
}
