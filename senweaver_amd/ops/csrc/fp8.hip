// fp8 (OCP e4m3) path for the 70B scorer (BASELINE config 5).
//
// gfx950 uses OCP e4m3fn (max 448), NOT MI300X's fnuz.  Weights are
// quantized once per-output-row, activations per-token-row on the fly;
// the GEMM runs v_mfma_f32_16x16x32_fp8_fp8 over a 128x128 tile with
// BK=128 (fp8 halves the staged bytes per K element, so the same 16 KiB
// LDS tile covers twice the K depth of the bf16 kernel) and the epilogue
// rescales by a_scale[m] * b_scale[n].
//
// Note on rates: non-MX-scaled fp8 MFMA runs at the bf16 rate on CDNA4
// (the 2x peak needs the MX block-scaled K=128 instructions — a follow-up);
// what this path buys today is halved weight/activation traffic and the
// fp8 numerics contract for ranking-stability testing.

#include "common.h"
#include "kernels.h"
#include "tile_gemm.h"

#define FBK 128  // fp8 K-tile depth (bytes == elements)

// ---------------------------------------------------------------------------
// Row-wise quantization: bf16 [rows, K] -> fp8 bytes + f32 scale per row.
//   scale = amax/448; q = fp8(x/scale)
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
quant_fp8_rowwise_kernel(const ushort* __restrict__ x, unsigned char* __restrict__ q,
                         float* __restrict__ scales, int K) {
  const long long base = (long long)blockIdx.x * K;
  float amax = 0.f;
  const int nvec = K / 8;
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(x + base + i * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(bf2f(v.v[j])));
  }
  __shared__ float sm[4];
  float wmax = wave_reduce_max(amax);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x / 64] = wmax;
  __syncthreads();
  const float total = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  const float scale = (total > 0.f) ? total / 448.f : 1.f;
  const float inv = 1.f / scale;
  if (threadIdx.x == 0) scales[blockIdx.x] = scale;
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(x + base + i * 8);
    unsigned int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v.v[0]) * inv, bf2f(v.v[1]) * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v.v[2]) * inv, bf2f(v.v[3]) * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v.v[4]) * inv, bf2f(v.v[5]) * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v.v[6]) * inv, bf2f(v.v[7]) * inv, hi, true);
    uint2 out = {lo, hi};
    *reinterpret_cast<uint2*>(q + base + i * 8) = out;
  }
}

// ---------------------------------------------------------------------------
// fp8 GEMM: C[M,N] = (A_q[M,K] @ B_q[N,K]^T) * a_s[m] * b_s[n], bf16 out.
// 128x128 tile, 4 waves (2x2), glds double buffer, one barrier per K-tile.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256, 2)
gemm_bt_fp8_kernel(const unsigned char* __restrict__ A, const float* __restrict__ a_s,
                   const unsigned char* __restrict__ B, const float* __restrict__ b_s,
                   ushort* __restrict__ C, int M, int N, int K) {
  const int nwg = (M / 128) * (N / 128);
  const int wgid = xcd_remap(blockIdx.x, nwg);
  const int tiles_n = N / 128;
  const int tile_m = wgid / tiles_n;
  const int tile_n = wgid % tiles_n;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1;
  const int wn = wid & 1;

  __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][128 * FBK];

  const unsigned char* Atile = A + (long long)tile_m * 128 * K;
  const unsigned char* Btile = B + (long long)tile_n * 128 * K;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int m_base = wm * 64;
  const int n_base = wn * 64;
  const int frag_row = lane & 15;
  const int frag_kgrp = lane >> 4;

  const int ntiles = K / FBK;
  stage_tile_glds<256>(Atile, K, lds[0][0], tid);
  stage_tile_glds<256>(Btile, K, lds[0][1], tid);
  __syncthreads();

  int buf = 0;
  for (int t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) {
      stage_tile_glds<256>(Atile + (long long)(t + 1) * FBK, K, lds[buf ^ 1][0], tid);
      stage_tile_glds<256>(Btile + (long long)(t + 1) * FBK, K, lds[buf ^ 1][1], tid);
    }
    const unsigned char* Al = lds[buf][0];
    const unsigned char* Bl = lds[buf][1];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {  // FBK=128 in 4 MFMA steps of K=32
      long af[4], bf[4];
      const int boff = kk * 32 + frag_kgrp * 8;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        af[mi] = read_fp8_frag(Al, m_base + mi * 16 + frag_row, boff);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        bf[ni] = read_fp8_frag(Bl, n_base + ni * 16 + frag_row, boff);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
              af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    buf ^= 1;
  }

  const long long c_row0 = (long long)tile_m * 128 + m_base + (lane >> 4) * 4;
  const long long c_col0 = (long long)tile_n * 128 + n_base + (lane & 15);
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long row = c_row0 + mi * 16 + e;
      ushort* crow = C + row * N;
      const float as = a_s[row];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const long long col = c_col0 + ni * 16;
        crow[col] = f2bf(acc[mi][ni][e] * as * b_s[col]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// MX block-scaled fp8 path — the CDNA4 5-PF-class fp8 rate.
// v_mfma_scale_f32_32x32x64_f8f6f4 takes per-lane e8m0 scales covering each
// lane's 32-element K block (HW-fused dequant: D += (A*2^sa)@(B*2^sb)), so
// the epilogue needs NO rescale.  OCP MX quantization: per 32-element block,
// scale exponent = floor(log2(amax)) - 8 (e4m3 emax), elements saturate at
// +-448.
// ---------------------------------------------------------------------------

// bf16 [rows, K] -> fp8 q[rows, K] + e8m0 scales [rows, K/32]
extern "C" __global__ void __launch_bounds__(256)
quant_mxfp8_kernel(const ushort* __restrict__ x, unsigned char* __restrict__ q,
                   unsigned char* __restrict__ scales, int K) {
  const long long row = blockIdx.x;
  const int nblocks = K / 32;
  for (int blk = threadIdx.x; blk < nblocks; blk += blockDim.x) {
    const ushort* src = x + row * K + blk * 32;
    float v[32];
    float amax = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      bf16x8 w = *reinterpret_cast<const bf16x8*>(src + c * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[c * 8 + j] = bf2f(w.v[j]);
        amax = fmaxf(amax, fabsf(v[c * 8 + j]));
      }
    }
    int e;
    if (amax > 0.f) {
      int ex;
      float m = frexpf(amax, &ex);  // amax = m * 2^ex, m in [0.5, 1)
      e = (ex - 1) - 8;             // floor(log2(amax)) - emax(e4m3)
      // non-saturating: if amax/2^e = m*512 > 448, step one finer
      if (m > 0.875f) e += 1;
    } else {
      e = -127;
    }
    e = max(-127, min(127, e));
    scales[row * nblocks + blk] = (unsigned char)(e + 127);
    const float inv = exp2f((float)(-e));
    unsigned char* dst = q + row * K + blk * 32;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      unsigned w = 0;
      w = __builtin_amdgcn_cvt_pk_fp8_f32(v[c * 4 + 0] * inv, v[c * 4 + 1] * inv, w, false);
      w = __builtin_amdgcn_cvt_pk_fp8_f32(v[c * 4 + 2] * inv, v[c * 4 + 3] * inv, w, true);
      *reinterpret_cast<unsigned*>(dst + c * 4) = w;
    }
  }
}

// C[M,N] = dequant(A_q, A_s) @ dequant(B_q, B_s)^T, bf16 out.
// TILE x TILE tile, BK=128 fp8 bytes, glds double buffer + one
// __syncthreads per K-tile.  TILE = 128: 4 waves (2x2), 64x64 per wave =
// 2x2 frags of 32x32.  TILE = 256: 8 waves (2 m x 4 n), 128x64 per wave =
// 4x2 frags.
//
// Fragment layout (probed empirically, benchmarks/probe_mx.py): per 64-k
// instruction, lane half lhi holds k in [lhi*16, lhi*16+16) u
// [32+lhi*16, 32+lhi*16+16) — 16 bytes from EACH of the two 32-element
// scale blocks — while the per-lane scale register of half lhi supplies
// the e8m0 scale for block lhi.  So the two 16-B chunks a lane reads are
// (kk*4 + lhi) and (kk*4 + lhi + 2) (read_mx_frag in tile_gemm.h), and the
// scale byte is block (t*4 + kk*2 + lhi) of that fragment's row.
template <int TILE>
static __device__ __forceinline__ void gemm_bt_mxfp8_body(
    const unsigned char* __restrict__ A, const unsigned char* __restrict__ As,
    const unsigned char* __restrict__ B, const unsigned char* __restrict__ Bs,
    ushort* __restrict__ C, int M, int N, int K) {
  constexpr int THREADS = 2 * TILE;
  constexpr int MI = TILE / 64;  // 32-row m-fragments per wave
  constexpr int WN = TILE / 64;  // waves along n (2 along m)

  const int nwg = (M / TILE) * (N / TILE);
  const int wgid = xcd_remap(blockIdx.x, nwg);
  const int tiles_n = N / TILE;
  const int tile_m = wgid / tiles_n;
  const int tile_n = wgid % tiles_n;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid / WN;
  const int wn = wid % WN;
  const int l31 = lane & 31;
  const int lhi = lane >> 5;

  __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][TILE * FBK];

  const unsigned char* Atile = A + (long long)tile_m * TILE * K;
  const unsigned char* Btile = B + (long long)tile_n * TILE * K;
  const int sld = K / 32;  // scale row stride

  f32x16 acc[MI][2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int m_base = wm * (TILE / 2);
  const int n_base = wn * 64;

  // scale rows this lane's fragments use (dword = the 4 e8m0 bytes of one
  // 128-deep K-tile); prefetched one tile ahead so the byte extracts in the
  // MFMA loop never wait on global memory
  const unsigned char* As_row[MI];
  const unsigned char* Bs_row[2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
    As_row[i] = As + ((long long)tile_m * TILE + m_base + i * 32 + l31) * sld;
#pragma unroll
  for (int i = 0; i < 2; ++i)
    Bs_row[i] = Bs + ((long long)tile_n * TILE + n_base + i * 32 + l31) * sld;
  unsigned sa_dw[MI], sb_dw[2];
#pragma unroll
  for (int i = 0; i < MI; ++i) sa_dw[i] = *reinterpret_cast<const unsigned*>(As_row[i]);
#pragma unroll
  for (int i = 0; i < 2; ++i) sb_dw[i] = *reinterpret_cast<const unsigned*>(Bs_row[i]);

  const int ntiles = K / FBK;
  stage_tile_glds<THREADS>(Atile, K, lds[0][0], tid);
  stage_tile_glds<THREADS>(Btile, K, lds[0][1], tid);
  __syncthreads();

  int buf = 0;
  for (int t = 0; t < ntiles; ++t) {
    unsigned na[MI], nb[2];
    if (t + 1 < ntiles) {
      stage_tile_glds<THREADS>(Atile + (long long)(t + 1) * FBK, K, lds[buf ^ 1][0], tid);
      stage_tile_glds<THREADS>(Btile + (long long)(t + 1) * FBK, K, lds[buf ^ 1][1], tid);
#pragma unroll
      for (int i = 0; i < MI; ++i) na[i] = *reinterpret_cast<const unsigned*>(As_row[i] + (t + 1) * 4);
#pragma unroll
      for (int i = 0; i < 2; ++i) nb[i] = *reinterpret_cast<const unsigned*>(Bs_row[i] + (t + 1) * 4);
    }
    const unsigned char* Al = lds[buf][0];
    const unsigned char* Bl = lds[buf][1];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {  // FBK=128 in 2 MFMA steps of K=64
      // lane half lhi supplies the scale of block (kk*2 + lhi) of this tile
      const int sh = 8 * (kk * 2 + lhi);
      i32x8 af[MI], bf[2];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        af[mi] = read_mx_frag(Al, m_base + mi * 32 + l31, kk * 4 + lhi);
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        bf[ni] = read_mx_frag(Bl, n_base + ni * 32 + l31, kk * 4 + lhi);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
              af[mi], bf[ni], acc[mi][ni], 0, 0, 0,
              (int)((sa_dw[mi] >> sh) & 0xff), 0, (int)((sb_dw[ni] >> sh) & 0xff));
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    buf ^= 1;
#pragma unroll
    for (int i = 0; i < MI; ++i) sa_dw[i] = na[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) sb_dw[i] = nb[i];
  }

  // C/D 32x32 map: col = lane&31, row = (r&3)+8*(r>>2)+4*(lane>>5)
  const long long c_col0 = (long long)tile_n * TILE + n_base + l31;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long row = (long long)tile_m * TILE + m_base + mi * 32
                            + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      ushort* crow = C + row * N;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        crow[c_col0 + ni * 32] = f2bf(acc[mi][ni][r]);
    }
}

extern "C" __global__ void __launch_bounds__(256, 2)
gemm_bt_mxfp8_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ As,
                     const unsigned char* __restrict__ B, const unsigned char* __restrict__ Bs,
                     ushort* __restrict__ C, int M, int N, int K) {
  gemm_bt_mxfp8_body<128>(A, As, B, Bs, C, M, N, K);
}

// 256x256 tile: raises the MFMA:ds_read ratio from 8:4 to 8:6-per-
// double-the-work (6 frag reads feed 8 scaled MFMAs vs 4 feeding 4) and
// halves barriers per flop; 1 block/CU (acc alone is 128 VGPRs).
extern "C" __global__ void __launch_bounds__(512, 1)
gemm_bt_mxfp8_256_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ As,
                         const unsigned char* __restrict__ B, const unsigned char* __restrict__ Bs,
                         ushort* __restrict__ C, int M, int N, int K) {
  gemm_bt_mxfp8_body<256>(A, As, B, Bs, C, M, N, K);
}
