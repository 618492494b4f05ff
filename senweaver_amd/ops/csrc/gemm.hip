// bf16 MFMA GEMM for gfx950 (MI355X): C[M,N] = A[M,K] @ B[N,K]^T
//
// This is the backbone projection GEMM (Llama weights are stored
// [out_features, in_features], so both operands are K-contiguous — the
// "B^T input" form whose fragments are plain 16-byte row loads).
//
// Structure (the CDNA4 guide's "step-3" LDS-staged design):
//   - 128x128 output tile per 256-thread block (4 waves, 2x2; each wave owns
//     a 64x64 quadrant = 4x4 fragments of v_mfma_f32_16x16x32_bf16)
//   - K-loop in BK=64 steps; A-tile and B-tile (16 KiB each) staged by
//     global_load_lds_dwordx4 (direct HBM->LDS DMA, 16 B/lane), double
//     buffered; one __syncthreads per K-step (its vmcnt(0) drains the DMA)
//   - LDS XOR swizzle (chunk ^= row&7) applied on the *source* address and
//     the ds_read address (glds writes lane-linear, so the swizzle cannot go
//     on the LDS destination) — keeps ds_read_b128 bank conflicts <=2-way
//   - XCD-aware bijective blockIdx remap so neighboring tiles (sharing A/B
//     panels) land on the same XCD's L2 (8 XCDs with private 4 MiB L2s)
//
// f32 accumulation in AGPRs; bf16 output.  M,N % 128 == 0, K % 64 == 0
// (host wrapper pads M; Llama-3 dims satisfy N,K natively).
//
// The pipeline itself (staging, swizzled reads, K loop, epilogue) is
// gemm_bt_bf16_body in tile_gemm.h, shared with the grouped GEMM of moe.hip.

#include "common.h"
#include "kernels.h"
#include "tile_gemm.h"

// dense tile: XCD remap of the flat block id, then the shared body
template <int TILE>
static __device__ __forceinline__ void gemm_bt_bf16_dense(
    const ushort* __restrict__ A, const ushort* __restrict__ B,
    ushort* __restrict__ C, int M, int N, int K) {
  const int nwg = (M / TILE) * (N / TILE);
  const int wgid = xcd_remap(blockIdx.x, nwg);
  const int tiles_n = N / TILE;
  const int tile_m = wgid / tiles_n;
  const int tile_n = wgid % tiles_n;
  gemm_bt_bf16_body<TILE, false>(A + (long long)tile_m * TILE * K,
                                 B + (long long)tile_n * TILE * K, C,
                                 (long long)tile_m * TILE, (long long)tile_n * TILE,
                                 N, K, 0);
}

extern "C" __global__ void __launch_bounds__(256, 2)
gemm_bt_bf16_kernel(const ushort* __restrict__ A, const ushort* __restrict__ B,
                    ushort* __restrict__ C, int M, int N, int K) {
  gemm_bt_bf16_dense<128>(A, B, C, M, N, K);
}

// ---------------------------------------------------------------------------
// 256x256-tile variant — the "BK=64 top tier" structure from the CDNA4
// guide: 8 waves (2Mx4N, each owning 128x64 = 8x4 fragments), 128 KiB LDS
// (1 block/CU), glds double-buffer, ONE __syncthreads per K-step.  Measured
// class: ~1.15-1.22 PF/s bf16 at 4-8k shapes (vs ~0.9 for the 128^2 tile).
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(512, 1)
gemm_bt_bf16_256_kernel(const ushort* __restrict__ A, const ushort* __restrict__ B,
                        ushort* __restrict__ C, int M, int N, int K) {
  gemm_bt_bf16_dense<256>(A, B, C, M, N, K);
}

// ---------------------------------------------------------------------------
// Decode GEMV: M <= 16 (beam decode).  One WAVE per output row n, lanes
// stride K (coalesced 16 B/lane row reads — the previous row-per-lane form
// was ~4x off the bandwidth bound), f32 accumulation, one wave reduction
// per (m, n) at the end.  N/4 blocks fill the chip without split-K, so the
// partial-reduce pass is gone too.  A (M x K, <=128 KiB) streams from L2.
// ---------------------------------------------------------------------------
template <int MM>
static __device__ __forceinline__ void gemv2_body(
    const ushort* A, const ushort* B, ushort* C, int M, int N, int K) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wid;
  if (n >= N) return;
  const ushort* brow = B + (long long)n * K;
  float acc[MM];
#pragma unroll
  for (int m = 0; m < MM; ++m) acc[m] = 0.f;
  // 2-deep software pipeline: the runtime-K loop otherwise keeps ONE
  // weight load in flight per lane (latency-bound on the small rows)
  short8 cur_ = __builtin_nontemporal_load(
      reinterpret_cast<const short8*>(brow + lane * 8));
  for (int k = lane * 8; k < K; k += 64 * 8) {
    short8 nxt_;
    if (k + 64 * 8 < K)
      nxt_ = __builtin_nontemporal_load(
          reinterpret_cast<const short8*>(brow + k + 64 * 8));
    bf16x8 bv = *reinterpret_cast<const bf16x8*>(&cur_);
    float bfv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bfv[j] = bf2f(bv.v[j]);
#pragma unroll
    for (int m = 0; m < MM; ++m) {
      bf16x8 av = *reinterpret_cast<const bf16x8*>(A + (long long)m * K + k);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s += bf2f(av.v[j]) * bfv[j];
      acc[m] += s;
    }
    cur_ = nxt_;
  }
#pragma unroll
  for (int m = 0; m < MM; ++m) {
    float v = wave_reduce_sum(acc[m]);
    if (lane == 0 && m < M) C[(long long)m * N + n] = f2bf(v);
  }
}

// concrete instantiations with C linkage for the bindings TU
#define GEMV2_INST(MM)                                                        \
  extern "C" __global__ void __launch_bounds__(256)                           \
  gemv_bt_bf16_v2_m##MM(const ushort* A, const ushort* B, ushort* C, int M,   \
                        int N, int K) {                                       \
    gemv2_body<MM>(A, B, C, M, N, K);                                         \
  }

// ---------------------------------------------------------------------------
// Decode GEMV v3 — loader/consumer LDS-DMA streaming engine (M = 1).
// The v2 form (one wave per row, 2-deep nt register pipeline) measures ~85%
// of the achievable HBM rate: its in-flight requests are single 1 KiB row
// chunks scattered across many DRAM pages.  The microarch price list
// (ldsdma-fill / nt-weights rows) measures 6.5-6.8 TB/s chip-wide when each
// CU streams CONTIGUOUS fills via global_load_lds with nt.  Here a block
// owns 8 consecutive output rows and walks K in 512-element chunks:
// slot = 8 rows x 1 KiB = 8 KiB in an LDS ring, wave 3 is loader AND
// consumer, each of the 4 waves owns 2 of the 8 rows (64 lanes x 8 elems
// per row per slot), x is staged to LDS once up front; counted
// s_waitcnt vmcnt(8*slots in flight) before each barrier (wait-then-barrier).
//
// The first form, gemv3_body (one slot per barrier, never launched since), is
// in this file at commit 6c7e738.
// gemv3_body2 (two slots per barrier, ring of 6) serves every launched
// kernel — gemv_bt_bf16_v3_m1 (K <= 4096), gemv_bt_bf16_v3w_m1 and
// swiglu_gemv_bt_bf16_m1 (K <= 14336).  Constraints: M == 1,
// K % 1024 == 0 and K >= 1024 (a step is 1024 elements: an odd slot count
// would lose the last slot, and the prologue fetches step 0 unconditionally),
// K <= XCAP, N % 8 == 0 (grid N/8, every block reads 8 full rows).
// ---------------------------------------------------------------------------
#define GV3_KW 512         /* chunk elems per row per slot */

// two slots per barrier round: the 1-slot cadence measured ~0.7 us/slot
// against a 0.32 us fill (barrier+loader-wait dominated); pairing slots
// halves the sync cost per byte.  Ring 6 (steps in flight: consuming,
// landed, in-flight = 3 steps x 2 slots).  Needs nslots even (K % 1024).
template <int XCAP, int FUSE_SWIGLU = 0>
static __device__ __forceinline__ void gemv3_body2(
    const ushort* __restrict__ A, const ushort* __restrict__ B,
    ushort* __restrict__ C, int N, int K) {
  const int n0 = blockIdx.x * 8;
  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;

  __shared__ __attribute__((aligned(16))) ushort gv3_smem[6 * 8 * GV3_KW + XCAP];
  ushort* slots = gv3_smem;
  ushort* x_lds = gv3_smem + 6 * 8 * GV3_KW;

  const int nsteps = K / (2 * GV3_KW);

#define GV3_ISSUE_STEP(ST)                                                    \
  do {                                                                        \
    const ushort* s0_ = B + (long long)n0 * K + (long long)(ST) * 2 * GV3_KW; \
    ushort* d0_ = slots + (((ST) * 2) % 6) * 8 * GV3_KW;                      \
    _Pragma("unroll") for (int r = 0; r < 8; ++r) {                           \
      __builtin_amdgcn_global_load_lds(                                       \
          (const __attribute__((address_space(1))) unsigned int*)             \
              (s0_ + (long long)r * K + lane * 8),                            \
          (__attribute__((address_space(3))) unsigned int*)                   \
              (d0_ + r * GV3_KW + lane * 8),                                  \
          16, 0, 2);                                                          \
      __builtin_amdgcn_global_load_lds(                                       \
          (const __attribute__((address_space(1))) unsigned int*)             \
              (s0_ + (long long)r * K + GV3_KW + lane * 8),                   \
          (__attribute__((address_space(3))) unsigned int*)                   \
              (d0_ + 8 * GV3_KW + r * GV3_KW + lane * 8),                     \
          16, 0, 2);                                                          \
    }                                                                         \
  } while (0)

  if (wid < 3) {
    if (FUSE_SWIGLU) {
      // x = silu(g) * u computed on the way in: A = gateup [1, 2K],
      // g = A[0..K), u = A[K..2K) — replaces the standalone swiglu
      // kernel (one ~5 us launch per decode layer)
      for (int c = wid; c < K / GV3_KW; c += 3) {
        bf16x8 g = *reinterpret_cast<const bf16x8*>(
            A + (long long)c * GV3_KW + lane * 8);
        bf16x8 u = *reinterpret_cast<const bf16x8*>(
            A + (long long)K + (long long)c * GV3_KW + lane * 8);
        bf16x8 out;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float gf = bf2f(g.v[e]);
          out.v[e] = f2bf(gf / (1.f + __expf(-gf)) * bf2f(u.v[e]));
        }
        *reinterpret_cast<bf16x8*>(x_lds + (long long)c * GV3_KW + lane * 8) =
            out;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // writes visible
    } else {
      for (int c = wid; c < K / GV3_KW; c += 3)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)
                (A + (long long)c * GV3_KW + lane * 8),
            (__attribute__((address_space(3))) unsigned int*)
                (x_lds + (long long)c * GV3_KW + lane * 8),
            16, 0, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  } else {
    GV3_ISSUE_STEP(0);
    if (1 < nsteps) {
      GV3_ISSUE_STEP(1);
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __builtin_amdgcn_s_barrier();

  float acc0 = 0.f, acc1 = 0.f;
  const int r0 = wid * 2;
  for (int st = 0; st < nsteps; ++st) {
    const ushort* slot0 = slots + ((st * 2) % 6) * 8 * GV3_KW;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const ushort* slot = slot0 + h * 8 * GV3_KW;
      bf16x8 xv = *reinterpret_cast<const bf16x8*>(
          x_lds + ((long long)st * 2 + h) * GV3_KW + lane * 8);
      bf16x8 w0 = *reinterpret_cast<const bf16x8*>(slot + r0 * GV3_KW + lane * 8);
      bf16x8 w1 = *reinterpret_cast<const bf16x8*>(slot + (r0 + 1) * GV3_KW + lane * 8);
      float xf[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) xf[e] = bf2f(xv.v[e]);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc0 += bf2f(w0.v[e]) * xf[e];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc1 += bf2f(w1.v[e]) * xf[e];
    }
    if (wid == 3) {
      const int nxt = st + 2;
      if (nxt < nsteps) {
        GV3_ISSUE_STEP(nxt);
        // outstanding: step st+1 (16, oldest) + step st+2 (16)
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      } else if (st + 1 < nsteps) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
#undef GV3_ISSUE_STEP

  acc0 = wave_reduce_sum(acc0);
  acc1 = wave_reduce_sum(acc1);
  if (lane == 0 && n0 + r0 < N) C[n0 + r0] = f2bf(acc0);
  if (lane == 0 && n0 + r0 + 1 < N) C[n0 + r0 + 1] = f2bf(acc1);
}

extern "C" __global__ void __launch_bounds__(256)
gemv_bt_bf16_v3_m1(const ushort* __restrict__ A, const ushort* __restrict__ B,
                   ushort* __restrict__ C, int M, int N, int K) {
  // 56 KiB LDS -> two blocks/CU; two slots per barrier round
  gemv3_body2<4096>(A, B, C, N, K);
}

extern "C" __global__ void __launch_bounds__(256)
gemv_bt_bf16_v3w_m1(const ushort* __restrict__ A, const ushort* __restrict__ B,
                    ushort* __restrict__ C, int M, int N, int K) {
  // wide-K (down-proj): 76 KiB LDS -> one block/CU
  gemv3_body2<14336>(A, B, C, N, K);
}

extern "C" __global__ void __launch_bounds__(256)
swiglu_gemv_bt_bf16_m1(const ushort* __restrict__ GU,
                       const ushort* __restrict__ B,
                       ushort* __restrict__ C, int M, int N, int K) {
  // fused silu(g)*u + down-proj GEMV (decode): GU = gateup [1, 2K]
  gemv3_body2<14336, 1>(GU, B, C, N, K);
}

// ---------------------------------------------------------------------------
// fp8-weight GEMV (decode, M = 1): W rows stored OCP e4m3 with a per-row
// f32 scale (the model's existing fp8 weight format); x stays bf16 — no
// per-step activation quant kernel and no M-pad through the 128-tile fp8
// GEMM (which measured 101 tok/s vs 267 bf16 in decode).  Weight bytes
// halve, and decode GEMV is weight-bandwidth-bound.
// One wave per output row; 16 fp8 bytes per lane per iter via
// v_cvt_pk_f32_fp8 pairs; K % 1024 == 0.
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(4))) unsigned uint4_t;

// TWO rows per wave: fp8 rows are half the bytes of bf16 rows, so a
// K=4096 row is only 4 pipeline iterations — latency-bound with one
// row's 2-deep pipeline.  Two interleaved rows double the in-flight
// loads at the same depth.
template <int MM, int R>  // R rows per wave (R=2 for batched: doubles
                           // in-flight loads on the short fp8 rows; R=1
                           // keeps the M=1 path's measured 332 tok/s)
static __device__ __forceinline__ void gemv_fp8w_body(
    const ushort* __restrict__ X, const unsigned char* __restrict__ Bq,
    const float* __restrict__ Bs, ushort* __restrict__ C, int M, int N,
    int K) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int n = (blockIdx.x * 4 + wid) * R;
  if (n >= N) return;
  const unsigned char* brow0 = Bq + (long long)n * K;
  const unsigned char* brow1 = brow0 + (R > 1 ? K : 0);
  float acc[MM][R];
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
  uint4_t cur0 = __builtin_nontemporal_load(
      reinterpret_cast<const uint4_t*>(brow0 + lane * 16));
  uint4_t cur1 = {};
  if (R > 1)
    cur1 = __builtin_nontemporal_load(
        reinterpret_cast<const uint4_t*>(brow1 + lane * 16));
  for (int k = lane * 16; k < K; k += 64 * 16) {
    uint4_t nxt0, nxt1;
    if (k + 64 * 16 < K) {
      nxt0 = __builtin_nontemporal_load(
          reinterpret_cast<const uint4_t*>(brow0 + k + 64 * 16));
      if (R > 1)
        nxt1 = __builtin_nontemporal_load(
            reinterpret_cast<const uint4_t*>(brow1 + k + 64 * 16));
    }
    float wf0[16], wf1[16];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      f32x2_t lo0 = __builtin_amdgcn_cvt_pk_f32_fp8(cur0[d], false);
      f32x2_t hi0 = __builtin_amdgcn_cvt_pk_f32_fp8(cur0[d], true);
      wf0[d * 4 + 0] = lo0[0]; wf0[d * 4 + 1] = lo0[1];
      wf0[d * 4 + 2] = hi0[0]; wf0[d * 4 + 3] = hi0[1];
      if (R > 1) {
        f32x2_t lo1 = __builtin_amdgcn_cvt_pk_f32_fp8(cur1[d], false);
        f32x2_t hi1 = __builtin_amdgcn_cvt_pk_f32_fp8(cur1[d], true);
        wf1[d * 4 + 0] = lo1[0]; wf1[d * 4 + 1] = lo1[1];
        wf1[d * 4 + 2] = hi1[0]; wf1[d * 4 + 3] = hi1[1];
      }
    }
#pragma unroll
    for (int m = 0; m < MM; ++m) {
      bf16x8 x0 = *reinterpret_cast<const bf16x8*>(X + (long long)m * K + k);
      bf16x8 x1 = *reinterpret_cast<const bf16x8*>(X + (long long)m * K + k + 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xf = bf2f(x0.v[e]);
        acc[m][0] += wf0[e] * xf;
        if (R > 1) acc[m][1] += wf1[e] * xf;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xf = bf2f(x1.v[e]);
        acc[m][0] += wf0[8 + e] * xf;
        if (R > 1) acc[m][1] += wf1[8 + e] * xf;
      }
    }
    cur0 = nxt0;
    if (R > 1) cur1 = nxt1;
  }
#pragma unroll
  for (int m = 0; m < MM; ++m) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float v = wave_reduce_sum(acc[m][r]);
      if (lane == 0 && m < M && n + r < N)
        C[(long long)m * N + n + r] = f2bf(v * Bs[n + r]);
    }
  }
}

// mxfp8-weight variant: e8m0 per-32-block scales.  A lane's 16 elems per
// iter never straddle a 32-block (k % 16 == 0), so ONE scale byte per lane
// per iter: wf *= 2^(s-127) via ldexpf on the per-iter partial: the scale is
// folded per-iter partial sum (s is block-constant).
template <int MM>
static __device__ __forceinline__ void gemv_mxfp8w_body(
    const ushort* __restrict__ X, const unsigned char* __restrict__ Bq,
    const unsigned char* __restrict__ Bs, ushort* __restrict__ C, int M,
    int N, int K) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wid;
  if (n >= N) return;
  const unsigned char* brow = Bq + (long long)n * K;
  const unsigned char* srow = Bs + (long long)n * (K / 32);
  float acc[MM];
#pragma unroll
  for (int m = 0; m < MM; ++m) acc[m] = 0.f;
  uint4_t cur = __builtin_nontemporal_load(
      reinterpret_cast<const uint4_t*>(brow + lane * 16));
  for (int k = lane * 16; k < K; k += 64 * 16) {
    uint4_t nxt;
    if (k + 64 * 16 < K)
      nxt = __builtin_nontemporal_load(
          reinterpret_cast<const uint4_t*>(brow + k + 64 * 16));
    const float scale = exp2f((float)srow[k / 32] - 127.f);
    float wf[16];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(cur[d], false);
      f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8(cur[d], true);
      wf[d * 4 + 0] = lo[0];
      wf[d * 4 + 1] = lo[1];
      wf[d * 4 + 2] = hi[0];
      wf[d * 4 + 3] = hi[1];
    }
#pragma unroll
    for (int m = 0; m < MM; ++m) {
      bf16x8 x0 = *reinterpret_cast<const bf16x8*>(X + (long long)m * K + k);
      bf16x8 x1 = *reinterpret_cast<const bf16x8*>(X + (long long)m * K + k + 8);
      float part = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) part += wf[e] * bf2f(x0.v[e]);
#pragma unroll
      for (int e = 0; e < 8; ++e) part += wf[8 + e] * bf2f(x1.v[e]);
      acc[m] += part * scale;
    }
    cur = nxt;
  }
#pragma unroll
  for (int m = 0; m < MM; ++m) {
    const float v = wave_reduce_sum(acc[m]);
    if (lane == 0 && m < M) C[(long long)m * N + n] = f2bf(v);
  }
}

#define GEMV_MXFP8W_INST(MM)                                                  \
  extern "C" __global__ void __launch_bounds__(256)                           \
  gemv_bt_mxfp8w_m##MM(const ushort* X, const unsigned char* Bq,              \
                       const unsigned char* Bs, ushort* C, int M, int N,      \
                       int K) {                                               \
    gemv_mxfp8w_body<MM>(X, Bq, Bs, C, M, N, K);                              \
  }

GEMV_MXFP8W_INST(1)
GEMV_MXFP8W_INST(2)
GEMV_MXFP8W_INST(4)
GEMV_MXFP8W_INST(8)

#define GEMV_FP8W_INST(MM)                                                    \
  extern "C" __global__ void __launch_bounds__(256)                           \
  gemv_bt_fp8w_m##MM(const ushort* X, const unsigned char* Bq,                \
                     const float* Bs, ushort* C, int M, int N, int K) {       \
    gemv_fp8w_body<MM, (MM > 1 ? 2 : 1)>(X, Bq, Bs, C, M, N, K);              \
  }

GEMV_FP8W_INST(1)
GEMV_FP8W_INST(2)
GEMV_FP8W_INST(4)
GEMV_FP8W_INST(8)

GEMV2_INST(1)
GEMV2_INST(2)
GEMV2_INST(4)
GEMV2_INST(8)
GEMV2_INST(16)

// ---------------------------------------------------------------------------
// Decode fused residual-add + RMSNorm + GEMV:
//   t[m] = x[m] (+ res_in[m]);  C[m][n] = (sum_k t*normw*B[n]) * rsqrt(ss/K+eps)
// RMSNorm is a per-row LINEAR scale, so the raw dot and the sum of squares
// accumulate in the SAME k-pass and the scale applies after the wave
// reduction — one kernel replaces (fused_add_rmsnorm + gemv), two of the
// ~5 us launches per decode layer.  Block 0 additionally writes
// res_out[m] = t[m] (a separate buffer: no cross-block write/read race).
//
// Still a macro, unlike the other GEMVs: as a template body the m16 instance
// rounds differently.  A device function is optimised before it is inlined,
// without the kernel's __launch_bounds__, so only one of dot[16] / ss[16] is
// promoted to a vector there; the loop then vectorises differently and the
// backend fuses 105 of its mul+add pairs into fma that are separate here.
// ---------------------------------------------------------------------------
#define GEMV_NORM_INST(MM)                                                   \
  extern "C" __global__ void __launch_bounds__(256)                           \
  gemv_norm_bt_bf16_m##MM(const ushort* x, const ushort* res_in,              \
                          const ushort* normw, const ushort* B, ushort* C,    \
                          ushort* res_out, int M, int N, int K, float eps) {  \
    const int wid = threadIdx.x >> 6;                                         \
    const int lane = threadIdx.x & 63;                                        \
    const int n = blockIdx.x * 4 + wid;                                       \
    if (n >= N) return;                                                       \
    const ushort* brow = B + (long long)n * K;                                \
    float dot[MM], ss[MM];                                                    \
    _Pragma("unroll") for (int m = 0; m < MM; ++m) { dot[m] = 0.f; ss[m] = 0.f; } \
    for (int k = lane * 8; k < K; k += 64 * 8) {                              \
      short8 bv_ = __builtin_nontemporal_load(                                \
          reinterpret_cast<const short8*>(brow + k));                         \
      bf16x8 bv = *reinterpret_cast<const bf16x8*>(&bv_);                     \
      bf16x8 wv = *reinterpret_cast<const bf16x8*>(normw + k);                \
      float bw[8];                                                            \
      _Pragma("unroll") for (int j = 0; j < 8; ++j)                           \
          bw[j] = bf2f(bv.v[j]) * bf2f(wv.v[j]);                              \
      _Pragma("unroll") for (int m = 0; m < MM; ++m) {                        \
        bf16x8 av = *reinterpret_cast<const bf16x8*>(x + (long long)m * K + k); \
        float t[8];                                                           \
        if (res_in != nullptr) {                                              \
          bf16x8 rv = *reinterpret_cast<const bf16x8*>(res_in + (long long)m * K + k); \
          _Pragma("unroll") for (int j = 0; j < 8; ++j)                       \
              t[j] = bf2f(av.v[j]) + bf2f(rv.v[j]);                           \
        } else {                                                              \
          _Pragma("unroll") for (int j = 0; j < 8; ++j) t[j] = bf2f(av.v[j]); \
        }                                                                     \
        float d = 0.f, s2 = 0.f;                                              \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) {                       \
          d += t[j] * bw[j];                                                  \
          s2 += t[j] * t[j];                                                  \
        }                                                                     \
        dot[m] += d;                                                          \
        ss[m] += s2;                                                          \
      }                                                                       \
    }                                                                         \
    _Pragma("unroll") for (int m = 0; m < MM; ++m) {                          \
      float d = wave_reduce_sum(dot[m]);                                      \
      float s2 = wave_reduce_sum(ss[m]);                                      \
      if (lane == 0 && m < M)                                                 \
        C[(long long)m * N + n] = f2bf(d * rsqrtf(s2 / (float)K + eps));      \
    }                                                                         \
    if (blockIdx.x == 0) {                                                    \
      /* waves stride rows; lanes stride k: res_out = t (vectorized) */       \
      for (int m = wid; m < M; m += 4) {                                      \
        for (int k = lane * 8; k < K; k += 64 * 8) {                          \
          bf16x8 av = *reinterpret_cast<const bf16x8*>(x + (long long)m * K + k); \
          bf16x8 o;                                                           \
          if (res_in != nullptr) {                                            \
            bf16x8 rv = *reinterpret_cast<const bf16x8*>(res_in + (long long)m * K + k); \
            _Pragma("unroll") for (int j = 0; j < 8; ++j)                     \
                o.v[j] = f2bf(bf2f(av.v[j]) + bf2f(rv.v[j]));                 \
          } else {                                                            \
            o = av;                                                           \
          }                                                                   \
          *reinterpret_cast<bf16x8*>(res_out + (long long)m * K + k) = o;     \
        }                                                                     \
      }                                                                       \
    }                                                                         \
  }

GEMV_NORM_INST(1)
GEMV_NORM_INST(2)
GEMV_NORM_INST(4)
GEMV_NORM_INST(8)
GEMV_NORM_INST(16)
