// Software-pipelined 256x256 bf16 MFMA GEMM for gfx950 (MI355X): the 16-wave
// single-barrier kernel that gemm_bt runs on its small-M 256-tile shapes.
//
//   C[M,N] = A[M,K] @ B[N,K]^T   (both operands K-contiguous, bf16, f32 acc)
//
// It replaces the one-barrier-per-K-tile glds double-buffer whose ~1.0-1.2 PF
// ceiling is the single vmcnt(0)+barrier drain per K-step (measured round 1:
// profiles/r01_pmc_summary.txt — 57% MFMA-busy, stall = the barrier drain).
//
// Structure per 1024-thread block (16 waves as 4M x 4N, wave tile 64x64):
//   - K advances in BK=64 tiles, staged whole by global_load_lds into 32 KiB
//     slots across the WHOLE 160 KiB LDS: A double-buffered (slots 0,1), B in
//     a ring of 3 (slots 2,3,4).
//   - One barrier per K-tile: {kk0 reads | issue A(t+1) | 16 MFMA | kk1 reads
//     | issue B(t+2) | 16 MFMA | counted vmcnt | BAR}.  The B ring gives
//     B(t+2) more than a full tile of flight; the wait at the tile end
//     leaves exactly B(t+2) in flight, and everything the next tile reads has
//     landed before the rendezvous (wait-then-barrier).  Only the last two
//     tiles, with nothing left to prefetch, wait vmcnt(0); raw s_barrier
//     (not __syncthreads) so in-flight DMA crosses barriers.
//   - LDS rows are 128 B (8 chunks of 16 B); chunk c of row r lands at slot
//     (c + 2*((r>>1)&3)) & 7.  The inverse is applied to the global SOURCE
//     address (glds destinations are lane-linear), staying within each row's
//     128 B segment so cacheline coalescing is preserved.
//   - XCD-aware bijective blockIdx remap, then grouped-m order (neighbor
//     tiles share L2 panels).
//
// The other rungs of the round-2 ladder (4-phase k-split bodies, the 8-wave
// 2-phase body, static wave priority, 2 blocks/CU at BK=32, 256x128 tiles)
// were measured in profiles/r02_gemm_pipeline.txt; their code is at commit
// 458d9e7.
//
// Constraints: M % 256 == 0 (host pads), N % 256 == 0, K % 128 == 0.
//
// Prologues and the smallest K.  gemm2ph_wide_body (and the asm kernels
// generated into gemm_asm.hip, which copy its 8-wave predecessor's prologue)
// issues tile 0 in full and part of tile 1, then waits with a COUNTED vmcnt
// sized for exactly the tile-1 loads it issued.  Each issue is skipped when
// its tile does not exist (TGT < ntiles), so with ONE K-tile the tile-1 loads
// would be missing from the count and the wait would let tile-0 loads still
// be in flight at the first barrier.  No body handles that case; all of them
// need ntiles >= 2, and the bindings guarantee it: gemm_bt_8ph_v and the
// 256-tile branch of gemm_bt that reaches v14 / asm4 / asm7 accept only
// K >= 128 with K % 128 == 0, and a K-tile here is PBK = 64, so K = 128 is
// two tiles, never one.
// What has landed at the first barrier at that smallest K, per body:
//   asm4 / asm7 (v21 / v24):   B(0), A(0), B(1) 4 loads each, vmcnt(4):
//                              B(0) and A(0).
//   gemm2ph_wide_body (v14):   2 loads per unit at 1024 threads, vmcnt(2):
//                              B(0) and A(0).
// In the loop the last two tiles wait vmcnt(0) (t >= ntiles - 2), so at
// ntiles == 2 the prologue runs straight into the drain.  K = 128 .. 640 is
// pinned bit for bit by tests/test_gemm_edges_gpu.py for v14, asm4 and asm7.
// gemm_bt_bf16_kernel and gemm_bt_bf16_256_kernel (gemm.hip) drain with
// __syncthreads per tile and take a single tile (K = 64).

#include "common.h"
#include "kernels.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define PBM 256
#define PBN 256
#define PBK 64

// 16-wave (1024-thread) single-barrier body: 4 waves/SIMD, wave tile 64x64
// (4x4 fragments, 64 acc VGPRs) — rendezvous skew hides behind 4-way wave
// interleave on each SIMD.  Staging is 2 glds/thread per 32 KiB unit.
__device__ __forceinline__ void
gemm2ph_wide_body(const ushort* __restrict__ A, const ushort* __restrict__ B,
                  ushort* __restrict__ C, int M, int N, int K) {
  const int nwg = (M / PBM) * (N / PBN);
  int wgid = blockIdx.x;
  {
    const int q = nwg / 8, r = nwg % 8;
    const int xcd = wgid % 8, pos = wgid / 8;
    wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
  }
  const int tiles_n = N / PBN;
  // grouped-m flat order: each XCD's contiguous wgid chunk becomes a
  // GM-row x n 2D block, so its L2 holds GM A-panels + chunk/GM B-panels
  // instead of 1-2 A-panels + a whole row of B-panels.
  const int GM = 8;
  const int tiles_m = M / PBM;
  const int group = wgid / (GM * tiles_n);
  const int rem = wgid % (GM * tiles_n);
  const int g0 = group * GM;
  const int gh = (tiles_m - g0 < GM) ? (tiles_m - g0) : GM;
  const int tile_m = g0 + rem % gh;
  const int tile_n = rem / gh;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;           // 0..15
  const int wm = wid >> 2;            // 0..3 -> 64-row band of A
  const int wn = wid & 3;             // 0..3 -> 64-row band of B
  const int l15 = lane & 15;
  const int kgrp = lane >> 4;

  // 5 x 32 KiB slots = the full 160 KiB: A in 0,1 (dbuf); B ring in 2,3,4
  __shared__ __attribute__((aligned(16))) ushort lds[5][256 * 64];

  const ushort* Atile = A + (long long)tile_m * PBM * K;
  const ushort* Btile = B + (long long)tile_n * PBN * K;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int swz0 = (kgrp + 2 * ((l15 >> 1) & 3)) & 7;
  const int frag0 = l15 * 128 + swz0 * 16;
  const int a_off = wm * 64 * 128 + frag0;
  const int b_off = wn * 64 * 128 + frag0;

  int st_row[2], st_cofs[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int s = i * 1024 + tid;
    const int r = s >> 3;
    const int c = ((s & 7) - 2 * ((r >> 1) & 3)) & 7;
    st_row[i] = r;
    st_cofs[i] = c * 8;
  }
  const int wave_chunk = tid & ~63;

  const int ntiles = K / PBK;

#define ISSUE2W(TGT, OP, SLOT)                                               \
  do {                                                                       \
    if ((TGT) < ntiles) {                                                    \
      const int k0_ = (TGT) * PBK;                                           \
      ushort* dst_ = &lds[(SLOT)][0];                                        \
      _Pragma("unroll") for (int i = 0; i < 2; ++i) {                        \
        const ushort* g = (OP) + (long long)st_row[i] * K + k0_ + st_cofs[i];\
        __builtin_amdgcn_global_load_lds(                                    \
            (const __attribute__((address_space(1))) unsigned int*)g,        \
            (__attribute__((address_space(3))) unsigned int*)(dst_ +         \
                (long long)(i * 1024 + wave_chunk) * 8),                     \
            16, 0, 0);                                                       \
      }                                                                      \
    }                                                                        \
  } while (0)

  // prologue: B(0)->2, A(0)->0, B(1)->3; wait all but B(1)
  ISSUE2W(0, Btile, 2);
  ISSUE2W(0, Atile, 0);
  ISSUE2W(1, Btile, 3);
  asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  __builtin_amdgcn_s_barrier();

#define LOAD_W4(DST, SLOTBASE, OFF, KX)                                      \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) {                            \
    DST[j] = *reinterpret_cast<const short8*>(                               \
        reinterpret_cast<const char*>(&lds[0][0]) + (SLOTBASE) * 32768 +     \
        (((OFF) + j * 2048) ^ ((KX) * 64)));                                 \
  }
#define MFMA16W(KX)                                                         \
  _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                          \
  _Pragma("unroll") for (int ni = 0; ni < 4; ++ni)                          \
      acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                \
          af[mi], bf[ni], acc[mi][ni], 0, 0, 0);

  for (int t = 0; t < ntiles; ++t) {
    const int aslot = t & 1;
    const int bslot = 2 + t % 3;
    const int bslot2 = 2 + (t + 2) % 3;
    short8 af[4], bf[4];
    LOAD_W4(af, aslot, a_off, 0);
    LOAD_W4(bf, bslot, b_off, 0);
    ISSUE2W(t + 1, Atile, aslot ^ 1);
    MFMA16W(0);
    LOAD_W4(af, aslot, a_off, 1);
    LOAD_W4(bf, bslot, b_off, 1);
    ISSUE2W(t + 2, Btile, bslot2);
    MFMA16W(1);
    if (t >= ntiles - 2)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
#undef MFMA16W
#undef LOAD_W4
#undef ISSUE2W

  const long long c_row0 = (long long)tile_m * PBM + wm * 64 + (lane >> 4) * 4;
  const long long c_col0 = (long long)tile_n * PBN + wn * 64 + l15;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long row = c_row0 + mi * 16 + e;
      ushort* crow = C + row * N;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        crow[c_col0 + ni * 16] = f2bf(acc[mi][ni][e]);
    }
  }
}

extern "C" __global__ void __launch_bounds__(1024, 4)
gemm_bt_bf16_8ph_v14_kernel(const ushort* __restrict__ A, const ushort* __restrict__ B,
                            ushort* __restrict__ C, int M, int N, int K) {
  gemm2ph_wide_body(A, B, C, M, N, K);
}
