// Flash attention forward v5 (gfx950): the production causal prefill kernel.
// D = 128, GQA, bf16 in, fp32 accumulate; 512 threads = 8 waves per block,
// each wave owns 32 query rows (256 per block) and all waves share one staged
// K / V^T tile of 64 keys.  QK^T is computed swapped (S^T = K Q^T), so a lane
// holds one query row's scores and the row max / sum need one cross-half
// shuffle instead of a reduction.  On top of that structure:
//
//   register-staged double buffer   the next tile's K and V^T are loaded to
//       VGPRs right after QK (K rows consumed, HBM latency hidden behind the
//       softmax) and written to the idle LDS buffer just before PV: one
//       barrier per tile and a short register lifetime.
//   defer-max   while every lane's tile max stays within 11.54 (= 8 / ln 2,
//       the exp2 domain) of its running max, the running max is kept and the
//       O rescale is skipped; P stays bounded by e^8.
//   VALU diet   log2(e) is folded into the scale so exp is a bare v_exp_f32,
//       max is a bare v_max_f32, and tiles entirely below the diagonal skip
//       the causal mask.
//   sm-split    exp, bf16 pack and the PV MFMAs run per group of 16 keys, so
//       the softmax VALU work of one group overlaps the MFMAs of the last.
//   PACK 0/1/2  0 stores O^T [B,H,D,S]; 1 and 2 are prefix-packed prefill
//       (see attn5_body).
//
// This is variant 15 of the v4 probe ladder (glds prefetch placements,
// single-buffer staging, 2-tiles-ahead rings, 4-wave blocks, an LDS-transposed
// epilogue, a persistent grid).  The measurements are in
// profiles/r02_attn_ladder.txt, under that name; the losers' code can be read
// at commit ee4d66d (attention_v4.hip).
// Numerics are asserted against the fp32 torch reference in
// tests/test_kernels_gpu.py and tests/test_prefill_edges_gpu.py.

#include "common.h"
#include "kernels.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define V5_KVBLK 64
#define V5_QBLK 256
#define V5_NT 512
#define V5_CHUNKS (V5_KVBLK * 16)      // 16-byte chunks in a K tile, and in a V^T tile
#define V5_KC (V5_CHUNKS / V5_NT)      // of which each thread moves this many

// A K tile is 64 keys x 128 d (16 chunks per row), a V^T tile 128 d x 64 keys
// (8 chunks per row).  In LDS, chunk cl of row r sits at physical chunk
// (cl ^ r) & (chunks_per_row - 1) of that row: conflict-free for the MFMA
// operand reads.  Tiles are written to LDS linearly (thread t fills slot t,
// t + 512, ..), so the swizzle is applied on the global side: v5_src is the
// source of the chunk that belongs in slot row * chunks_per_row + cl.
//
// The callers split a slot into (row, cl) themselves, where the slot is a
// thread id of known range and chunks_per_row a literal.  With s / cpr and
// s % cpr inside a helper the compiler narrows them to 16 bits before it
// inlines, and every kernel of this file comes out 7 instructions longer with
// another register assignment (probably the build that commit ee4d66d
// measured 2 % slower at S 2048).
static __device__ __forceinline__ const ushort* v5_src(
    const ushort* __restrict__ src, long long ld, int chunks_per_row, int row,
    int cl) {
  const int c = (cl ^ row) & (chunks_per_row - 1);
  return src + (long long)row * ld + c * 8;
}

// global -> LDS without a register round trip (prologue); lds_wave is the
// wave-uniform slot of the wave's first lane
static __device__ __forceinline__ void v5_glds(const ushort* g,
                                               ushort* lds_wave) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) unsigned int*)g,
      (__attribute__((address_space(3))) unsigned int*)lds_wave, 16, 0, 0);
}

static __device__ __forceinline__ short8 v5_read(const ushort* lds_tile,
                                                 int row, int c,
                                                 int chunks_per_row) {
  const int phys = (c ^ row) & (chunks_per_row - 1);
  return *reinterpret_cast<const short8*>(lds_tile + (row * chunks_per_row + phys) * 8);
}

// Row-major V tile (VROWS): 64 keys x 128 d, plain 256-byte rows.  The
// 16-byte chunk ch of key row r sits at physical chunk ch ^ v5_vx(r): with
// that XOR the transposed 32x32x16 operand read below touches every bank of a
// 32-lane half exactly once.
static __device__ __forceinline__ int v5_vx(int r) {
  return ((r & 3) << 2) | ((r >> 2) & 3);
}

// PV operand from the row-major tile: lane (l31, lhi) gets
// V[kvg + 8*lhi + 0..7][db*32 + l31], what v5_read hands it from a V^T tile.
// ds_read_b64_tr_b16 gathers, per 16 lanes, a block of 4 keys x 16 d and
// gives lane i the 4 keys of column i; lane 4q+p supplies the address of key
// row q, columns 4p .. 4p+3.  Two reads (keys +0..3 and +4..7) make the
// operand.  Every lane of the wave must be active, and every address is a
// multiple of 8 bytes.
static __device__ __forceinline__ short8 v5_read_tr(const ushort* v_lds,
                                                    int lane, int kvg, int db) {
  const int p = lane & 3, q = (lane >> 2) & 3, hh = (lane >> 4) & 1;
  const int lhi = lane >> 5;
  short4v part[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = kvg + 8 * lhi + 4 * j + q;
    const int ch = db * 4 + 2 * hh + (p >> 1);
    const int off = row * 128 + (ch ^ v5_vx(row)) * 8 + 4 * (p & 1);
    part[j] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) short4v*)(v_lds + off));
  }
  return __builtin_shufflevector(part[0], part[1], 0, 1, 2, 3, 4, 5, 6, 7);
}

static __device__ __forceinline__ unsigned v5_cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

static __device__ __forceinline__ float v5_max(float a, float b) {
  // plain v_max_f32: fmaxf on MFMA outputs gets a canonicalising v_max
  // prepended at -O3 — 2 VALU where 1 does
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

static __device__ __forceinline__ float v5_exp2(float x) {
  float r;
  asm("v_exp_f32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

// Block order for a 1-D grid of nqb * H * B blocks.  The hardware deals
// consecutive workgroups round-robin over the 8 XCDs, each with an L2 of its
// own.  The nqb * (H / Hk) blocks of one (batch, kv head) read the same K and
// V, so they all go to one XCD: group g runs on XCD g % 8, and inside an XCD
// the blocks run heaviest first (q block slowest, descending), the heads of a
// group next to each other.  A bijection whenever B * Hk is a multiple of 8;
// otherwise the order of the 3-D grid (q block fastest, descending) is kept.
static __device__ __forceinline__ void attn5_xcd_block(int B, int H, int Hk,
                                                       int nqb, int& qb,
                                                       int& h, int& b) {
  const int i = blockIdx.x;
  const int groups = B * Hk;
  if (groups % 8 == 0) {
    const int rep = H / Hk;
    const int per_rank = (groups / 8) * rep;  // blocks per XCD and q block
    const int j = i / 8;
    const int r = j % per_rank;
    const int g = i % 8 + 8 * (r / rep);
    qb = nqb - 1 - j / per_rank;
    h = (g % Hk) * rep + r % rep;
    b = g / Hk;
  } else {
    qb = nqb - 1 - i % nqb;
    h = (i / nqb) % H;
    b = i / (nqb * H);
  }
}

// PACK (prefix-packed prefill): Q/K/V^T are indexed as usual, but query rows
// below skip[b] belong to the group leader and are not recomputed — a block
// entirely below skip[b] exits before any LDS traffic or barrier, and the
// epilogue stores row q of batch row b to column base[b] + q of ONE 2-D O^T
// [H*D, Tp] (row h*D + d) instead of [B,H,D,S].
// PACK == 2 stores the same values row-major instead, O[Tp, H*D] (packed row
// base[b] + q, column h*D + d), so that o_proj reads an ordinary row-major
// A.  (Staging the rows through LDS for fully coalesced 16-byte stores was
// tried and timed the same, 322.8 against 321.6 us in situ; isolated, both
// layouts run within 1 us of each other.  The plain stores stay.)
//
// VROWS (with PACK): there is no V^T.  VT is the packed qkv GEMM output
// [Tq, ld] itself, and key s of batch row b is the 256 contiguous bytes at
// row packed_src_row(b, s), column v_off + kvh*128.  The tile is staged
// row-major (v5_vx) and the PV operand comes out of ds_read_b64_tr_b16
// (v5_read_tr): the same operands in the same MFMA order, so the same bits.
// A row that a bad plan sends outside [0, Tq) reads row 0 instead.
//
// The VROWS kernel is also the one that got the two scheduling changes below
// (measured with it, profiles/attn_v_rows.txt); the V^T instances keep their
// code as it was.
//
// WSKIP: a wave does no QK^T, softmax or PV for a tile that lies wholly above
// its own 32 query rows (the last three tiles of a block's diagonal, for 2, 4
// and 6 of the 8 waves).  Such a tile has p = 0 everywhere and defer-max
// holds, so it adds +-0 to O and 0 to the row sum: skipping it is exact.  The
// wave still stages its share of the next tile and meets the barrier.
//
// XCD: a 1-D grid, mapped by attn5_xcd_block.
template <int PACK, bool VROWS = false>
static __device__ __forceinline__ void attn5_body(
    const ushort* __restrict__ Q, const ushort* __restrict__ K,
    const ushort* __restrict__ VT, ushort* __restrict__ OT, int B, int H,
    int Hk, int S, float scale, const int* __restrict__ pk_skip = nullptr,
    const int* __restrict__ pk_base = nullptr, int Tp = 0,
    const int* __restrict__ pk_owner = nullptr, long long ld = 0,
    long long v_off = 0, long long Tq = 0) {
  static_assert(!VROWS || PACK == 2, "VROWS reads packed qkv rows");
  constexpr bool WSKIP = VROWS, XCD = VROWS;
  int qb = gridDim.x - 1 - blockIdx.x;  // heaviest-first
  int h = blockIdx.y;
  int b = blockIdx.z;
  if (XCD) attn5_xcd_block(B, H, Hk, (S + V5_QBLK - 1) / V5_QBLK, qb, h, b);
  int skip = 0;
  if (PACK) {
    // block-uniform early-out: every query row of this block is a prefix
    // row the leader already produced
    skip = pk_skip[b];
    if (qb * V5_QBLK + V5_QBLK <= skip) return;
  }
  const int kvh = h / (H / Hk);
  const int D = 128;

  const ushort* Qh = Q + (((long long)b * H + h) * S) * D;
  const ushort* Kh = K + (((long long)b * Hk + kvh) * S) * D;
  const ushort* VTh = VROWS ? VT + v_off + (long long)kvh * D
                             : VT + (((long long)b * Hk + kvh) * D) * S;
  // VROWS: packed_src_row(b, s) is pre0 + s below skip and own0 + s from it
  // on; the block-uniform parts are fetched once
  long long pre0 = 0, own0 = 0;
  if (VROWS) {
    pre0 = packed_src_row(b, 0, B, pk_skip, pk_base, pk_owner);
    own0 = pk_base[b];
  }
  // source of the chunk that belongs in slot s (key row s / 16, physical
  // chunk s % 16) of the V tile that starts at key kv0
  auto v_rows_src = [&](int kv0, int s) -> const ushort* {
    const int r = s >> 4;
    const int key = kv0 + r;
    long long tr = (key < skip ? pre0 : own0) + key;
    if ((key < skip && pre0 < 0) || tr < 0 || tr >= Tq) tr = 0;
    return VTh + tr * ld + ((s & 15) ^ v5_vx(r)) * 8;
  };
  ushort* OTh = OT + (((long long)b * H + h) * D) * S;

  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int l31 = lane & 31;
  const int lhi = lane >> 5;
  const int q0 = qb * V5_QBLK + wid * 32;  // 32 q rows per wave
  const int q_lane = q0 + l31;
  const int q0_wave = qb * V5_QBLK + __builtin_amdgcn_readfirstlane(wid) * 32;
  const bool live = q_lane < S;

  __shared__ __attribute__((aligned(16))) ushort smem[2][V5_KVBLK * 128 + 128 * V5_KVBLK];

  short8 qf[8];
  {
    const long long qrow = (long long)(live ? q_lane : 0) * D;
#pragma unroll
    for (int st = 0; st < 8; ++st)
      qf[st] = *reinterpret_cast<const short8*>(Qh + qrow + st * 16 + lhi * 8);
  }

  float m_run = -INFINITY, l_run = 0.f;
  f32x16 o_acc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[db][r] = 0.f;

  const int kv_end = min(S, qb * V5_QBLK + V5_QBLK);
  // tile 0 goes straight to LDS buffer 0.  With 512 threads the bound never
  // trips, but without it the compiler schedules the whole kernel otherwise,
  // and that schedule has not been measured.
  for (int s0 = 0; s0 < V5_CHUNKS; s0 += V5_NT) {
    const int s = s0 + tid;
    if (s >= V5_CHUNKS) break;
    v5_glds(v5_src(Kh, D, 16, s / 16, s % 16),
            smem[0] + (long long)(s0 + (tid & ~63)) * 8);
  }
  for (int s0 = 0; s0 < V5_CHUNKS; s0 += V5_NT) {
    const int s = s0 + tid;
    if (s >= V5_CHUNKS) break;
    v5_glds(VROWS ? v_rows_src(0, s) : v5_src(VTh, S, 8, s / 8, s % 8),
            smem[0] + V5_KVBLK * 128 + (long long)(s0 + (tid & ~63)) * 8);
  }
  __syncthreads();
  int buf = 0;
  for (int kv0 = 0; kv0 < kv_end; kv0 += V5_KVBLK) {
    const bool more = kv0 + V5_KVBLK < kv_end;
    const ushort* k_lds = smem[buf];
    const ushort* vt_lds = smem[buf] + V5_KVBLK * 128;
    // wave-uniform, and known to the compiler as such: the transposed reads
    // of the waves that do work need all their lanes
    const bool work = !WSKIP || kv0 <= q0_wave + 31;

    f32x16 st[2];
    if (work) {
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int stp = 0; stp < 8; ++stp) {
          short8 kf = v5_read(k_lds, sub * 32 + l31, stp * 2 + lhi, 16);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[stp], acc, 0, 0, 0);
        }
        st[sub] = acc;
      }
      __builtin_amdgcn_s_setprio(0);
    }

    // issue the next tile's loads to registers: the K rows of this tile are
    // consumed, and its V^T stays live in LDS until PV
    short8 stg[2 * V5_KC];
    if (more) {
      const ushort* Kn = Kh + (long long)(kv0 + V5_KVBLK) * D;
      const ushort* VTn = VTh + kv0 + V5_KVBLK;
#pragma unroll
      for (int c = 0; c < V5_KC; ++c) {
        const int s = tid + c * V5_NT;
        stg[c] = *reinterpret_cast<const short8*>(v5_src(Kn, D, 16, s / 16, s % 16));
        stg[V5_KC + c] = *reinterpret_cast<const short8*>(
            VROWS ? v_rows_src(kv0 + V5_KVBLK, s) : v5_src(VTn, S, 8, s / 8, s % 8));
      }
    }

    float vals[32];
    float m_new = m_run, alpha = 1.f;
    if (work) {
      float tile_max = -INFINITY;
      const float scl = scale * 1.44269504f;  // exp2 domain
      const bool interior = kv0 + V5_KVBLK - 1 <= q0;
      if (interior) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float v = st[sub][r] * scl;
            vals[sub * 16 + r] = v;
            tile_max = v5_max(tile_max, v);
          }
      } else {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kv = kv0 + sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            float v = st[sub][r] * scl;
            if (kv > q_lane) v = -INFINITY;
            vals[sub * 16 + r] = v;
            tile_max = v5_max(tile_max, v);
          }
      }
      tile_max = v5_max(tile_max, __shfl_xor(tile_max, 32, 64));
      // wave-uniform: every lane's tile max within the threshold of its running
      // max (first tile: m_run = -inf makes the difference +inf -> no defer)
      const bool defer = __all((int)(tile_max - m_run <= 11.54f));
      if (!defer) {
        m_new = fmaxf(m_run, tile_max);
        alpha = (m_run == -INFINITY) ? 0.f : v5_exp2(m_run - m_new);
      }
      m_run = m_new;
      if (!defer) {
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) o_acc[db][r] *= alpha;
      }
    }

    // park the fetched tile in the idle buffer before PV (waits the loads
    // here; QK+softmax has been covering the HBM latency)
    if (more) {
      ushort* kd = smem[buf ^ 1];
      ushort* vd = smem[buf ^ 1] + V5_KVBLK * 128;
#pragma unroll
      for (int c = 0; c < V5_KC; ++c) {
        *reinterpret_cast<short8*>(kd + (long long)(tid + c * V5_NT) * 8) = stg[c];
        *reinterpret_cast<short8*>(vd + (long long)(tid + c * V5_NT) * 8) = stg[V5_KC + c];
      }
    }

    if (work) {
      float rsum = 0.f;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          const int base = sub * 16 + g * 8;
          float p[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            p[i] = v5_exp2(vals[base + i] - m_new);
            rsum += p[i];
          }
          unsigned x0 = v5_cvt_pk_bf16(p[0], p[1]);
          unsigned y0 = v5_cvt_pk_bf16(p[4], p[5]);
          unsigned x1 = v5_cvt_pk_bf16(p[2], p[3]);
          unsigned y1 = v5_cvt_pk_bf16(p[6], p[7]);
          auto r0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
          auto r1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
          short8 pfrag;
          unsigned* pw = reinterpret_cast<unsigned*>(&pfrag);
          pw[0] = (unsigned)r0[0];
          pw[1] = (unsigned)r1[0];
          pw[2] = (unsigned)r0[1];
          pw[3] = (unsigned)r1[1];
          const int kvg = sub * 32 + g * 16;
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int db = 0; db < 4; ++db) {
            short8 vf = VROWS ? v5_read_tr(vt_lds, lane, kvg, db)
                              : v5_read(vt_lds, db * 32 + l31, (kvg >> 3) + lhi, 8);
            o_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pfrag, o_acc[db], 0, 0, 0);
          }
          __builtin_amdgcn_s_setprio(0);
        }
      }
      rsum += __shfl_xor(rsum, 32, 64);
      l_run = l_run * alpha + rsum;
    }

    __syncthreads();
    buf ^= 1;
  }

  const float inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
  if (!live) return;
  if (PACK) {
    // dead waves of a straddling block took part in every barrier above;
    // only their store is dropped.  The column bound keeps a bad plan from
    // writing outside O^T.
    const long long col = (long long)pk_base[b] + q_lane;
    if (q_lane < skip || col < 0 || col >= Tp) return;
    if (PACK == 2) {
      // a lane's 64 d values are 16 runs of four consecutive d: 16 stores
      // of 8 bytes in place of 64 2-byte column stores
      ushort* Op = OT + col * ((long long)H * D) + h * D + 4 * lhi;
#pragma unroll
      for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          // r = 4g .. 4g+3  ->  d = db*32 + 8g + 4*lhi + (0..3)
          ushort4 v;
          v.x = f2bf(o_acc[db][g * 4 + 0] * inv_l);
          v.y = f2bf(o_acc[db][g * 4 + 1] * inv_l);
          v.z = f2bf(o_acc[db][g * 4 + 2] * inv_l);
          v.w = f2bf(o_acc[db][g * 4 + 3] * inv_l);
          *reinterpret_cast<ushort4*>(Op + db * 32 + 8 * g) = v;
        }
      return;
    }
    ushort* OTp = OT + (long long)h * D * Tp + col;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        OTp[(long long)d * Tp] = f2bf(o_acc[db][r] * inv_l);
      }
    return;
  }
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = db * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      OTh[(long long)d * S + q_lane] = f2bf(o_acc[db][r] * inv_l);
    }
}

extern "C" __global__ void __launch_bounds__(512)
attn_fwd_v5_kernel(const ushort* __restrict__ Q, const ushort* __restrict__ K,
                   const ushort* __restrict__ VT, ushort* __restrict__ OT,
                   int B, int H, int Hk, int S, float scale) {
  attn5_body<0>(Q, K, VT, OT, B, H, Hk, S, scale);
}

// Prefix-packed prefill (see attn5_body's PACK note): same body, skipped
// prefix blocks and a [H*D, Tp] packed O^T.
extern "C" __global__ void __launch_bounds__(512)
attn_fwd_v5_packed_kernel(const ushort* __restrict__ Q,
                          const ushort* __restrict__ K,
                          const ushort* __restrict__ VT,
                          ushort* __restrict__ OT, int B, int H, int Hk,
                          int S, float scale, const int* __restrict__ skip,
                          const int* __restrict__ base, int Tp) {
  attn5_body<1>(Q, K, VT, OT, B, H, Hk, S, scale, skip, base, Tp);
}

// The packed kernel with a row-major O [Tp, H*D] (attn5_body's PACK == 2).
extern "C" __global__ void __launch_bounds__(512)
attn_fwd_v5_packed_rm_kernel(const ushort* __restrict__ Q,
                             const ushort* __restrict__ K,
                             const ushort* __restrict__ VT,
                             ushort* __restrict__ O, int B, int H, int Hk,
                             int S, float scale, const int* __restrict__ skip,
                             const int* __restrict__ base, int Tp) {
  attn5_body<2>(Q, K, VT, O, B, H, Hk, S, scale, skip, base, Tp);
}

// The row-major packed kernel reading V straight from the packed qkv rows
// (attn5_body's VROWS): no V^T tensor and no transpose pass before it.
// Launched on a 1-D grid of ceil(S / 256) * H * B blocks.
extern "C" __global__ void __launch_bounds__(512)
attn_fwd_v5_packed_rm_qkv_kernel(const ushort* __restrict__ Q,
                                 const ushort* __restrict__ K,
                                 const ushort* __restrict__ qkv, long long ld,
                                 long long v_off, long long Tq,
                                 ushort* __restrict__ O, int B, int H, int Hk,
                                 int S, float scale,
                                 const int* __restrict__ skip,
                                 const int* __restrict__ base,
                                 const int* __restrict__ owner, int Tp) {
  attn5_body<2, true>(Q, K, qkv, O, B, H, Hk, S, scale, skip, base, Tp, owner,
                      ld, v_off, Tq);
}
