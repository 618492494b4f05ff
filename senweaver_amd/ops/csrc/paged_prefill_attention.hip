// Paged-context prefill attention (rectangular causal) for gfx950, D=128,
// GQA, page size 16.
//
// Q rows are NEW tokens of sequences whose keys and values (the new tokens'
// included) already sit in the paged KV cache [P, 16, Hk, D]:
//   q, o        [B, Sq, H, D]   token-major (o feeds o_proj untransposed)
//   query row i of sequence b sits at position hist + i,
//   hist = ctx_lens[b] - q_lens[b]; it attends to positions 0 .. hist + i.
//   Rows i >= q_lens[b] are never read from q and are written as zeros.
// Used by prefix caching (append a prompt suffix to a cached conversation);
// shaped so that a K-token speculative verify can use it unchanged.
//
// Structure is attention.hip's (v1): grid (ceil(Sq/64), H, B), 256 threads
// = 4 waves x 16 Q rows; KV tiles of 64 positions = 4 pages; f32 online
// softmax in the MFMA C-fragment layout; P through a wave-private LDS tile.
// What differs:
//   - K and V tiles are gathered page by page through the block table.  One
//     kv head's share of a page is 16 rows x 256 B = 256 sixteen-byte
//     chunks = ONE global_load_lds per thread per page, 8 per tile for K+V,
//     so v1's counted vmcnt carries over; the ring is PP_NSTAGE = 3 buffers
//     deep (two tiles in flight, vmcnt(16)): with ceil(Sq/64) * H blocks the
//     grid leaves most CUs one block or none, and one tile of prefetch hid
//     a fraction of the load latency (profiles/prefix_cache_breakdown.txt).
//     The block's block-table entries are copied to LDS once, so the loop
//     issues no vector-memory operation besides the glds.
//   - Tail positions past the last key are CLAMPED on the load side
//     (every lane loads in bounds, EXEC stays full, no block-table entry at
//     or beyond ceil(ctx/16) is ever turned into an address, and no cache
//     slot at a position >= ctx is ever read) and masked by SELECT on the
//     score side: col > qpos covers both the causal edge (later new keys are
//     present in the cache) and the clamped duplicates.  The clamp is to
//     the last key the BLOCK needs, kv_end - 1 <= ctx - 1, and every row of
//     the block has qpos <= kv_end - 1.
//   - V is row-major [pos][d] here, not V^T: the PV B operand comes from
//     ds_read_b64_tr_b16 (hardware transpose read, inline asm) off an
//     XOR-swizzled image with plain 256-byte rows that the glds source side
//     produces.

#include "common.h"
#include "kernels.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define PP_KVBLK 64
#define PP_QBLK 64
#define PP_PAGE 16
#define PP_D 128
#define PP_NSTAGE 3  // K/V staging ring: PP_NSTAGE - 1 tiles in flight
#define PP_MAX_PAGES 2048  // block-table row length the LDS copy can hold

// XOR of the 16-byte chunk index (0..15) of V image row `row`.  A 32-lane
// half of a transposed read of the 16x16x32 B operand takes rows r..r+3 and
// r+8..r+11, 32 bytes of each: row&3 moves a row by 64 bytes and bit 3 by
// 32, so the 8 rows cover the 64 banks once.  Bits 2 and 5 of the row are
// left out on purpose: rows r+4 and r+32 then sit at a constant byte offset
// from row r, which the reads take as an immediate.
__device__ __forceinline__ int pp_vswz(int row) {
  return ((row & 3) << 2) | (((row >> 3) & 1) << 1);
}

// 16 transposed reads (8 d-tiles x rows r..r+3 and r+4..r+7) at 8 per-lane
// byte addresses plus an immediate, then the wait for their data.  Inline
// asm on purpose: hipcc drains vmcnt before the ds_read_tr builtin (it
// treats the read as aliasing the global_load_lds still in flight), which
// serialises the staging ring; inside asm nothing is waited for that is not
// written here, and nothing is padded either, hence the explicit lgkmcnt.
#define PP_TR_READ16(lo, hi, addr, OFF_LO, OFF_HI)                              \
  asm volatile(                                                                 \
      "ds_read_b64_tr_b16 %0, %16 offset:" #OFF_LO "\n"                          \
      "ds_read_b64_tr_b16 %1, %16 offset:" #OFF_HI "\n"                          \
      "ds_read_b64_tr_b16 %2, %17 offset:" #OFF_LO "\n"                          \
      "ds_read_b64_tr_b16 %3, %17 offset:" #OFF_HI "\n"                          \
      "ds_read_b64_tr_b16 %4, %18 offset:" #OFF_LO "\n"                          \
      "ds_read_b64_tr_b16 %5, %18 offset:" #OFF_HI "\n"                          \
      "ds_read_b64_tr_b16 %6, %19 offset:" #OFF_LO "\n"                          \
      "ds_read_b64_tr_b16 %7, %19 offset:" #OFF_HI "\n"                          \
      "ds_read_b64_tr_b16 %8, %20 offset:" #OFF_LO "\n"                          \
      "ds_read_b64_tr_b16 %9, %20 offset:" #OFF_HI "\n"                          \
      "ds_read_b64_tr_b16 %10, %21 offset:" #OFF_LO "\n"                         \
      "ds_read_b64_tr_b16 %11, %21 offset:" #OFF_HI "\n"                         \
      "ds_read_b64_tr_b16 %12, %22 offset:" #OFF_LO "\n"                         \
      "ds_read_b64_tr_b16 %13, %22 offset:" #OFF_HI "\n"                         \
      "ds_read_b64_tr_b16 %14, %23 offset:" #OFF_LO "\n"                         \
      "ds_read_b64_tr_b16 %15, %23 offset:" #OFF_HI "\n"                         \
      "s_waitcnt lgkmcnt(0)\n"                                                  \
      : "=&v"(lo[0]), "=&v"(hi[0]), "=&v"(lo[1]), "=&v"(hi[1]), "=&v"(lo[2]),   \
        "=&v"(hi[2]), "=&v"(lo[3]), "=&v"(hi[3]), "=&v"(lo[4]), "=&v"(hi[4]),   \
        "=&v"(lo[5]), "=&v"(hi[5]), "=&v"(lo[6]), "=&v"(hi[6]), "=&v"(lo[7]),   \
        "=&v"(hi[7])                                                            \
      : "v"(addr[0]), "v"(addr[1]), "v"(addr[2]), "v"(addr[3]), "v"(addr[4]),   \
        "v"(addr[5]), "v"(addr[6]), "v"(addr[7])                                \
      : "memory")

// Page numbers of the four pages of the KV tile starting at kv0, as seen by
// this thread: page j of the tile holds positions kv0 + 16 j + (tid >> 4).
// Positions past the end are clamped to kv_end - 1 BEFORE the table (the
// block's LDS copy of its first ceil(kv_end / 16) entries) is indexed.
__device__ __forceinline__ void pp_pages(const int* pg_lds, int kv0, int kv_end,
                                         int tid, int pg[4], int off[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int pos = min(kv0 + j * PP_PAGE + (tid >> 4), kv_end - 1);
    pg[j] = pg_lds[pos / PP_PAGE];
    off[j] = pos % PP_PAGE;
  }
}

// Stage one 64-position K tile and V tile (lane-linear glds destination,
// swizzle on the source side).  Thread tid owns LDS slot j*256 + tid of each
// tile: row j*16 + (tid>>4), physical chunk tid&15.
__device__ __forceinline__ void pp_stage(const ushort* __restrict__ Kc,
                                         const ushort* __restrict__ Vc,
                                         const int pg[4], const int off[4],
                                         int Hk, int kvh, ushort* k_lds,
                                         ushort* v_lds, int tid) {
  const int wave_chunk = tid & ~63;
  const int cl = tid & 15;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = j * PP_PAGE + (tid >> 4);
    const long long slot = (long long)pg[j] * PP_PAGE + off[j];
    const long long base = (slot * Hk + kvh) * PP_D;
    const int ck = (cl & 7) ^ (row & 7) | (cl & 8);
    const int cv = cl ^ pp_vswz(row);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)(Kc + base + ck * 8),
        (__attribute__((address_space(3))) unsigned int*)(k_lds + (j * 256 + wave_chunk) * 8),
        16, 0, 0);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)(Vc + base + cv * 8),
        (__attribute__((address_space(3))) unsigned int*)(v_lds + (j * 256 + wave_chunk) * 8),
        16, 0, 0);
  }
}

__device__ __forceinline__ short8 pp_read_k(const ushort* k_lds, int row, int c) {
  const int phys = ((c & 7) ^ (row & 7)) | (c & 8);
  return *reinterpret_cast<const short8*>(k_lds + (row * 16 + phys) * 8);
}

extern "C" __global__ void __launch_bounds__(256, 2)
paged_prefill_attn_kernel(const ushort* __restrict__ Q,       // [B, Sq, H, D]
                          const ushort* __restrict__ Kcache,  // [P, 16, Hk, D]
                          const ushort* __restrict__ Vcache,  // [P, 16, Hk, D]
                          ushort* __restrict__ O,             // [B, Sq, H, D]
                          const int* __restrict__ block_table,  // [B, max_pages]
                          const int* __restrict__ ctx_lens,     // [B]
                          const int* __restrict__ q_lens,       // [B]
                          int Sq, int H, int Hk, int max_pages, float scale) {
  const int qb = blockIdx.x;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int kvh = h / (H / Hk);
  const int tid = threadIdx.x;
  const int wid = tid >> 6;
  const int lane = tid & 63;
  const int kg = lane >> 4;

  const int ctx = ctx_lens[b];
  const int qlen = q_lens[b];
  const int hist = ctx - qlen;
  const int* pages = block_table + (long long)b * max_pages;
  const long long row_ld = (long long)H * PP_D;
  const ushort* Qb = Q + ((long long)b * Sq * H + h) * PP_D;
  ushort* Ob = O + ((long long)b * Sq * H + h) * PP_D;
  const int q0 = qb * PP_QBLK + wid * 16;  // this wave's first Q row

  // A block with no real row (or a sequence whose lengths break the
  // contract 1 <= q_len <= min(Sq, ctx), ctx within the table) only
  // writes its zeros.
  // Block-uniform exit.
  if (qb * PP_QBLK >= qlen || qlen > ctx || qlen > Sq ||
      ctx > min(max_pages, PP_MAX_PAGES) * PP_PAGE) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = q0 + kg * 4 + e;
      if (i < Sq) {
#pragma unroll
        for (int nt = 0; nt < 8; ++nt)
          Ob[(long long)i * row_ld + (lane & 15) + nt * 16] = 0;
      }
    }
    return;
  }

  // ONE __shared__ object: [buf][K | V] tiles, the per-wave P tiles, then
  // the block's copy of its block-table row
  __shared__ __attribute__((aligned(16))) ushort smem[PP_NSTAGE * 2 * PP_KVBLK * PP_D + 4 * 16 * PP_KVBLK + 2 * PP_MAX_PAGES];
  ushort* p_lds = smem + PP_NSTAGE * 2 * PP_KVBLK * PP_D + wid * 16 * PP_KVBLK;
  int* pg_lds = reinterpret_cast<int*>(smem + PP_NSTAGE * 2 * PP_KVBLK * PP_D + 4 * 16 * PP_KVBLK);

  // Q fragments: lane holds Q[q0 + lane%16][kk*32 + kg*8 .. +7]; pad rows
  // read the sequence's last real row instead (their result is discarded).
  short8 qf[4];
  {
    const int i = min(q0 + (lane & 15), qlen - 1);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      qf[kk] = *reinterpret_cast<const short8*>(Qb + (long long)i * row_ld + kk * 32 + kg * 8);
  }

  float m_run[4], l_run[4];
  f32x4 o_acc[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    m_run[e] = -INFINITY;
    l_run[e] = 0.f;
  }
#pragma unroll
  for (int nt = 0; nt < 8; ++nt) o_acc[nt] = {0.f, 0.f, 0.f, 0.f};

  // keys needed by this block: up to its last real row's position
  const int kv_end = hist + min(qlen, qb * PP_QBLK + PP_QBLK);

  // The page numbers this block needs, into LDS first.  Fetched per tile
  // from global memory they would sit in vmcnt between the glds, and hipcc
  // waits for a register load that has glds behind it with vmcnt(0): the
  // ring would drain every iteration.  Entries < ceil(kv_end / 16) only.
  const int ntiles = (kv_end + PP_KVBLK - 1) / PP_KVBLK;
  for (int i = tid; i < (kv_end + PP_PAGE - 1) / PP_PAGE; i += 256) pg_lds[i] = pages[i];
  __syncthreads();

  // prologue: tiles 0 .. PP_NSTAGE-2 into their buffers.  Positions are
  // clamped, so a tile past the end is legal to stage (it re-reads row
  // kv_end-1 and is never used): staging is UNCONDITIONAL, here and in the
  // loop, every iteration issues the same 8 glds and the counted wait is a
  // constant.
  int pg[4], off[4];
#pragma unroll
  for (int s = 0; s < PP_NSTAGE - 1; ++s) {
    ushort* bk = smem + s * (2 * PP_KVBLK * PP_D);
    pp_pages(pg_lds, s * PP_KVBLK, kv_end, tid, pg, off);
    pp_stage(Kcache, Vcache, pg, off, Hk, kvh, bk, bk + PP_KVBLK * PP_D, tid);
  }

  // Transposed reads: lane 4q+p of a 16-lane group supplies row q, columns
  // 4p..4p+3 of the group's 4x16 block.  voff[nt]: this lane's byte offset
  // in a V tile for d-tile nt, rows 8 kg + q; rows +4 and +32 are +1024 and
  // +8192 bytes (pp_vswz).  Every address is inside the tile.
  unsigned voff[8];
  {
    const int tq = (lane & 15) >> 2;
    const int tp = lane & 3;
    const int r = kg * 8 + tq;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
      const int ch = nt * 2 + (tp >> 1);
      voff[nt] = r * 256 + ((ch ^ pp_vswz(r)) * 16) + (tp & 1) * 8;
    }
  }
  const unsigned smem_addr =
      (unsigned)(__UINTPTR_TYPE__)(__attribute__((address_space(3))) const void*)smem;

  int cur = 0;                  // buffer of tile t
  int nxt = PP_NSTAGE - 1;      // buffer of tile t + PP_NSTAGE - 1
  for (int t = 0; t < ntiles; ++t) {
    const int kv0 = t * PP_KVBLK;
    {
      ushort* nk = smem + nxt * (2 * PP_KVBLK * PP_D);
      pp_pages(pg_lds, (t + PP_NSTAGE - 1) * PP_KVBLK, kv_end, tid, pg, off);
      pp_stage(Kcache, Vcache, pg, off, Hk, kvh, nk, nk + PP_KVBLK * PP_D, tid);
    }
    // Counted vmcnt across raw barriers, as in attention.hip: tile t has
    // landed once at most the glds of the PP_NSTAGE - 1 younger tiles (8
    // each) are outstanding; the loop issues no other vector-memory op.
    static_assert(PP_NSTAGE == 3, "the immediate below is 8 * (PP_NSTAGE - 1)");
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const ushort* k_lds = smem + cur * (2 * PP_KVBLK * PP_D);
    const ushort* v_lds = k_lds + PP_KVBLK * PP_D;

    // ---- QK^T: S_tile[16 q][64 kv] ----
    f32x4 s_frag[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        short8 kfrag = pp_read_k(k_lds, kt * 16 + (lane & 15), kk * 4 + kg);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[kk], kfrag, acc, 0, 0, 0);
      }
      s_frag[kt] = acc;
    }

    // ---- online softmax over the 64 new columns ----
    const int col_base = kv0 + (lane & 15);
    float p[4][4];  // [kt][e]
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int qpos = hist + min(q0 + kg * 4 + e, qlen - 1);
      float rmax = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        float sv = s_frag[kt][e] * scale;
        // select, not arithmetic: causal edge and clamped tail in one test
        sv = (col_base + kt * 16 > qpos) ? -INFINITY : sv;
        p[kt][e] = sv;
        rmax = fmaxf(rmax, sv);
      }
      rmax = group_reduce_max<16>(rmax);
      const float m_new = fmaxf(m_run[e], rmax);
      const float alpha = (m_run[e] == -INFINITY) ? 0.f : __expf(m_run[e] - m_new);
      float rsum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        float pv = (p[kt][e] == -INFINITY) ? 0.f : __expf(p[kt][e] - m_new);
        p[kt][e] = pv;
        rsum += pv;
      }
      rsum = group_reduce_sum<16>(rsum);
      l_run[e] = l_run[e] * alpha + rsum;
      m_run[e] = m_new;
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) o_acc[nt][e] *= alpha;
    }

    // ---- P -> wave-private LDS tile (bf16, swizzled rows of 64) ----
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = kg * 4 + e;
        const int col = (lane & 15) + kt * 16;
        const int phys = ((col >> 3) ^ (row & 7)) * 8 + (col & 7);
        p_lds[row * PP_KVBLK + phys] = f2bf(p[kt][e]);
      }
    }

    // ---- PV: O[16,128] += P[16,64] @ V[64,128] ----
    // B operand: lane holds V[k = kk*32 + 8 kg + j][d = nt*16 + lane%16],
    // j = 0..7, from two transposed reads of 4 rows each.  EXEC is full (no
    // divergence in this loop) and no lane's address leaves the tile.
    unsigned vaddr[8];
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
      vaddr[nt] = smem_addr + (unsigned)((cur * 2 + 1) * PP_KVBLK * PP_D * 2) + voff[nt];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      short8 pfrag = *reinterpret_cast<const short8*>(
          p_lds + ((lane & 15) * 8 + (((kk * 4 + kg) & 7) ^ ((lane & 15) & 7))) * 8);
      short4v lo[8], hi[8];
      if (kk == 0) {
        PP_TR_READ16(lo, hi, vaddr, 0, 1024);
      } else {
        PP_TR_READ16(lo, hi, vaddr, 8192, 9216);
      }
#pragma unroll
      for (int nt = 0; nt < 8; ++nt) {
        short8 vfrag = {lo[nt][0], lo[nt][1], lo[nt][2], lo[nt][3],
                        hi[nt][0], hi[nt][1], hi[nt][2], hi[nt][3]};
        o_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pfrag, vfrag, o_acc[nt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_barrier();  // all reads of this tile done
    cur = (cur + 1 == PP_NSTAGE) ? 0 : cur + 1;
    nxt = (nxt + 1 == PP_NSTAGE) ? 0 : nxt + 1;
  }

  // the tiles staged past the end are still landing in LDS: the block must
  // not finish (and free its LDS) before they have
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- epilogue: O /= l, bf16; pad rows get zeros; rows >= Sq nothing ----
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = q0 + kg * 4 + e;
    if (i >= Sq) continue;
    const bool real = i < qlen;
    const float inv_l = (real && l_run[e] > 0.f) ? 1.f / l_run[e] : 0.f;
    ushort* orow = Ob + (long long)i * row_ld;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt)
      orow[(lane & 15) + nt * 16] = real ? f2bf(o_acc[nt][e] * inv_l) : (ushort)0;
  }
}
