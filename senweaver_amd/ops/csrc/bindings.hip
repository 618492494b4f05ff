// PyTorch bindings for the senweaver_amd gfx950 kernel library.
// HIP-native throughout (c10::hip stream accessors) — no CUDA shims.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace {

inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

inline const ushort* bf16_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const ushort*>(t.data_ptr());
}
inline ushort* bf16_mut(torch::Tensor& t) {
  return reinterpret_cast<ushort*>(t.data_ptr());
}

void check_bf16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// Operand checks shared by every dense bf16 GEMM binding (C = A @ B^T).
// The kernels index both operands from M, N and K alone, so a B of another K,
// of another rank or on another device must be refused here.
struct GemmDims { int M, N, K; };

GemmDims check_gemm_operands(const torch::Tensor& a, const torch::Tensor& b,
                             const char* op) {
  check_bf16(a, "a");
  check_bf16(b, "b");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2, op, ": a must be [M, K] and b [N, K]; got ",
              a.dim(), "-d and ", b.dim(), "-d");
  TORCH_CHECK(a.device() == b.device(), op, ": a and b must be on one device");
  TORCH_CHECK(b.size(1) == a.size(1), op, ": K mismatch: a has K=", a.size(1),
              ", b has K=", b.size(1));
  return {(int)a.size(0), (int)b.size(0), (int)a.size(1)};
}

// gemm_bt_8ph_v: whole 256 x 256 tiles only, K a positive multiple of 128
// (the counted-vmcnt pipelines' prologues need two 64-wide K-tiles).
GemmDims check_gemm_256(const torch::Tensor& a, const torch::Tensor& b,
                        const char* op) {
  const GemmDims d = check_gemm_operands(a, b, op);
  TORCH_CHECK(d.M % 256 == 0 && d.N % 256 == 0 && d.K >= 128 && d.K % 128 == 0,
              op, " needs M, N % 256 == 0 and K a positive multiple of 128",
              "; got ", d.M, "x", d.N, "x", d.K);
  return d;
}

// Decode GEMV M-bucket.  The GEMV kernels are instantiated for 1 / 2 / 4 / 8
// (/ 16) activation rows and read that many rows unconditionally: MM is the
// bucket M rounds up to, pad() the activation zero-padded to MM rows.
struct MBucket {
  int MM = 1;
  MBucket(int M, int max_bucket) {
    while (MM < M && MM < max_bucket) MM *= 2;
  }
  torch::Tensor pad(const torch::Tensor& x) const {
    if (x.size(0) >= MM) return x;
    auto xp = torch::zeros({(long)MM, x.size(1)}, x.options());
    xp.narrow(0, 0, x.size(0)).copy_(x);
    return xp;
  }
};

// rmsnorm / fused_add_rmsnorm: the kernel reads hidden / 8 16-byte vectors
// of every row of x and of w.  Returns hidden.
int check_norm_operands(const torch::Tensor& x, const torch::Tensor& w, const char* op) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0, op, ": x must be [..., hidden]");
  const int hidden = x.size(-1);
  TORCH_CHECK(hidden % 8 == 0, op, ": hidden % 8 != 0; got ", hidden);
  TORCH_CHECK(w.numel() == hidden, op, ": w has ", w.numel(), " elements, hidden is ",
              hidden);
  TORCH_CHECK(w.device() == x.device(), op, ": x and w must be on one device");
  return hidden;
}

}  // namespace

// ---------------- RMSNorm ----------------
torch::Tensor rmsnorm(torch::Tensor x, torch::Tensor w, double eps) {
  const int hidden = check_norm_operands(x, w, "rmsnorm");
  const long long rows = x.numel() / hidden;
  auto y = torch::empty_like(x);
  rmsnorm_fwd_kernel<<<dim3((unsigned)rows), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(x), bf16_ptr(w), bf16_mut(y), nullptr, hidden, (float)eps);
  HIP_CHECK_KERNEL();
  return y;
}

// y = rmsnorm(x + residual); residual <- x + residual (in place)
torch::Tensor fused_add_rmsnorm(torch::Tensor x, torch::Tensor residual,
                                torch::Tensor w, double eps) {
  const int hidden = check_norm_operands(x, w, "fused_add_rmsnorm");
  check_bf16(residual, "residual");
  TORCH_CHECK(residual.sizes() == x.sizes() && residual.device() == x.device(),
              "fused_add_rmsnorm: residual must have x's shape and device");
  const long long rows = x.numel() / hidden;
  auto y = torch::empty_like(x);
  rmsnorm_fwd_kernel<<<dim3((unsigned)rows), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(x), bf16_ptr(w), bf16_mut(y), bf16_mut(residual), hidden, (float)eps);
  HIP_CHECK_KERNEL();
  return y;
}

// ---------------- RoPE (in place over q and k) ----------------
void rope_inplace(torch::Tensor q, torch::Tensor k, torch::Tensor cos_sin,
                  torch::Tensor positions) {
  check_bf16(q, "q");
  check_bf16(k, "k");
  TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32 && cos_sin.is_contiguous());
  TORCH_CHECK(positions.scalar_type() == torch::kInt32 && positions.is_contiguous());
  TORCH_CHECK(k.device() == q.device() && cos_sin.device() == q.device() &&
              positions.device() == q.device(),
              "rope_inplace: q, k, cos_sin and positions must be on one GPU");
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && cos_sin.dim() == 2,
              "rope_inplace: q [T,Hq,D], k [T,Hk,D], cos_sin [max_pos,D]");
  const int T = q.size(0);
  const int Hq = q.size(1), Hk = k.size(1), D = q.size(2);
  TORCH_CHECK(k.size(0) == T && k.size(2) == D);
  TORCH_CHECK(cos_sin.size(1) == D && D % 2 == 0);
  // the kernel reads positions[t] for every one of the T grid rows
  TORCH_CHECK(positions.numel() == T, "rope_inplace: ", positions.numel(),
              " positions for ", T, " tokens");
  rope_fwd_kernel<<<dim3(T, Hq + Hk), dim3(64), 0, cur_stream()>>>(
      bf16_mut(q), bf16_mut(k), cos_sin.data_ptr<float>(),
      positions.data_ptr<int>(), Hq, Hk, D);
  HIP_CHECK_KERNEL();
}

// qkv: [T, Hq*D + 2*Hk*D] fused projection -> rope -> q [B,Hq,S,D], k [B,Hk,S,D]
std::vector<torch::Tensor> rope_scatter_qkv(torch::Tensor qkv, torch::Tensor cos_sin,
                                            torch::Tensor positions,
                                            int64_t Hq, int64_t Hk, int64_t D,
                                            int64_t B, int64_t S) {
  check_bf16(qkv, "qkv");
  const long long T = qkv.size(0);
  const long long ld = qkv.size(1);
  TORCH_CHECK(T == B * S && cos_sin.size(1) == D && ld >= (Hq + 2 * Hk) * D);
  auto qo = torch::empty({B, Hq, S, D}, qkv.options());
  auto ko = torch::empty({B, Hk, S, D}, qkv.options());
  TORCH_CHECK((D / 2) % 8 == 0, "rope_scatter needs D/2 % 8 == 0");
  const int heads_per_blk = (int)(256 / (D / 16));
  rope_scatter_kernel<<<dim3((unsigned)T, (unsigned)((Hq + Hk + heads_per_blk - 1) / heads_per_blk)),
                        dim3(256), 0, cur_stream()>>>(
      bf16_ptr(qkv), ld, bf16_mut(qo), bf16_mut(ko),
      cos_sin.data_ptr<float>(), positions.data_ptr<int>(), (int)Hq, (int)Hk,
      (int)D, (int)S);
  HIP_CHECK_KERNEL();
  return {qo, ko};
}

torch::Tensor vt_from_qkv(torch::Tensor qkv, int64_t Hq, int64_t Hk, int64_t D,
                          int64_t B, int64_t S) {
  check_bf16(qkv, "qkv");
  const long long ld = qkv.size(1);
  TORCH_CHECK(qkv.size(0) == B * S && ld >= (Hq + 2 * Hk) * D);
  // the kernel reads 16-byte chunks at (row * ld + head * D + 8 c)
  TORCH_CHECK(ld % 8 == 0 && D % 8 == 0, "vt_from_qkv: row length and D must be multiples of 8");
  auto vt = torch::empty({B, Hk, D, S}, qkv.options());
  const long long v_off = (Hq + Hk) * D;
  transpose_v_kernel<<<dim3((unsigned)((S + 31) / 32), (unsigned)((D + 63) / 64),
                           (unsigned)(B * Hk)),
                       dim3(256), 0, cur_stream()>>>(
      bf16_ptr(qkv), ld, v_off, bf16_mut(vt), (int)B, (int)S, (int)Hk, (int)D);
  HIP_CHECK_KERNEL();
  return vt;
}

torch::Tensor rope_kv_append(torch::Tensor qkv, torch::Tensor cos_sin,
                             torch::Tensor positions, torch::Tensor slot,
                             torch::Tensor kcache, torch::Tensor vcache,
                             int64_t Hq, int64_t Hk, int64_t D) {
  check_bf16(qkv, "qkv");
  const int B = qkv.size(0);
  const long long ld = qkv.size(1);
  TORCH_CHECK(ld >= (Hq + 2 * Hk) * D && (D / 2) % 8 == 0);
  TORCH_CHECK(positions.scalar_type() == torch::kInt32 &&
              slot.scalar_type() == torch::kInt32);
  auto q = torch::empty({(long)B, Hq, D}, qkv.options());
  const int heads_per_blk = (int)(256 / (D / 16));
  const long long H_total = Hq + 2 * Hk;
  rope_kv_append_kernel<<<dim3((unsigned)B, (unsigned)((H_total + heads_per_blk - 1) / heads_per_blk)),
                          dim3(256), 0, cur_stream()>>>(
      bf16_ptr(qkv), ld, bf16_mut(q),
      reinterpret_cast<ushort*>(kcache.data_ptr()),
      reinterpret_cast<ushort*>(vcache.data_ptr()),
      cos_sin.data_ptr<float>(), positions.data_ptr<int>(),
      slot.data_ptr<int>(), (int)Hq, (int)Hk, (int)D);
  HIP_CHECK_KERNEL();
  return q;
}

// ---------------- SwiGLU ----------------
torch::Tensor swiglu(torch::Tensor gateup) {
  check_bf16(gateup, "gateup");
  const int inter2 = gateup.size(-1);
  TORCH_CHECK(inter2 % 16 == 0);
  const int inter = inter2 / 2;
  const long long rows = gateup.numel() / inter2;
  auto sizes = gateup.sizes().vec();
  sizes.back() = inter;
  auto y = torch::empty(sizes, gateup.options());
  const int nvec_blocks = (inter / 8 + 255) / 256;
  swiglu_fwd_kernel<<<dim3(nvec_blocks, (unsigned)rows), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(gateup), bf16_mut(y), rows, inter);
  HIP_CHECK_KERNEL();
  return y;
}

// swiglu into a buffer of out_rows >= rows rows; the rows past the input's
// are zero.  Lets the caller run the next GEMM at a row count of its choice
// without a pad copy of the activation.
torch::Tensor swiglu_padded(torch::Tensor gateup, int64_t out_rows) {
  check_bf16(gateup, "gateup");
  TORCH_CHECK(gateup.dim() == 2, "swiglu_padded: gateup must be [rows, 2*inter]");
  const int inter2 = gateup.size(1);
  TORCH_CHECK(inter2 % 16 == 0);
  const int inter = inter2 / 2;
  const long long rows = gateup.size(0);
  TORCH_CHECK(out_rows >= rows, "swiglu_padded: out_rows < rows");
  auto y = torch::empty({out_rows, (int64_t)inter}, gateup.options());
  const int nvec_blocks = (inter / 8 + 255) / 256;
  if (rows > 0) {
    swiglu_fwd_kernel<<<dim3(nvec_blocks, (unsigned)rows), dim3(256), 0, cur_stream()>>>(
        bf16_ptr(gateup), bf16_mut(y), rows, inter);
    HIP_CHECK_KERNEL();
  }
  if (out_rows > rows) {
    TORCH_CHECK(hipMemsetAsync(bf16_mut(y) + rows * inter, 0,
                               (size_t)(out_rows - rows) * inter * sizeof(ushort),
                               cur_stream()) == hipSuccess,
                "swiglu_padded: hipMemsetAsync failed");
  }
  return y;
}

torch::Tensor add_bf16(torch::Tensor a, torch::Tensor b) {
  check_bf16(a, "a");
  check_bf16(b, "b");
  TORCH_CHECK(a.numel() == b.numel() && a.numel() % 8 == 0);
  auto y = torch::empty_like(a);
  const long long n8 = a.numel() / 8;
  const int blocks = (int)std::min<long long>((n8 + 255) / 256, 2048);
  add_bf16_kernel<<<dim3(blocks), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(a), bf16_ptr(b), bf16_mut(y), n8);
  HIP_CHECK_KERNEL();
  return y;
}

// ---------------- GEMM: C[M,N] = A[M,K] @ B[N,K]^T ----------------
torch::Tensor gemm_bt(torch::Tensor A, torch::Tensor B) {
  const GemmDims d = check_gemm_operands(A, B, "gemm_bt");
  const int M = d.M, K = d.K, N = d.N;
  auto C = torch::empty({M, N}, A.options());
  if (M <= 16) {
    TORCH_CHECK(N % 4 == 0 && K >= 512 && K % 512 == 0,
                "gemv path needs N%4==0, K%512==0 (K >= 512)");
    // wave-per-row coalesced GEMV; A must be padded to the MM bucket rows
    const MBucket bucket(M, 16);
    const int MM = bucket.MM;
    const torch::Tensor Ap = bucket.pad(A);
    const dim3 grid((N + 3) / 4);
    auto launch = [&](auto kern) {
      kern<<<grid, dim3(256), 0, cur_stream()>>>(bf16_ptr(Ap), bf16_ptr(B),
                                                 bf16_mut(C), M, N, K);
    };
    // M=1 wide-K rows: the loader/consumer LDS-DMA streaming engine
    // measures +25% over v2 at K=14336 (5.9 vs 4.7 TB/s,
    // profiles/r02_gemv_engine.txt); at K<=4096 its per-block prologue
    // (x stage + 2-step ring fill) can't amortize over 4 steps and v2 wins
    if (MM == 1 && K % 1024 == 0 && K > 4096 && K <= 14336 && N % 8 == 0) {
      gemv_bt_bf16_v3w_m1<<<dim3(N / 8), dim3(256), 0, cur_stream()>>>(
          bf16_ptr(Ap), bf16_ptr(B), bf16_mut(C), M, N, K);
      HIP_CHECK_KERNEL();
      return C;
    }
    switch (MM) {
      case 1: launch(gemv_bt_bf16_v2_m1); break;
      case 2: launch(gemv_bt_bf16_v2_m2); break;
      case 4: launch(gemv_bt_bf16_v2_m4); break;
      case 8: launch(gemv_bt_bf16_v2_m8); break;
      default: launch(gemv_bt_bf16_v2_m16); break;
    }
    HIP_CHECK_KERNEL();
    return C;
  }
  TORCH_CHECK(K >= 64 && K % 64 == 0,
              "gemm_bt needs K a positive multiple of 64; got K=", K);
  // 256-tile kernels run 1 block/CU (128 KiB LDS): they need >=~160 blocks
  // to fill 256 CUs; below that the 2-block/CU 128-tile kernel wins.
  if (M % 256 == 0 && N % 256 == 0 && (M / 256) * (N / 256) >= 160) {
    const int nwg = (M / 256) * (N / 256);
    if (K % 128 == 0)
      // in-repo best per shape (profiles/r02_gemm_pipeline.txt +
      // r02_gemm_asm_glds.txt): asm7 (raw glds staged INSIDE the MFMA
      // stream) wins big-M and wide-N shapes (1.41/1.23 PF at 8k/gateup);
      // asm4 (between-statement staging) keeps 4096-class; the 16-wave
      // plain-HIP pipeline keeps the remaining small-M shapes
      if (M >= 8192 || (long long)N * 2 >= (long long)M * 7)
        gemm_bt_bf16_asm7_kernel<<<dim3(nwg), dim3(512), 0, cur_stream()>>>(
            bf16_ptr(A), bf16_ptr(B), bf16_mut(C), M, N, K);
      else if (M >= 4096)
        gemm_bt_bf16_asm4_kernel<<<dim3(nwg), dim3(512), 0, cur_stream()>>>(
            bf16_ptr(A), bf16_ptr(B), bf16_mut(C), M, N, K);
      else
        gemm_bt_bf16_8ph_v14_kernel<<<dim3(nwg), dim3(1024), 0, cur_stream()>>>(
            bf16_ptr(A), bf16_ptr(B), bf16_mut(C), M, N, K);
    else
      gemm_bt_bf16_256_kernel<<<dim3(nwg), dim3(512), 0, cur_stream()>>>(
          bf16_ptr(A), bf16_ptr(B), bf16_mut(C), M, N, K);
  } else {
    TORCH_CHECK(M % 128 == 0 && N % 128 == 0,
                "gemm_bt needs M,N % 128 == 0 (pad host-side); got ",
                M, "x", N, "x", K);
    const int nwg = (M / 128) * (N / 128);
    gemm_bt_bf16_kernel<<<dim3(nwg), dim3(256), 0, cur_stream()>>>(
        bf16_ptr(A), bf16_ptr(B), bf16_mut(C), M, N, K);
  }
  HIP_CHECK_KERNEL();
  return C;
}

// ---------------- Grouped GEMM (MoE) ----------------
torch::Tensor grouped_gemm_bt(torch::Tensor A, torch::Tensor W,
                              torch::Tensor tile_expert, torch::Tensor tile_m0,
                              torch::Tensor seg_ends) {
  check_bf16(A, "A");
  check_bf16(W, "W");
  TORCH_CHECK(tile_expert.scalar_type() == torch::kInt32 && tile_expert.is_contiguous());
  TORCH_CHECK(tile_m0.scalar_type() == torch::kInt32 && tile_m0.is_contiguous());
  TORCH_CHECK(seg_ends.scalar_type() == torch::kInt32 && seg_ends.is_contiguous());
  TORCH_CHECK(A.dim() == 2 && W.dim() == 3, "A must be [T, K], W [E, N, K]");
  TORCH_CHECK(W.device() == A.device() && tile_expert.device() == A.device() &&
              tile_m0.device() == A.device() && seg_ends.device() == A.device(),
              "grouped_gemm_bt operands must be on one device");
  TORCH_CHECK(tile_expert.dim() == 1 && tile_m0.dim() == 1 && seg_ends.dim() == 1);
  TORCH_CHECK(seg_ends.size(0) == W.size(0), "seg_ends needs one entry per expert; got ",
              seg_ends.size(0), " for ", W.size(0), " experts");
  TORCH_CHECK(tile_m0.size(0) == tile_expert.size(0),
              "tile_m0 and tile_expert differ in length");
  const int K = A.size(1);
  const int N = W.size(1);
  TORCH_CHECK(W.size(2) == K && N % 128 == 0 && K % 64 == 0);
  const int n_mtiles = tile_expert.size(0);
  // every tile stages 128 rows of A from its m0, whatever the segment holds
  TORCH_CHECK(n_mtiles == 0 || A.size(0) >= 128,
              "grouped_gemm_bt stages 128-row tiles: A needs >= 128 rows (pad); got ",
              A.size(0));
  const int tiles_n = N / 128;
  auto C = torch::empty({A.size(0), (long)N}, A.options());
  if (n_mtiles > 0) {
    grouped_gemm_bt_bf16_kernel<<<dim3(n_mtiles * tiles_n), dim3(256), 0, cur_stream()>>>(
        bf16_ptr(A), bf16_ptr(W), bf16_mut(C), tile_expert.data_ptr<int>(),
        tile_m0.data_ptr<int>(), seg_ends.data_ptr<int>(), N, K, tiles_n);
    HIP_CHECK_KERNEL();
  }
  return C;
}

// ---------------- fp8 path ----------------
// The tiled quantized GEMMs index A, B and both scale tensors from M, N, K
// alone: all four on one GPU, contiguous, one scale row per operand row.
static void check_qgemm_operands(const torch::Tensor& Aq, const torch::Tensor& As,
                                 const torch::Tensor& Bq, const torch::Tensor& Bs) {
  TORCH_CHECK(Aq.is_cuda() && As.device() == Aq.device() && Bq.device() == Aq.device() &&
              Bs.device() == Aq.device(), "quantized GEMM operands must be on one GPU");
  TORCH_CHECK(Aq.is_contiguous() && As.is_contiguous() && Bq.is_contiguous() &&
              Bs.is_contiguous(), "quantized GEMM operands must be contiguous");
  TORCH_CHECK(Aq.dim() == 2 && Bq.dim() == 2, "A_q must be [M, K], B_q [N, K]");
  TORCH_CHECK(As.dim() >= 1 && As.size(0) == Aq.size(0), "a_s needs one row per row of A_q; got ",
              As.size(0), " for M=", Aq.size(0));
  TORCH_CHECK(Bs.dim() >= 1 && Bs.size(0) == Bq.size(0), "b_s needs one row per row of B_q; got ",
              Bs.size(0), " for N=", Bq.size(0));
}

std::vector<torch::Tensor> quant_fp8(torch::Tensor x) {
  check_bf16(x, "x");
  const int K = x.size(-1);
  TORCH_CHECK(K > 0 && K % 8 == 0);
  const long long rows = x.numel() / K;
  auto q = torch::empty({rows, (long)K}, x.options().dtype(torch::kUInt8));
  auto s = torch::empty({rows}, x.options().dtype(torch::kFloat32));
  if (rows == 0) return {q, s};
  quant_fp8_rowwise_kernel<<<dim3((unsigned)rows), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(x), q.data_ptr<unsigned char>(), s.data_ptr<float>(), K);
  HIP_CHECK_KERNEL();
  return {q, s};
}

torch::Tensor gemm_bt_fp8(torch::Tensor Aq, torch::Tensor As,
                          torch::Tensor Bq, torch::Tensor Bs) {
  TORCH_CHECK(Aq.scalar_type() == torch::kUInt8 && Bq.scalar_type() == torch::kUInt8);
  TORCH_CHECK(As.scalar_type() == torch::kFloat32 && Bs.scalar_type() == torch::kFloat32);
  check_qgemm_operands(Aq, As, Bq, Bs);
  TORCH_CHECK(As.dim() == 1 && Bs.dim() == 1, "fp8 scales are one f32 per row");
  const int M = Aq.size(0), K = Aq.size(1), N = Bq.size(0);
  TORCH_CHECK(Bq.size(1) == K && M % 128 == 0 && N % 128 == 0 && K % 128 == 0,
              "fp8 gemm needs M,N%128, K%128; got ", M, "x", N, "x", K);
  auto C = torch::empty({M, N}, Aq.options().dtype(torch::kBFloat16));
  const int nwg = (M / 128) * (N / 128);
  gemm_bt_fp8_kernel<<<dim3(nwg), dim3(256), 0, cur_stream()>>>(
      Aq.data_ptr<unsigned char>(), As.data_ptr<float>(),
      Bq.data_ptr<unsigned char>(), Bs.data_ptr<float>(),
      bf16_mut(C), M, N, K);
  HIP_CHECK_KERNEL();
  return C;
}

// ---------------- MX block-scaled fp8 path ----------------
std::vector<torch::Tensor> quant_mxfp8(torch::Tensor x) {
  check_bf16(x, "x");
  const int K = x.size(-1);
  TORCH_CHECK(K > 0 && K % 32 == 0, "mxfp8 needs K%32; got ", K);
  const long long rows = x.numel() / K;
  auto q = torch::empty({rows, (long)K}, x.options().dtype(torch::kUInt8));
  auto s = torch::empty({rows, (long)(K / 32)}, x.options().dtype(torch::kUInt8));
  if (rows == 0) return {q, s};
  quant_mxfp8_kernel<<<dim3((unsigned)rows), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(x), q.data_ptr<unsigned char>(), s.data_ptr<unsigned char>(), K);
  HIP_CHECK_KERNEL();
  return {q, s};
}

torch::Tensor gemm_bt_mxfp8(torch::Tensor Aq, torch::Tensor As,
                            torch::Tensor Bq, torch::Tensor Bs) {
  TORCH_CHECK(Aq.scalar_type() == torch::kUInt8 && Bq.scalar_type() == torch::kUInt8);
  TORCH_CHECK(As.scalar_type() == torch::kUInt8 && Bs.scalar_type() == torch::kUInt8);
  check_qgemm_operands(Aq, As, Bq, Bs);
  TORCH_CHECK(As.dim() == 2 && Bs.dim() == 2, "mx scales are [rows, K/32] e8m0 bytes");
  const int M = Aq.size(0), K = Aq.size(1), N = Bq.size(0);
  TORCH_CHECK(Bq.size(1) == K && M % 128 == 0 && N % 128 == 0 && K % 128 == 0,
              "mxfp8 gemm needs M,N%128, K%128; got ", M, "x", N, "x", K);
  TORCH_CHECK(As.size(1) == K / 32 && Bs.size(1) == K / 32);
  auto C = torch::empty({M, N}, Aq.options().dtype(torch::kBFloat16));
  const int nwg256 = (M % 256 == 0 && N % 256 == 0) ? (M / 256) * (N / 256) : 0;
  if (nwg256 >= 160) {
    gemm_bt_mxfp8_256_kernel<<<dim3(nwg256), dim3(512), 0, cur_stream()>>>(
        Aq.data_ptr<unsigned char>(), As.data_ptr<unsigned char>(),
        Bq.data_ptr<unsigned char>(), Bs.data_ptr<unsigned char>(),
        bf16_mut(C), M, N, K);
  } else {
    const int nwg = (M / 128) * (N / 128);
    gemm_bt_mxfp8_kernel<<<dim3(nwg), dim3(256), 0, cur_stream()>>>(
        Aq.data_ptr<unsigned char>(), As.data_ptr<unsigned char>(),
        Bq.data_ptr<unsigned char>(), Bs.data_ptr<unsigned char>(),
        bf16_mut(C), M, N, K);
  }
  HIP_CHECK_KERNEL();
  return C;
}

// decode fused add+RMSNorm+GEMV: returns (C [M,N], res_out=x(+res) [M,K])
std::vector<torch::Tensor> gemv_norm_bt(torch::Tensor x, c10::optional<torch::Tensor> res_in,
                                        torch::Tensor normw, torch::Tensor B, double eps) {
  check_bf16(x, "x");
  check_bf16(normw, "normw");
  check_bf16(B, "B");
  const int M = x.size(0), K = x.size(1), N = B.size(0);
  TORCH_CHECK(M <= 16 && N % 4 == 0 && K % 512 == 0 && B.size(1) == K);
  // the kernel reads K norm weights and an [M, K] residual unconditionally
  TORCH_CHECK(normw.numel() == K, "gemv_norm_bt: normw must have K elements");
  TORCH_CHECK(!res_in.has_value() ||
                  (res_in->dim() == 2 && res_in->size(0) == M && res_in->size(1) == K),
              "gemv_norm_bt: res_in must be [M, K]");
  auto C = torch::empty({M, N}, x.options());
  auto res_out = torch::empty({M, K}, x.options());
  const MBucket bucket(M, 16);
  const int MM = bucket.MM;
  const torch::Tensor xp = bucket.pad(x);
  torch::Tensor rp;
  const ushort* rptr = nullptr;
  if (res_in.has_value()) {
    check_bf16(*res_in, "res_in");
    rp = bucket.pad(*res_in);
    rptr = bf16_ptr(rp);
  }
  const dim3 grid((N + 3) / 4);
  auto launch = [&](auto kern) {
    kern<<<grid, dim3(256), 0, cur_stream()>>>(bf16_ptr(xp), rptr,
                                               bf16_ptr(normw), bf16_ptr(B),
                                               bf16_mut(C), bf16_mut(res_out),
                                               M, N, K, (float)eps);
  };
  switch (MM) {
    case 1: launch(gemv_norm_bt_bf16_m1); break;
    case 2: launch(gemv_norm_bt_bf16_m2); break;
    case 4: launch(gemv_norm_bt_bf16_m4); break;
    case 8: launch(gemv_norm_bt_bf16_m8); break;
    default: launch(gemv_norm_bt_bf16_m16); break;
  }
  HIP_CHECK_KERNEL();
  return {C, res_out};
}

// ---------------- Flash attention prefill ----------------
// The kernels index k and vt with q's batch / sequence strides, so a k or vt
// of another shape would be read at the wrong rows (or out of bounds).
static void check_attn_kv(const torch::Tensor& k, const torch::Tensor& vt,
                          int B, int S, int D, const char* op) {
  TORCH_CHECK(k.dim() == 4 && vt.dim() == 4, op, ": k and vt must be 4-D");
  TORCH_CHECK(k.size(0) == B && k.size(2) == S && k.size(3) == D, op,
              ": k must be [B,Hk,S,D] matching q's B, S and D");
  TORCH_CHECK(vt.size(0) == B, op, ": vt batch must match q");
}

torch::Tensor attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor vt,
                       double scale) {
  check_bf16(q, "q");
  check_bf16(k, "k");
  check_bf16(vt, "vt");
  const int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  const int Hk = k.size(1);
  TORCH_CHECK(D == 128, "attn_fwd supports D=128");
  TORCH_CHECK(S % 64 == 0, "S must be padded to 64");
  TORCH_CHECK(vt.size(1) == Hk && vt.size(2) == D && vt.size(3) == S, "vt must be [B,Hk,D,S]");
  TORCH_CHECK(H % Hk == 0);
  check_attn_kv(k, vt, B, S, D, "attn_fwd");
  auto o = torch::empty_like(q);
  attn_fwd_bf16_kernel<<<dim3(S / 64, H, B), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(q), bf16_ptr(k), bf16_ptr(vt), bf16_mut(o), B, H, Hk, S, (float)scale);
  HIP_CHECK_KERNEL();
  return o;
}

// What the kernels that return O^T ask of their operands: D = 128, query
// tiles of 128 rows, vt = V^T [B,Hk,D,S].
struct AttnDims {
  int B, H, Hk, S, D;
};

static AttnDims check_attn_ot(const torch::Tensor& q, const torch::Tensor& k,
                              const torch::Tensor& vt, const char* op) {
  check_bf16(q, "q");
  check_bf16(k, "k");
  check_bf16(vt, "vt");
  const int B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  const int Hk = k.size(1);
  TORCH_CHECK(D == 128 && S % 128 == 0 && H % Hk == 0);
  TORCH_CHECK(vt.size(1) == Hk && vt.size(2) == D && vt.size(3) == S);
  check_attn_kv(k, vt, B, S, D, op);
  return {B, H, Hk, S, D};
}

// v2: swapped-QK^T in-register-softmax kernel; returns O^T [B,H,D,S]
torch::Tensor attn_fwd_v2(torch::Tensor q, torch::Tensor k, torch::Tensor vt,
                          double scale) {
  const auto [B, H, Hk, S, D] = check_attn_ot(q, k, vt, "attn_fwd_v2");
  auto ot = torch::empty({B, H, D, S}, q.options());
  attn_fwd_v2_kernel<<<dim3(S / 128, H, B), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(q), bf16_ptr(k), bf16_ptr(vt), bf16_mut(ot), B, H, Hk, S, (float)scale);
  HIP_CHECK_KERNEL();
  return ot;
}

// v3: v2 structure with 8 waves sharing one staged K/V tile (256 q rows);
// the ladder point v5 is measured against, not reached from ops
torch::Tensor attn_fwd_v3(torch::Tensor q, torch::Tensor k, torch::Tensor vt,
                          double scale) {
  const auto [B, H, Hk, S, D] = check_attn_ot(q, k, vt, "attn_fwd_v3");
  auto ot = torch::empty({B, H, D, S}, q.options());
  attn_fwd_v3_kernel<<<dim3((S + 255) / 256, H, B), dim3(512), 0, cur_stream()>>>(
      bf16_ptr(q), bf16_ptr(k), bf16_ptr(vt), bf16_mut(ot), B, H, Hk, S, (float)scale);
  HIP_CHECK_KERNEL();
  return ot;
}

// v5, the production kernel (attention_v5.hip): 8 waves share a K/V tile
// (256 q rows per block), register-staged prefetch into a double LDS buffer,
// defer-max, softmax VALU diet, sm-split; 501 TF @ B4 H32 S2048 / 580 TF @ B1
// H32 S8192 causal (profiles/r02_attn_ladder.txt).  Returns O^T [B,H,D,S].
torch::Tensor attn_fwd_v5(torch::Tensor q, torch::Tensor k, torch::Tensor vt,
                          double scale) {
  const auto [B, H, Hk, S, D] = check_attn_ot(q, k, vt, "attn_fwd_v5");
  auto ot = torch::empty({B, H, D, S}, q.options());
  attn_fwd_v5_kernel<<<dim3((S + 255) / 256, H, B), dim3(512), 0, cur_stream()>>>(
      bf16_ptr(q), bf16_ptr(k), bf16_ptr(vt), bf16_mut(ot), B, H, Hk, S, (float)scale);
  HIP_CHECK_KERNEL();
  return ot;
}

// ---------------- Prefix-packed prefill ----------------
// skip/base/owner: the per-batch-row layout plan (csrc/README.md, "Packed
// prefill layout").  They live on the device, so only their form is checked
// here; the kernels drop any row a bad plan would send out of bounds.
static void check_plan(const torch::Tensor& t, int64_t B, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kInt32 &&
                  t.is_contiguous() && t.dim() == 1 && t.size(0) == B,
              name, " must be a contiguous int32 GPU tensor of length B");
}

std::vector<torch::Tensor> rope_scatter_qkv_packed(
    torch::Tensor qkv, torch::Tensor cos_sin, torch::Tensor positions,
    int64_t Hq, int64_t Hk, int64_t D, int64_t B, int64_t S,
    torch::Tensor skip, torch::Tensor base, torch::Tensor owner) {
  check_bf16(qkv, "qkv");
  const long long Tp = qkv.size(0);
  const long long ld = qkv.size(1);
  TORCH_CHECK(qkv.dim() == 2 && Tp <= B * S && B * S < (1LL << 31) &&
              cos_sin.size(1) == D && ld >= (Hq + 2 * Hk) * D);
  TORCH_CHECK(cos_sin.is_cuda() && cos_sin.scalar_type() == torch::kFloat32 &&
              cos_sin.is_contiguous());
  TORCH_CHECK(positions.is_cuda() && positions.scalar_type() == torch::kInt32 &&
              positions.is_contiguous() && positions.numel() == Tp,
              "positions must be int32 [Tp] (one per packed row)");
  TORCH_CHECK((D / 2) % 8 == 0 && ld % 8 == 0, "rope_scatter needs D/2 % 8 == 0");
  check_plan(skip, B, "skip");
  check_plan(base, B, "base");
  check_plan(owner, B, "owner");
  auto qo = torch::empty({B, Hq, S, D}, qkv.options());
  auto ko = torch::empty({B, Hk, S, D}, qkv.options());
  const int heads_per_blk = (int)(256 / (D / 16));
  rope_scatter_packed_kernel<<<dim3((unsigned)(B * S), (unsigned)((Hq + Hk + heads_per_blk - 1) / heads_per_blk)),
                               dim3(256), 0, cur_stream()>>>(
      bf16_ptr(qkv), ld, bf16_mut(qo), bf16_mut(ko),
      cos_sin.data_ptr<float>(), positions.data_ptr<int>(), (int)Hq, (int)Hk,
      (int)D, (int)S, (int)B, skip.data_ptr<int>(), base.data_ptr<int>(),
      owner.data_ptr<int>(), Tp);
  HIP_CHECK_KERNEL();
  return {qo, ko};
}

torch::Tensor vt_from_qkv_packed(torch::Tensor qkv, int64_t Hq, int64_t Hk,
                                 int64_t D, int64_t B, int64_t S,
                                 torch::Tensor skip, torch::Tensor base,
                                 torch::Tensor owner) {
  check_bf16(qkv, "qkv");
  const long long Tp = qkv.size(0);
  const long long ld = qkv.size(1);
  TORCH_CHECK(qkv.dim() == 2 && Tp <= B * S && ld >= (Hq + 2 * Hk) * D);
  TORCH_CHECK(ld % 8 == 0 && D % 8 == 0, "vt_from_qkv: row length and D must be multiples of 8");
  check_plan(skip, B, "skip");
  check_plan(base, B, "base");
  check_plan(owner, B, "owner");
  auto vt = torch::empty({B, Hk, D, S}, qkv.options());
  const long long v_off = (Hq + Hk) * D;
  transpose_v_packed_kernel<<<dim3((unsigned)((S + 31) / 32), (unsigned)((D + 63) / 64),
                                  (unsigned)(B * Hk)),
                              dim3(256), 0, cur_stream()>>>(
      bf16_ptr(qkv), ld, v_off, bf16_mut(vt), (int)B, (int)S, (int)Hk, (int)D,
      skip.data_ptr<int>(), base.data_ptr<int>(), owner.data_ptr<int>(), Tp);
  HIP_CHECK_KERNEL();
  return vt;
}

// attn_fwd_v5 on prefix-packed rows: returns ONE O^T [H*D, Tp]; query rows
// below skip[b] are the leader's and are not computed
// row_major: O [Tp, H*D] instead of O^T [H*D, Tp]; the same values.  A
// caller-provided ``out`` lets a test see which rows the kernel leaves alone.
static torch::Tensor attn_packed_launch(torch::Tensor q, torch::Tensor k,
                                        torch::Tensor vt, double scale,
                                        torch::Tensor skip, torch::Tensor base,
                                        int64_t Tp, bool row_major,
                                        c10::optional<torch::Tensor> out) {
  TORCH_CHECK(q.dim() == 4, "attn_fwd_v5_packed: q must be [B,H,S,D]");
  const auto [B, H, Hk, S, D] = check_attn_ot(q, k, vt, "attn_fwd_v5_packed");
  TORCH_CHECK(Tp > 0 && Tp <= (int64_t)B * S && (int64_t)B * S < (1LL << 31),
              "attn_fwd_v5_packed: Tp must be in (0, B*S]");
  check_plan(skip, B, "skip");
  check_plan(base, B, "base");
  const std::vector<int64_t> shape = row_major
      ? std::vector<int64_t>{Tp, (int64_t)H * D}
      : std::vector<int64_t>{(int64_t)H * D, Tp};
  torch::Tensor ot;
  if (out.has_value()) {
    ot = *out;
    check_bf16(ot, "out");
    TORCH_CHECK(ot.sizes().vec() == shape, "attn_fwd_v5_packed: out has the wrong shape");
    TORCH_CHECK((uintptr_t)ot.data_ptr() % 16 == 0, "attn_fwd_v5_packed: out must be 16-byte aligned");
  } else {
    ot = torch::empty(shape, q.options());
  }
  const dim3 grid((S + 255) / 256, H, B);
  if (row_major) {
    attn_fwd_v5_packed_rm_kernel<<<grid, dim3(512), 0, cur_stream()>>>(
        bf16_ptr(q), bf16_ptr(k), bf16_ptr(vt), bf16_mut(ot), B, H, Hk, S,
        (float)scale, skip.data_ptr<int>(), base.data_ptr<int>(), (int)Tp);
  } else {
    attn_fwd_v5_packed_kernel<<<grid, dim3(512), 0, cur_stream()>>>(
        bf16_ptr(q), bf16_ptr(k), bf16_ptr(vt), bf16_mut(ot), B, H, Hk, S,
        (float)scale, skip.data_ptr<int>(), base.data_ptr<int>(), (int)Tp);
  }
  HIP_CHECK_KERNEL();
  return ot;
}

torch::Tensor attn_fwd_v5_packed(torch::Tensor q, torch::Tensor k,
                                 torch::Tensor vt, double scale,
                                 torch::Tensor skip, torch::Tensor base,
                                 int64_t Tp) {
  return attn_packed_launch(q, k, vt, scale, skip, base, Tp, false, c10::nullopt);
}

torch::Tensor attn_fwd_v5_packed_rm(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor vt, double scale,
                                    torch::Tensor skip, torch::Tensor base,
                                    int64_t Tp, c10::optional<torch::Tensor> out) {
  return attn_packed_launch(q, k, vt, scale, skip, base, Tp, true, out);
}

// attn_fwd_v5_packed_rm with V read from the packed qkv rows [Tq, ld] (the
// fused qkv GEMM's output) in place of a V^T made by vt_from_qkv_packed: the
// same O [Tp, Hq*D], bit for bit, without the transpose pass.
torch::Tensor attn_fwd_v5_packed_rm_qkv(torch::Tensor q, torch::Tensor k,
                                        torch::Tensor qkv, int64_t Hq,
                                        int64_t Hk, double scale,
                                        torch::Tensor skip, torch::Tensor base,
                                        torch::Tensor owner, int64_t Tp,
                                        c10::optional<torch::Tensor> out) {
  check_bf16(q, "q");
  check_bf16(k, "k");
  check_bf16(qkv, "qkv");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && qkv.dim() == 2,
              "attn_fwd_v5_packed_rm_qkv: q [B,H,S,D], k [B,Hk,S,D], qkv [Tq,ld]");
  const int64_t B = q.size(0), S = q.size(2), D = q.size(3);
  TORCH_CHECK(q.size(1) == Hq && Hk > 0 && Hq % Hk == 0 && D == 128 && S % 128 == 0,
              "attn_fwd_v5_packed_rm_qkv: needs D == 128, S % 128 == 0, Hq % Hk == 0");
  TORCH_CHECK(k.size(0) == B && k.size(1) == Hk && k.size(2) == S && k.size(3) == D,
              "attn_fwd_v5_packed_rm_qkv: k must be [B,Hk,S,D]");
  const long long Tq = qkv.size(0);
  const long long ld = qkv.size(1);
  TORCH_CHECK(Tq > 0 && Tq <= B * S && ld % 8 == 0 && ld >= (Hq + 2 * Hk) * D,
              "attn_fwd_v5_packed_rm_qkv: qkv must hold (0, B*S] rows of at least "
              "(Hq+2Hk)*D columns, row length a multiple of 8");
  TORCH_CHECK(Tp > 0 && Tp <= B * S && B * S < (1LL << 31),
              "attn_fwd_v5_packed_rm_qkv: Tp must be in (0, B*S]");
  check_plan(skip, B, "skip");
  check_plan(base, B, "base");
  check_plan(owner, B, "owner");
  const std::vector<int64_t> shape{Tp, Hq * D};
  torch::Tensor o;
  if (out.has_value()) {
    o = *out;
    check_bf16(o, "out");
    TORCH_CHECK(o.sizes().vec() == shape, "attn_fwd_v5_packed_rm_qkv: out has the wrong shape");
    TORCH_CHECK((uintptr_t)o.data_ptr() % 16 == 0, "attn_fwd_v5_packed_rm_qkv: out must be 16-byte aligned");
  } else {
    o = torch::empty(shape, q.options());
  }
  const long long v_off = (Hq + Hk) * D;
  const int nqb = (int)((S + 255) / 256);
  // 1-D grid: the kernel orders its blocks over the XCDs itself
  attn_fwd_v5_packed_rm_qkv_kernel<<<dim3((unsigned)(nqb * Hq * B)), dim3(512), 0, cur_stream()>>>(
      bf16_ptr(q), bf16_ptr(k), bf16_ptr(qkv), ld, v_off, Tq, bf16_mut(o),
      (int)B, (int)Hq, (int)Hk, (int)S, (float)scale, skip.data_ptr<int>(),
      base.data_ptr<int>(), owner.data_ptr<int>(), (int)Tp);
  HIP_CHECK_KERNEL();
  return o;
}

// ---------------- Paged decode attention ----------------
torch::Tensor paged_decode_attn(torch::Tensor q, torch::Tensor kcache,
                                torch::Tensor vcache, torch::Tensor block_table,
                                torch::Tensor ctx_lens, double scale) {
  check_bf16(q, "q");
  check_bf16(kcache, "kcache");
  check_bf16(vcache, "vcache");
  TORCH_CHECK(block_table.scalar_type() == torch::kInt32 && block_table.is_contiguous());
  TORCH_CHECK(ctx_lens.scalar_type() == torch::kInt32 && ctx_lens.is_contiguous());
  const int B = q.size(0), H = q.size(1), D = q.size(2);
  const int Hk = kcache.size(2);
  TORCH_CHECK(D == 128 && kcache.size(3) == D);
  TORCH_CHECK(kcache.size(1) == 16, "PAGE_SIZE=16");
  const int max_pages = block_table.size(1);
  auto o = torch::empty_like(q);
  // flash-decoding split-8: partial kernel fills the chip (H*B*8 blocks),
  // merge kernel combines slices.  Both graph-capturable.
  auto partials = torch::empty({B, H, 8, 2 + 128},
                               q.options().dtype(torch::kFloat32));
  paged_decode_attn_partial_kernel<<<dim3(H, B, 8), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(q), bf16_ptr(kcache), bf16_ptr(vcache),
      partials.data_ptr<float>(),
      block_table.data_ptr<int>(), ctx_lens.data_ptr<int>(), H, Hk, max_pages,
      (float)scale);
  paged_decode_attn_merge_kernel<<<dim3(H, B), dim3(64), 0, cur_stream()>>>(
      partials.data_ptr<float>(), bf16_mut(o), H);
  HIP_CHECK_KERNEL();
  return o;
}

// ---------------- Paged-context prefill attention ----------------
// q [B, Sq, H, 128]: the q_lens[b] new tokens of sequence b, whose K/V are
// already in the cache; ctx_lens[b] counts them.  o has q's layout, pad rows
// (i >= q_lens[b]) zero.
torch::Tensor paged_prefill_attn(torch::Tensor q, torch::Tensor kcache,
                                 torch::Tensor vcache, torch::Tensor block_table,
                                 torch::Tensor ctx_lens, torch::Tensor q_lens,
                                 double scale) {
  check_bf16(q, "q");
  check_bf16(kcache, "kcache");
  check_bf16(vcache, "vcache");
  TORCH_CHECK(q.dim() == 4, "q must be [B, Sq, H, D]");
  TORCH_CHECK(kcache.dim() == 4 && vcache.sizes() == kcache.sizes(),
              "caches must be [P, 16, Hk, D] and alike");
  for (const torch::Tensor* t : {&block_table, &ctx_lens, &q_lens})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kInt32 && t->is_contiguous(),
                "block_table / ctx_lens / q_lens must be contiguous int32 on GPU");
  const int B = q.size(0), Sq = q.size(1), H = q.size(2), D = q.size(3);
  const int Hk = kcache.size(2);
  TORCH_CHECK(D == 128 && kcache.size(3) == D, "D must be 128");
  TORCH_CHECK(kcache.size(1) == 16, "PAGE_SIZE=16");
  TORCH_CHECK(Sq >= 1 && B >= 1 && Hk >= 1 && H % Hk == 0);
  TORCH_CHECK(block_table.dim() == 2 && block_table.size(0) == B &&
              block_table.size(1) >= 1 && ctx_lens.numel() == B &&
              q_lens.numel() == B, "block_table / ctx_lens / q_lens: B mismatch");
  // the kernel keeps a block-table row in LDS (PP_MAX_PAGES entries)
  TORCH_CHECK(block_table.size(1) <= 2048,
              "paged_prefill_attn: at most 2048 pages (32768 positions) per sequence");
  auto o = torch::empty_like(q);
  paged_prefill_attn_kernel<<<dim3((Sq + 63) / 64, H, B), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(q), bf16_ptr(kcache), bf16_ptr(vcache), bf16_mut(o),
      block_table.data_ptr<int>(), ctx_lens.data_ptr<int>(), q_lens.data_ptr<int>(),
      Sq, H, Hk, (int)block_table.size(1), (float)scale);
  HIP_CHECK_KERNEL();
  return o;
}

// ---------------- Logit post-processing ----------------
torch::Tensor argmax_rows(torch::Tensor logits) {
  check_bf16(logits, "logits");
  const int rows = logits.size(0), vocab = logits.size(1);
  auto out = torch::empty({rows}, logits.options().dtype(torch::kInt32));
  argmax_rows_kernel<<<dim3(rows), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(logits), out.data_ptr<int>(), vocab);
  HIP_CHECK_KERNEL();
  return out;
}

torch::Tensor target_logprob(torch::Tensor logits, torch::Tensor targets) {
  check_bf16(logits, "logits");
  TORCH_CHECK(targets.scalar_type() == torch::kInt32 && targets.is_contiguous());
  const int rows = logits.size(0), vocab = logits.size(1);
  TORCH_CHECK(targets.size(0) == rows);
  auto out = torch::empty({rows}, logits.options().dtype(torch::kFloat32));
  target_logprob_kernel<<<dim3(rows), dim3(256), 0, cur_stream()>>>(
      bf16_ptr(logits), targets.data_ptr<int>(), out.data_ptr<float>(), vocab);
  HIP_CHECK_KERNEL();
  return out;
}

// gemm_lt.hip: direct hipBLASLt binding with the per-shape tuner
void register_gemm_lt(pybind11::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  register_gemm_lt(m);
  m.def("rmsnorm", &rmsnorm, "RMSNorm fwd (bf16)");
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm, "residual += x; y = rmsnorm(residual)");
  m.def("rope_inplace", &rope_inplace, "RoPE in place over q,k");
  m.def("rope_scatter_qkv", &rope_scatter_qkv, "fused RoPE + [B,H,S,D] scatter from qkv");
  m.def("vt_from_qkv", &vt_from_qkv, "LDS-tiled V^T [B,Hk,D,S] from the qkv slice");
  m.def("rope_kv_append", &rope_kv_append, "decode: slice+RoPE+KV-append in one kernel");
  m.def("gemv_norm_bt", &gemv_norm_bt, "decode: fused add+RMSNorm+GEMV");
  m.def("swiglu", &swiglu, "silu(gate)*up from fused gateup");
  m.def("swiglu_padded", &swiglu_padded,
        "swiglu into [out_rows, inter]; rows past the input's are zero");
  m.def("add_bf16", &add_bf16, "a + b (bf16)");
  m.def("gemm_bt", &gemm_bt, "C = A @ B^T (bf16 MFMA)");
  m.def("gemm_bt_8ph_v", [](torch::Tensor a, torch::Tensor b, long var) {
    const GemmDims d = check_gemm_256(a, b, "gemm_bt_8ph_v");
    const int M = d.M, K = d.K, N = d.N;
    auto C = torch::empty({M, N}, a.options());
    const dim3 g((M / 256) * (N / 256));
    switch (var) {
      case 14: gemm_bt_bf16_8ph_v14_kernel<<<g, dim3(1024), 0, cur_stream()>>>(
                  bf16_ptr(a), bf16_ptr(b), bf16_mut(C), M, N, K); break;
      case 21: gemm_bt_bf16_asm4_kernel<<<g, dim3(512), 0, cur_stream()>>>(
                  bf16_ptr(a), bf16_ptr(b), bf16_mut(C), M, N, K); break;
      case 24: gemm_bt_bf16_asm7_kernel<<<g, dim3(512), 0, cur_stream()>>>(
                  bf16_ptr(a), bf16_ptr(b), bf16_mut(C), M, N, K); break;
      default:
        TORCH_CHECK(false, "gemm_bt_8ph_v: unknown variant ", var,
                    " (known: 14, 21, 24)");
    }
    HIP_CHECK_KERNEL();
    return C;
  }, "the pipelined 256-tile GEMMs gemm_bt dispatches to: 14 = v14, 21 = asm4, 24 = asm7");
  m.def("gemv_bt_v3", [](torch::Tensor a, torch::Tensor b) {
    check_bf16(a, "a"); check_bf16(b, "b");
    const int M = a.size(0), K = a.size(1), N = b.size(0);
    // both kernels walk K in 1024-element steps (two 512 slots per barrier
    // round): K % 1024 != 0 would drop the last slot, and K = 512 would run
    // no step while the loader prologue still fetches 1024 elements per row
    TORCH_CHECK(M == 1 && K >= 1024 && K % 1024 == 0 && K <= 14336 &&
                N >= 8 && N % 8 == 0 && b.size(1) == K,
                "gemv_bt_v3 needs M==1, K%1024==0, 1024<=K<=14336, N%8==0");
    auto C = torch::empty({M, N}, a.options());
    if (K <= 4096)
      gemv_bt_bf16_v3_m1<<<dim3(N / 8), dim3(256), 0, cur_stream()>>>(
          bf16_ptr(a), bf16_ptr(b), bf16_mut(C), M, N, K);
    else
      gemv_bt_bf16_v3w_m1<<<dim3(N / 8), dim3(256), 0, cur_stream()>>>(
          bf16_ptr(a), bf16_ptr(b), bf16_mut(C), M, N, K);
    HIP_CHECK_KERNEL();
    return C;
  }, "loader/consumer LDS-DMA streaming GEMV (M=1)");
  m.def("gemv_bt_fp8w", [](torch::Tensor x, torch::Tensor bq, torch::Tensor bs) {
    check_bf16(x, "x");
    TORCH_CHECK(bq.scalar_type() == torch::kUInt8 && bs.scalar_type() == torch::kFloat32);
    const int M = x.size(0), K = x.size(1), N = bq.size(0);
    TORCH_CHECK(M >= 1 && M <= 8 && K >= 1024 && K % 1024 == 0 && bq.size(1) == K &&
                N % 4 == 0 && bs.numel() == N);
    TORCH_CHECK(bq.is_contiguous() && bs.is_contiguous());
    const MBucket bucket(M, 8);
    const int MM = bucket.MM;
    const torch::Tensor xp = bucket.pad(x);
    auto C = torch::empty({M, N}, x.options());
    // MM==1 runs 1 row/wave (grid N/4); MM>1 runs 2 rows/wave (N/8)
    const int nb = MM > 1 ? (N + 7) / 8 : (N + 3) / 4;
    auto launch = [&](auto kern) {
      kern<<<dim3(nb), dim3(256), 0, cur_stream()>>>(
          bf16_ptr(xp), bq.data_ptr<unsigned char>(), bs.data_ptr<float>(),
          bf16_mut(C), M, N, K);
    };
    switch (MM) {
      case 1: launch(gemv_bt_fp8w_m1); break;
      case 2: launch(gemv_bt_fp8w_m2); break;
      case 4: launch(gemv_bt_fp8w_m4); break;
      default: launch(gemv_bt_fp8w_m8); break;
    }
    HIP_CHECK_KERNEL();
    return C;
  }, "fp8-weight x bf16-activation GEMV (decode, M<=8)");
  m.def("gemv_bt_mxfp8w", [](torch::Tensor x, torch::Tensor bq, torch::Tensor bs) {
    check_bf16(x, "x");
    TORCH_CHECK(bq.scalar_type() == torch::kUInt8 && bs.scalar_type() == torch::kUInt8);
    const int M = x.size(0), K = x.size(1), N = bq.size(0);
    TORCH_CHECK(M >= 1 && M <= 8 && K >= 1024 && K % 1024 == 0 && bq.size(1) == K &&
                bs.dim() == 2 && bs.size(0) == N && bs.size(1) == K / 32 && N % 4 == 0);
    TORCH_CHECK(bq.is_contiguous() && bs.is_contiguous());
    const MBucket bucket(M, 8);
    const int MM = bucket.MM;
    const torch::Tensor xp = bucket.pad(x);
    auto C = torch::empty({M, N}, x.options());
    auto launch = [&](auto kern) {
      kern<<<dim3(N / 4), dim3(256), 0, cur_stream()>>>(
          bf16_ptr(xp), bq.data_ptr<unsigned char>(),
          bs.data_ptr<unsigned char>(), bf16_mut(C), M, N, K);
    };
    switch (MM) {
      case 1: launch(gemv_bt_mxfp8w_m1); break;
      case 2: launch(gemv_bt_mxfp8w_m2); break;
      case 4: launch(gemv_bt_mxfp8w_m4); break;
      default: launch(gemv_bt_mxfp8w_m8); break;
    }
    HIP_CHECK_KERNEL();
    return C;
  }, "mxfp8-weight x bf16-activation GEMV (decode, M<=8)");
  m.def("swiglu_gemv_bt", [](torch::Tensor gu, torch::Tensor b) {
    check_bf16(gu, "gateup"); check_bf16(b, "w");
    const int M = gu.size(0), K2 = gu.size(1), N = b.size(0);
    const int K = K2 / 2;
    TORCH_CHECK(M == 1 && K2 % 2 == 0 && K % 1024 == 0 && K > 4096 &&
                K <= 14336 && N % 8 == 0 && b.size(1) == K);
    auto C = torch::empty({M, N}, gu.options());
    swiglu_gemv_bt_bf16_m1<<<dim3(N / 8), dim3(256), 0, cur_stream()>>>(
        bf16_ptr(gu), bf16_ptr(b), bf16_mut(C), M, N, K);
    HIP_CHECK_KERNEL();
    return C;
  }, "fused silu(g)*u + streaming GEMV (decode down-proj, M=1)");
  m.def("grouped_gemm_bt", &grouped_gemm_bt, "segment-grouped C = A @ W[e]^T (MoE)");
  m.def("moe_combine", [](torch::Tensor down, torch::Tensor pos, torch::Tensor weight) {
    check_bf16(down, "down");
    TORCH_CHECK(pos.scalar_type() == torch::kInt32 && pos.dim() == 2);
    TORCH_CHECK(weight.scalar_type() == torch::kFloat32);
    const long long T = pos.size(0);
    const int k = pos.size(1), H = down.size(1);
    TORCH_CHECK(H % 8 == 0);
    auto out = torch::empty({T, (long)H}, down.options());
    moe_combine_kernel<<<dim3((unsigned)T), dim3(256), 0, cur_stream()>>>(
        bf16_ptr(down), pos.data_ptr<int>(), weight.data_ptr<float>(),
        bf16_mut(out), H, k);
    HIP_CHECK_KERNEL();
    return out;
  }, "routed-FFN weighted combine via inverse permutation");
  m.def("quant_fp8", &quant_fp8, "row-wise bf16 -> e4m3 + scale");
  m.def("gemm_bt_fp8", &gemm_bt_fp8, "fp8 MFMA GEMM with row/col rescale");
  m.def("quant_mxfp8", &quant_mxfp8, "OCP MX quant: bf16 -> e4m3 + e8m0 per-32 scales");
  m.def("gemm_bt_mxfp8", &gemm_bt_mxfp8, "MX block-scaled fp8 MFMA GEMM (32x32x64)");
  m.def("attn_fwd", &attn_fwd, "causal flash attention fwd (D=128, GQA)");
  m.def("attn_fwd_v2", &attn_fwd_v2, "swapped-QK^T attention; O^T out [B,H,D,S]");
  m.def("attn_fwd_v3", &attn_fwd_v3, "v2 with 8-wave shared K/V tiles; O^T out");
  m.def("attn_fwd_v5", &attn_fwd_v5, "production attention; O^T out");
  m.def("rope_scatter_qkv_packed", &rope_scatter_qkv_packed,
        "rope_scatter_qkv reading prefix-packed qkv rows");
  m.def("vt_from_qkv_packed", &vt_from_qkv_packed,
        "vt_from_qkv reading prefix-packed qkv rows");
  m.def("attn_fwd_v5_packed_rm", &attn_fwd_v5_packed_rm,
        "packed attention, row-major O [Tp, H*D]", pybind11::arg("q"), pybind11::arg("k"),
        pybind11::arg("vt"), pybind11::arg("scale"), pybind11::arg("skip"),
        pybind11::arg("base"), pybind11::arg("Tp"), pybind11::arg("out") = pybind11::none());
  m.def("attn_fwd_v5_packed_rm_qkv", &attn_fwd_v5_packed_rm_qkv,
        "packed attention reading V from the packed qkv rows, row-major O [Tp, Hq*D]",
        pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("qkv"), pybind11::arg("Hq"),
        pybind11::arg("Hk"), pybind11::arg("scale"), pybind11::arg("skip"),
        pybind11::arg("base"), pybind11::arg("owner"), pybind11::arg("Tp"),
        pybind11::arg("out") = pybind11::none());
  m.def("attn_fwd_v5_packed", &attn_fwd_v5_packed,
        "attn_fwd_v5 skipping shared-prefix query rows; packed O^T [H*D, Tp] out");
  m.def("paged_decode_attn", &paged_decode_attn, "paged decode attention");
  m.def("paged_prefill_attn", &paged_prefill_attn,
        "prefill attention over the paged cache, queries at an offset");
  m.def("argmax_rows", &argmax_rows, "row argmax over bf16 logits");
  m.def("target_logprob", &target_logprob, "fused log_softmax gather");
}
