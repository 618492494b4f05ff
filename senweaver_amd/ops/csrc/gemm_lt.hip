// Direct hipBLASLt binding with a per-shape tuner.
//
// C[M,N] = A[M,K] . B[N,K]^T, bf16 in/out, fp32 compute, on torch's current
// stream.  torch.matmul takes whatever solution the library's heuristic
// ranks first for a shape; away from M = 8192 that choice is often far from
// the best one the library holds (profiles/prefix_packed_breakdown.txt).
// Here the heuristic is asked for ALL its candidates and, on first sight of
// a (M, N, K, A layout, A stride) key, each one is timed on the shape that
// actually runs; the winner is cached in-process.
//
// Linked against the hipBLASLt that libtorch already loaded (same SONAME),
// so there is exactly one copy of the library in the process.  Only the C
// API decides anything; hipblaslt_ext is used for solution names/indices in
// the report.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <hipblaslt/hipblaslt.h>
#include <hipblaslt/hipblaslt-ext.hpp>

#include <algorithm>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

namespace py = pybind11;

namespace {

// One workspace per stream (two streams run prefills concurrently; a shared
// one would be a race).  128 MiB keeps the stream-K solutions torch picks
// with its own (smaller) workspace among the candidates.
constexpr size_t kWorkspaceBytes = 128ull << 20;
// Asked of the heuristic.  A request for 512 returns 230 at the Llama-3-8B
// prefill shapes; none past the first 128 beat those before it, and every
// candidate costs two runs of tuning time.
constexpr int kMaxCandidates = 128;
constexpr int kMaxTunedKeys = 64;       // cap on cached keys (M varies in real use)
constexpr int kWarmup = 2, kTimed = 10;
constexpr double kDropRatio = 1.5;      // first run this far behind the best: dropped
constexpr double kTieRatio = 1.05;      // within 5% of the sweep's best: the earliest in heuristic order wins
constexpr int kRematch = 3;             // head-to-head rounds, first choice against the winner
// The winner must beat the first choice by 10%.  Smaller margins flip from
// one process to the next (a 3% bar gave two runs of the benchmark different
// solutions, hence different sums), and outputs must not depend on timing
// noise.
constexpr double kMinGain = 0.90;
constexpr double kMinFlops = 1e11;      // ~65 us at 1.5 PF/s; smaller is not tuned

#define LT_CHECK(expr)                                                        \
  do {                                                                        \
    hipblasStatus_t s_ = (expr);                                              \
    TORCH_CHECK(s_ == HIPBLAS_STATUS_SUCCESS, "hipBLASLt: ", #expr,           \
                " failed with status ", (int)s_);                             \
  } while (0)
#define HIP_OK(expr)                                                          \
  do {                                                                        \
    hipError_t e_ = (expr);                                                   \
    TORCH_CHECK(e_ == hipSuccess, #expr, ": ", hipGetErrorString(e_));        \
  } while (0)

// (rows, N, K, layout: 0 row-major / 1 transposed view, A leading stride)
using Key = std::tuple<int64_t, int64_t, int64_t, int, int64_t>;

struct Problem {
  hipblasLtMatmulDesc_t desc = nullptr;
  hipblasLtMatrixLayout_t lw = nullptr, la = nullptr, lc = nullptr;
  std::vector<hipblasLtMatmulHeuristicResult_t> cands;  // heuristic order
  int chosen = 0;        // index into cands
  bool tuned = false;
  double first_us = 0, best_us = 0, tune_ms = 0;
  py::list report;       // per-candidate rows of the tuning run
};

struct State {
  std::mutex mu;
  hipblasLtHandle_t handle = nullptr;
  hipblasLtMatmulPreference_t pref = nullptr;
  int version = 0;
  std::map<Key, Problem> problems;
  std::unordered_map<hipStream_t, torch::Tensor> workspaces;
  int64_t tunes = 0, tuned_keys = 0;
};

State& state() {
  static State* s = new State();  // never destroyed: outlives the HIP runtime teardown order
  return *s;
}

void init_locked(State& st) {
  if (st.handle) return;
  LT_CHECK(hipblasLtCreate(&st.handle));
  LT_CHECK(hipblasLtGetVersion(st.handle, &st.version));
  LT_CHECK(hipblasLtMatmulPreferenceCreate(&st.pref));
  size_t ws = kWorkspaceBytes;
  LT_CHECK(hipblasLtMatmulPreferenceSetAttribute(
      st.pref, HIPBLASLT_MATMUL_PREF_MAX_WORKSPACE_BYTES, &ws, sizeof(ws)));
}

void* workspace_locked(State& st, hipStream_t stream, const torch::Tensor& like) {
  auto it = st.workspaces.find(stream);
  if (it == st.workspaces.end()) {
    auto ws = torch::empty({(int64_t)kWorkspaceBytes},
                           like.options().dtype(torch::kUInt8));
    it = st.workspaces.emplace(stream, ws).first;
  }
  return it->second.data_ptr();
}

// A is row-major [M,K] with row stride >= K (layout 0), or the transposed
// view of a row-major [K,M] tensor (layout 1).
int layout_of(const torch::Tensor& a, int64_t* ld) {
  TORCH_CHECK(a.dim() == 2, "gemm_lt: A must be 2-D");
  const int64_t M = a.size(0), K = a.size(1);
  if (a.stride(1) == 1 && a.stride(0) >= K) { *ld = a.stride(0); return 0; }
  if (a.stride(0) == 1 && a.stride(1) >= M) { *ld = a.stride(1); return 1; }
  TORCH_CHECK(false, "gemm_lt: A must be row-major (any row stride) or the "
                     "transposed view of a row-major tensor");
}

void check_operands(const torch::Tensor& a, const torch::Tensor& b) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda(), "gemm_lt: tensors must be on GPU");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 &&
              b.scalar_type() == torch::kBFloat16, "gemm_lt: bf16 only");
  TORCH_CHECK(b.dim() == 2 && b.is_contiguous(), "gemm_lt: B must be [N,K] contiguous");
  TORCH_CHECK(a.dim() == 2 && a.size(1) == b.size(1), "gemm_lt: K mismatch");
  TORCH_CHECK(a.size(0) > 0 && b.size(0) > 0 && b.size(1) > 0, "gemm_lt: empty operand");
  TORCH_CHECK(a.get_device() == b.get_device(), "gemm_lt: device mismatch");
  TORCH_CHECK((uintptr_t)a.data_ptr() % 16 == 0 && (uintptr_t)b.data_ptr() % 16 == 0,
              "gemm_lt: operands must be 16-byte aligned");
}

// The GEMM may run at more rows than A's view has (out_rows > M): the rows
// past M must then exist in A's storage, which the caller has padded.
void check_rows_in_storage(const torch::Tensor& a, int layout, int64_t ld, int64_t rows) {
  const int64_t K = a.size(1);
  const int64_t last = layout == 0 ? (rows - 1) * ld + K : (K - 1) * ld + rows;
  const int64_t have = (int64_t)(a.storage().nbytes() / a.element_size()) - a.storage_offset();
  TORCH_CHECK(last <= have, "gemm_lt: out_rows reaches past A's storage");
  TORCH_CHECK(layout == 0 || rows <= ld, "gemm_lt: out_rows exceeds the transposed view's row length");
}

Problem& problem_locked(State& st, const Key& key) {
  auto it = st.problems.find(key);
  if (it != st.problems.end()) return it->second;
  if (st.problems.size() >= 4 * (size_t)kMaxTunedKeys) {
    // untuned entries are cheap to rebuild; tuned ones are kept
    for (auto p = st.problems.begin(); p != st.problems.end();)
      p = p->second.tuned ? std::next(p) : st.problems.erase(p);
  }
  const auto [rows, N, K, layout, ld] = key;
  Problem pb;
  LT_CHECK(hipblasLtMatmulDescCreate(&pb.desc, HIPBLAS_COMPUTE_32F, HIP_R_32F));
  // column-major view: C^T[N,rows] = op(W)[N,K] . op(A)[K,rows]
  hipblasOperation_t opw = HIPBLAS_OP_T;
  hipblasOperation_t opa = layout == 0 ? HIPBLAS_OP_N : HIPBLAS_OP_T;
  LT_CHECK(hipblasLtMatmulDescSetAttribute(pb.desc, HIPBLASLT_MATMUL_DESC_TRANSA, &opw, sizeof(opw)));
  LT_CHECK(hipblasLtMatmulDescSetAttribute(pb.desc, HIPBLASLT_MATMUL_DESC_TRANSB, &opa, sizeof(opa)));
  LT_CHECK(hipblasLtMatrixLayoutCreate(&pb.lw, HIP_R_16BF, K, N, K));
  if (layout == 0)
    LT_CHECK(hipblasLtMatrixLayoutCreate(&pb.la, HIP_R_16BF, K, rows, ld));
  else
    LT_CHECK(hipblasLtMatrixLayoutCreate(&pb.la, HIP_R_16BF, rows, K, ld));
  LT_CHECK(hipblasLtMatrixLayoutCreate(&pb.lc, HIP_R_16BF, N, rows, N));
  pb.cands.resize(kMaxCandidates);
  int found = 0;
  hipblasStatus_t s = hipblasLtMatmulAlgoGetHeuristic(
      st.handle, pb.desc, pb.lw, pb.la, pb.lc, pb.lc, st.pref, kMaxCandidates,
      pb.cands.data(), &found);
  if (s != HIPBLAS_STATUS_SUCCESS) found = 0;
  pb.cands.resize(found);
  pb.cands.erase(std::remove_if(pb.cands.begin(), pb.cands.end(),
                                [](const hipblasLtMatmulHeuristicResult_t& r) {
                                  return r.state != HIPBLAS_STATUS_SUCCESS ||
                                         r.workspaceSize > kWorkspaceBytes;
                                }),
                 pb.cands.end());
  return st.problems.emplace(key, std::move(pb)).first->second;
}

hipblasStatus_t run_locked(State& st, Problem& pb, int cand, const void* a,
                           const void* w, void* c, void* ws, hipStream_t stream) {
  const float alpha = 1.f, beta = 0.f;
  return hipblasLtMatmul(st.handle, pb.desc, &alpha, w, pb.lw, a, pb.la, &beta,
                         c, pb.lc, c, pb.lc, &pb.cands[cand].algo, ws,
                         kWorkspaceBytes, stream);
}

Key key_of(const torch::Tensor& a, const torch::Tensor& b, int64_t out_rows,
           int* layout, int64_t* ld) {
  *layout = layout_of(a, ld);
  const int64_t rows = std::max<int64_t>(a.size(0), out_rows);
  if (rows > a.size(0)) check_rows_in_storage(a, *layout, *ld, rows);
  return Key(rows, b.size(0), b.size(1), *layout, *ld);
}

std::string solution_name(State& st, hipblasLtMatmulAlgo_t& algo) {
  try {
    return hipblaslt_ext::getSolutionNameFromAlgo(st.handle, algo);
  } catch (...) {
    return "?";
  }
}

}  // namespace

// C[M,N] = A . B^T with the cached winner of the key (the heuristic's first
// choice where the key was never tuned).  ``out_rows`` > M runs the GEMM at
// out_rows rows (A's storage padded by the caller) and returns the first M.
torch::Tensor gemm_lt(torch::Tensor a, torch::Tensor b, int64_t out_rows,
                      c10::optional<torch::Tensor> out) {
  check_operands(a, b);
  int layout;
  int64_t ld;
  const Key key = key_of(a, b, out_rows, &layout, &ld);
  const int64_t rows = std::get<0>(key), M = a.size(0), N = b.size(0);
  torch::Tensor c;
  if (out.has_value()) {
    c = *out;
    TORCH_CHECK(c.is_cuda() && c.scalar_type() == torch::kBFloat16 && c.is_contiguous() &&
                c.dim() == 2 && c.size(0) == rows && c.size(1) == N,
                "gemm_lt: out must be a contiguous bf16 [rows, N] tensor");
  } else {
    c = torch::empty({rows, N}, a.options());
  }
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  State& st = state();
  std::lock_guard<std::mutex> g(st.mu);
  init_locked(st);
  Problem& pb = problem_locked(st, key);
  TORCH_CHECK(!pb.cands.empty(), "gemm_lt: hipBLASLt has no solution for this problem");
  void* ws = workspace_locked(st, stream, a);
  LT_CHECK(run_locked(st, pb, pb.chosen, a.data_ptr(), b.data_ptr(), c.data_ptr(), ws, stream));
  return rows > M ? c.narrow(0, 0, M) : c;
}

int64_t gemm_lt_candidates(torch::Tensor a, torch::Tensor b) {
  check_operands(a, b);
  int layout;
  int64_t ld;
  const Key key = key_of(a, b, 0, &layout, &ld);
  State& st = state();
  std::lock_guard<std::mutex> g(st.mu);
  init_locked(st);
  return (int64_t)problem_locked(st, key).cands.size();
}

// One named candidate of the key's list (tests and the candidate table).
torch::Tensor gemm_lt_run(torch::Tensor a, torch::Tensor b, int64_t cand) {
  check_operands(a, b);
  int layout;
  int64_t ld;
  const Key key = key_of(a, b, 0, &layout, &ld);
  auto c = torch::empty({a.size(0), b.size(0)}, a.options());
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  State& st = state();
  std::lock_guard<std::mutex> g(st.mu);
  init_locked(st);
  Problem& pb = problem_locked(st, key);
  TORCH_CHECK(cand >= 0 && cand < (int64_t)pb.cands.size(), "gemm_lt_run: no such candidate");
  void* ws = workspace_locked(st, stream, a);
  LT_CHECK(run_locked(st, pb, (int)cand, a.data_ptr(), b.data_ptr(), c.data_ptr(), ws, stream));
  return c;
}

// Tune the key of (a, b, out_rows) unless it is cached.  ``rotation`` is a
// list of weight buffers shaped like b (the same projection in other
// layers): the timed runs cycle through them so that B arrives from HBM, as
// it does in situ, and not from the 256 MB Infinity Cache.  Returns a dict:
// status (tuned | cached | capturing | small | full | unsupported),
// and for tuned/cached keys first_us, best_us, chosen, tune_ms, candidates.
py::dict gemm_lt_tune(torch::Tensor a, torch::Tensor b, int64_t out_rows,
                      std::vector<torch::Tensor> rotation, bool force) {
  check_operands(a, b);
  int layout;
  int64_t ld;
  const Key key = key_of(a, b, out_rows, &layout, &ld);
  const int64_t rows = std::get<0>(key), N = b.size(0), K = b.size(1);
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  State& st = state();
  std::lock_guard<std::mutex> g(st.mu);
  init_locked(st);
  py::dict res;
  auto fill = [&](Problem& pb, const char* status) {
    res["status"] = status;
    res["first_us"] = pb.first_us;
    res["best_us"] = pb.best_us;
    res["chosen"] = pb.chosen;
    res["tune_ms"] = pb.tune_ms;
    res["candidates"] = pb.report;
  };
  {
    auto it = st.problems.find(key);
    if (it != st.problems.end() && it->second.tuned) {
      fill(it->second, "cached");
      return res;
    }
  }
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_OK(hipStreamIsCapturing(stream, &cap));
  if (cap != hipStreamCaptureStatusNone) { res["status"] = "capturing"; return res; }
  if (a.size(0) <= 16) { res["status"] = "small"; return res; }
  if (!force && 2.0 * (double)rows * (double)N * (double)K < kMinFlops) {
    res["status"] = "small";
    return res;
  }
  if (st.tuned_keys >= kMaxTunedKeys) { res["status"] = "full"; return res; }
  Problem& pb = problem_locked(st, key);
  if (pb.cands.empty()) { res["status"] = "unsupported"; return res; }

  std::vector<const void*> ws_b;
  for (auto& t : rotation) {
    // buffers that do not look like b are left out, not an error
    if (!(t.is_cuda() && t.scalar_type() == torch::kBFloat16 && t.is_contiguous() &&
          t.dim() == 2 && t.size(0) == N && t.size(1) == K &&
          t.get_device() == b.get_device() && (uintptr_t)t.data_ptr() % 16 == 0))
      continue;
    ws_b.push_back(t.data_ptr());
  }
  if (ws_b.empty()) ws_b.push_back(b.data_ptr());

  const auto t0 = std::chrono::steady_clock::now();
  void* ws = workspace_locked(st, stream, a);
  auto c1 = torch::empty({rows, N}, a.options());
  auto c2 = torch::empty({rows, N}, a.options());
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  HIP_OK(hipDeviceSynchronize());
  auto timed = [&](int cand, void* c, int n, size_t rot0, float* ms) {
    HIP_OK(hipEventRecord(e0, stream));
    for (int i = 0; i < n; ++i) {
      hipblasStatus_t s = run_locked(st, pb, cand, a.data_ptr(),
                                     ws_b[(rot0 + i) % ws_b.size()], c, ws, stream);
      if (s != HIPBLAS_STATUS_SUCCESS) return false;
    }
    HIP_OK(hipEventRecord(e1, stream));
    HIP_OK(hipEventSynchronize(e1));
    HIP_OK(hipEventElapsedTime(ms, e0, e1));
    return true;
  };
  py::list report;
  std::vector<std::pair<int, double>> sweep;  // (candidate, mean us), heuristic order
  double best = 0;
  int best_i = -1;
  size_t rot = 0;
  for (int i = 0; i < (int)pb.cands.size(); ++i) {
    py::dict row;
    row["cand"] = i;
    row["index"] = hipblaslt_ext::getIndexFromAlgo(pb.cands[i].algo);
    row["name"] = solution_name(st, pb.cands[i].algo);
    row["workspace"] = (int64_t)pb.cands[i].workspaceSize;
    report.append(row);
    float ms = 0;
    // two runs on b itself, into c1 and c2.  The first also pays the
    // one-off load of the solution's code object, so the second is the one
    // that decides whether the candidate is worth timing in full.
    const void* keep = ws_b[0];
    ws_b[0] = b.data_ptr();
    bool ok = timed(i, c1.data_ptr(), 1, 0, &ms) && timed(i, c2.data_ptr(), 1, 0, &ms);
    ws_b[0] = keep;
    if (!ok) { row["status"] = "rejected by the library"; continue; }
    row["first_run_us"] = ms * 1e3;
    if (best_i >= 0 && ms * 1e3 > kDropRatio * best) {
      row["status"] = "dropped after first run";
      continue;
    }
    // same input, two runs: the output must not change
    if (!torch::equal(c1.view(torch::kInt16), c2.view(torch::kInt16))) {
      row["status"] = "not reproducible";
      continue;
    }
    if (!timed(i, c2.data_ptr(), kWarmup, rot, &ms)) { row["status"] = "rejected by the library"; continue; }
    rot += kWarmup;
    if (!timed(i, c2.data_ptr(), kTimed, rot, &ms)) { row["status"] = "rejected by the library"; continue; }
    rot += kTimed;
    const double us = ms * 1e3 / kTimed;
    row["us"] = us;
    row["status"] = "timed";
    if (i == 0) pb.first_us = us;
    sweep.emplace_back(i, us);
    if (best_i < 0 || us < best) { best = us; best_i = i; }
  }
  // Near-ties go to the earliest candidate in the heuristic's order, so that
  // two solutions a percent apart do not trade places from run to run.
  for (const auto& [i, us] : sweep)
    if (us <= kTieRatio * best) { best_i = i; best = us; break; }
  // The sweep ranks; it does not decide.  The first choice ran first, on a
  // GPU that had just been idle, and a 10-run mean moves by a few percent
  // anyway: the sweep's winner is timed again head to head with the first
  // choice, alternating, and replaces it only on a clear win.  Otherwise
  // the first choice (what torch.matmul runs) stays, and with it the
  // summation order.
  if (best_i > 0 && pb.first_us > 0) {
    double t_first = 0, t_best = 0;
    bool ok = true;
    for (int r = 0; r < kRematch && ok; ++r) {
      float m0 = 0, m1 = 0;
      ok = timed(0, c2.data_ptr(), kTimed, rot, &m0) &&
           timed(best_i, c2.data_ptr(), kTimed, rot, &m1);
      rot += kTimed;
      if (r == 0 || m0 < t_first) t_first = m0;
      if (r == 0 || m1 < t_best) t_best = m1;
    }
    if (ok) {
      pb.first_us = t_first * 1e3 / kTimed;
      best = t_best * 1e3 / kTimed;
    }
    if (!ok || best >= kMinGain * pb.first_us) { best_i = 0; best = pb.first_us; }
  }
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipEventDestroy(e0));
  HIP_OK(hipEventDestroy(e1));
  if (best_i < 0) { res["status"] = "unsupported"; return res; }
  pb.chosen = best_i;
  pb.best_us = best;
  pb.tuned = true;
  pb.report = report;
  pb.tune_ms = std::chrono::duration<double, std::milli>(
                   std::chrono::steady_clock::now() - t0).count();
  st.tunes += 1;
  st.tuned_keys += 1;
  fill(pb, "tuned");
  return res;
}

// Device time of zero-filling ``nbytes`` (the cost of padding an activation
// to a row count the GEMM likes better), for the measured down_rows choice.
double gemm_lt_fill_us(torch::Tensor like, int64_t nbytes) {
  TORCH_CHECK(like.is_cuda() && nbytes > 0);
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  auto buf = torch::empty({nbytes}, like.options().dtype(torch::kUInt8));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  HIP_OK(hipMemsetAsync(buf.data_ptr(), 0, (size_t)nbytes, stream));
  HIP_OK(hipEventRecord(e0, stream));
  for (int i = 0; i < kTimed; ++i) HIP_OK(hipMemsetAsync(buf.data_ptr(), 0, (size_t)nbytes, stream));
  HIP_OK(hipEventRecord(e1, stream));
  HIP_OK(hipEventSynchronize(e1));
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  HIP_OK(hipEventDestroy(e0));
  HIP_OK(hipEventDestroy(e1));
  return ms * 1e3 / kTimed;
}

// Every tuned key with its report (the evidence file is written from this).
py::list gemm_lt_tuned() {
  State& st = state();
  std::lock_guard<std::mutex> g(st.mu);
  py::list out;
  for (auto& kv : st.problems) {
    if (!kv.second.tuned) continue;
    const auto& [rows, N, K, layout, ld] = kv.first;
    py::dict d;
    d["rows"] = rows;
    d["N"] = N;
    d["K"] = K;
    d["layout"] = layout == 0 ? "row-major" : "transposed";
    d["ld"] = ld;
    d["first_us"] = kv.second.first_us;
    d["best_us"] = kv.second.best_us;
    d["chosen"] = kv.second.chosen;
    d["tune_ms"] = kv.second.tune_ms;
    d["candidates"] = kv.second.report;
    out.append(d);
  }
  return out;
}

py::dict gemm_lt_stats() {
  State& st = state();
  std::lock_guard<std::mutex> g(st.mu);
  init_locked(st);
  py::dict d;
  d["version"] = st.version;
  d["tunes"] = st.tunes;
  d["tuned_keys"] = st.tuned_keys;
  d["problems"] = (int64_t)st.problems.size();
  d["workspaces"] = (int64_t)st.workspaces.size();
  d["workspace_bytes"] = (int64_t)kWorkspaceBytes;
  return d;
}

void register_gemm_lt(py::module_& m) {
  m.def("gemm_lt", &gemm_lt, "C = A @ B^T through the tuned hipBLASLt solution",
        py::arg("a"), py::arg("b"), py::arg("out_rows") = 0, py::arg("out") = py::none());
  m.def("gemm_lt_tune", &gemm_lt_tune, "time every hipBLASLt candidate of this key once",
        py::arg("a"), py::arg("b"), py::arg("out_rows") = 0,
        py::arg("rotation") = std::vector<torch::Tensor>(), py::arg("force") = false);
  m.def("gemm_lt_candidates", &gemm_lt_candidates, "number of candidates for this key");
  m.def("gemm_lt_run", &gemm_lt_run, "run candidate i of this key's list");
  m.def("gemm_lt_fill_us", &gemm_lt_fill_us, "device time of a zero fill of nbytes");
  m.def("gemm_lt_tuned", &gemm_lt_tuned, "every tuned key with its candidate report");
  m.def("gemm_lt_stats", &gemm_lt_stats, "library version, tune counter, cache sizes");
}
