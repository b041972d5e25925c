// _fks_hip: pybind11 host side of the MI355X replay engine.
//
// DeviceEngine uploads one workload (SoA, already relabelled by pod rank and
// with the initial heap pre-heapified on the host) to HBM once, then
// evaluates batches of candidate policies: one k_replay workgroup per policy
// (replay_kernels.hip, separate translation units), followed by
// k_eval_reduce (here), on the engine's own HIP stream.  Results come back
// as a float64 [P, 13] table with the same columns as the CPU oracle's batch
// API.
#include <hip/hip_runtime.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "launch.h"
#include "replay.hip.h"
#include "replay_rows.hip.h"
#include "replay_duo.hip.h"
#include "scorers.hip.h"
#include "vm_dev.hip.h"
#include "jit_abi.h"
#include "screen_mfma.hip.h"

namespace py = pybind11;
using namespace fksd;


namespace {

// ----------------------------------------------------------------------------
// k_eval_reduce: exact means -> EvaluationResults + policy score, one lane per
// policy (reference simulator/evaluator.py:77-127).
// out columns: score, avg_cpu, avg_mem, avg_gcnt, avg_gmilli, frag, n_snap, n_frag,
//              n_events, n_unplaced, exc, inexact, hash_hi
__global__ __launch_bounds__(64) void k_eval_reduce(const DevResult* __restrict__ res, double* __restrict__ table, int P) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const DevResult r = res[p];
  double* row = table + (size_t)p * 13;
  if (r.exc != EXC_NONE) {   // an aborted replay reports only its exception class
#pragma unroll
    for (int k = 0; k < 13; ++k) row[k] = 0.0;
    row[10] = (double)r.exc;
    return;
  }
  double avg[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const i128 s = (i128)(((u128)r.acc_hi[k] << 64) | r.acc_lo[k]);
    const int64_t c = k < 4 ? r.n_snap : r.n_frag;
    avg[k] = c > 0 ? fixed_div_round_dev(s, (uint64_t)c) : 0.0;
  }
  double score = 0.0;
  if (r.exc == EXC_NONE && r.n_snap > 0 && r.n_unplaced == 0) {
    const double overall = (avg[0] + avg[1] + avg[2] + avg[3]) / 4.0;
    const double pen = avg[4] < 0.1 ? avg[4] : 0.1;
    double s = overall - pen;
    s = s < 1.0 ? s : 1.0;
    score = s > 0.0 ? s : 0.0;
  }
  row[0] = score;
  row[1] = avg[0]; row[2] = avg[1]; row[3] = avg[2]; row[4] = avg[3]; row[5] = avg[4];
  row[6] = (double)r.n_snap; row[7] = (double)r.n_frag; row[8] = (double)r.n_events;
  row[9] = (double)r.n_unplaced; row[10] = (double)r.exc; row[11] = (double)r.inexact;
  row[12] = (double)(r.hash >> 11);
}


// ---- primitive self-tests (one wave) ----------------------------------------------
// out[0] = wave max, out[1] = wave sum, out[2..65] = pair-swapped values,
// out[66..129] = row_shr:1 of the low 32 bits
__global__ __launch_bounds__(64) void k_test_wave_ops(const uint64_t* in, uint64_t* out) {
  const int lane = lane_id();
  const uint64_t v = in[lane];
  const uint64_t m = wave_max_u64(v);
  const int64_t s = wave_sum_i64((int64_t)v);
  const uint64_t sw = swap_pairs64(v);
  const int sh = __builtin_amdgcn_update_dpp(-1, (int)(uint32_t)v, 0x111, 0xF, 0xF, false);
  if (lane == 0) { out[0] = m; out[1] = (uint64_t)s; }
  out[2 + lane] = sw;
  out[66 + lane] = (uint64_t)(int64_t)sh;
}

// Run a sequence of heap operations (op >= 0: push key op; op < 0: pop) on the
// wave-parallel LDS heap; returns the final array (size in out_n).
__global__ __launch_bounds__(64) void k_test_heap(const uint64_t* init, int n0, const int64_t* ops, int nops,
                                                   int lb, uint64_t* out, int* out_n, uint64_t* popped) {
  extern __shared__ uint64_t lds[];
  const int lane = lane_id();
  WaveHeap hp;
  hp.h = nullptr;
  hp.top = lds_ptr(lds);
  hp.T = 1 << 30;   // all slots in LDS
  hp.delmap = reinterpret_cast<FKS_LDS uint32_t*>(lds_ptr(lds) + 4096);
  hp.M = 1 << 30;   // the bitmap covers every slot
  hp.lb = lb;
  hp.lane = lane;
  for (int i = lane; i < n0; i += 64) lds[i] = init[i];
  for (int i = lane; i < 256; i += 64) hp.delmap[i] = 0;
  __syncthreads();
  int n = n0, np = 0;
  uint64_t t_push = 0, t_pop = 0, c_push = 0, c_pop = 0;
  for (int k = 0; k < nops; ++k) {
    const int64_t op = ops[k];
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    if (op >= 0) {
      hp.push(n, (uint64_t)op);
      ++n;
      t_push += __builtin_amdgcn_s_memtime() - t0;
      ++c_push;
    } else if (n > 0) {
      const uint64_t top = uniu64(lds[0]);
      const uint64_t last = uniu64(lds[n - 1]);
      --n;
      if (n > 0) hp.pop_reinsert(n, last);
      if (lane == 0) popped[np] = top;
      ++np;
      t_pop += __builtin_amdgcn_s_memtime() - t0;
      ++c_pop;
    }
  }
  __syncthreads();
  for (int i = lane; i < n; i += 64) out[i] = lds[i];
  if (lane == 0) {
    *out_n = n;
    popped[nops] = c_push ? t_push / c_push : 0;       // cycles per push
    popped[nops + 1] = c_pop ? t_pop / c_pop : 0;      // cycles per pop
  }
}

// ---- exact-arithmetic self-tests (tests/test_gpu_exact_arith.py) -------------------
// The production accumulators, division and finalisers, unchanged, on inputs
// no replay forms.  One wave per block.
//
// Block g runs five sequences through LaneAcc::add, one per accumulator k:
// vals[offs[5g + k], offs[5g + k + 1]); lane k reports (lo, hi, count, inexact).
__global__ __launch_bounds__(64) void k_test_lane_acc(const double* vals, const int32_t* offs, uint64_t* out) {
  const int g = blockIdx.x, lane = lane_id();
  LaneAcc acc;
  acc.init();
  for (int k = 0; k < 5; ++k) {
    const int b = offs[5 * g + k], e = offs[5 * g + k + 1];
    for (int i = b; i < e; ++i) acc.add(k, vals[i]);   // (block-uniform index: v is wave-uniform)
  }
  if (lane < 5) {
    uint64_t* o = out + (size_t)(5 * g + lane) * 4;
    o[0] = (uint64_t)(u128)acc.sum;
    o[1] = (uint64_t)((u128)acc.sum >> 64);
    o[2] = (uint64_t)acc.count;
    o[3] = (uint64_t)(uint32_t)acc.inexact;
  }
}

// Row slot s = 4 * block + row runs its own program ops[offs[s], offs[s + 1])
// on a RowAcc (optionally started from the injected state of lanes 0-4), every
// lane of the row reports its raw (lo, hi, count, inexact), and the row then
// finishes like a replay: write_row_result with the slot's meta
// (processed, exc, n_repush, n_dropped, hash) into res[s] and table row s.
enum { kTestAdd = 0, kTestAddUnit = 1, kTestStashUnit = 2, kTestAddStash = 3, kTestStashDrop = 4 };
__global__ __launch_bounds__(64) void k_test_row_acc(const int32_t* ops, const double* vals, const int32_t* offs,
                                                      const uint64_t* inject, const int64_t* meta, int S, uint64_t* raw,
                                                      DevResult* res, double* table) {
  const int lane = lane_id(), jv = lane & 15, rbase = lane & 48;
  const int s = blockIdx.x * kRowsPerWave + (lane >> 4);
  if (s >= S) return;   // whole rows leave
  RowAcc acc;
  acc.init();
  if (inject && jv < 5) {
    const uint64_t* q = inject + ((size_t)s * 5 + jv) * 4;
    acc.lo = q[0];
    acc.hi = q[1];
    acc.count = (int32_t)q[2];
    acc.inexact = (int32_t)q[3];
  }
  const int b = offs[s], e = offs[s + 1];
  for (int i = b; i < e; ++i) {   // row-uniform trip count and operands
    const int op = ops[i] & 0xFF, k = ops[i] >> 8;
    const double v = vals[i];
    if (op == kTestAdd) acc.add(k, v, jv);
    else if (op == kTestAddUnit) acc.add_unit(k, v, jv);
    else if (op == kTestStashUnit) acc.stash_unit(v, jv);
    else if (op == kTestAddStash) acc.add_stash(jv);
    else acc.stash_drop();
  }
  uint64_t* o = raw + ((size_t)s * kRow + jv) * 4;
  o[0] = acc.lo;
  o[1] = acc.hi;
  o[2] = (uint64_t)(int64_t)acc.count;
  o[3] = (uint64_t)(uint32_t)acc.inexact;
  const int64_t* m = meta + (size_t)s * 5;
  write_row_result(acc, jv, rbase, (int32_t)m[0], (int32_t)m[1], m[2], (int)m[3], (uint64_t)m[4], res + s,
                   table + (size_t)s * 13);
}

// fixed_div_round_dev(A, n), A = (hi << 64 | lo) as a signed 128-bit word: one pair per lane
__global__ __launch_bounds__(64) void k_test_fixed_div(const uint64_t* lo, const uint64_t* hi, const uint64_t* n,
                                                        double* out, int64_t N) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= N) return;
  out[i] = fixed_div_round_dev((i128)(((u128)hi[i] << 64) | lo[i]), n[i]);
}

// div_by_recip(n, d, z) for the integers n in [start, start + count)
__global__ __launch_bounds__(256) void k_test_div_by_recip(double d, double z, int64_t start, int64_t count, double* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  out[i] = div_by_recip((double)(start + i), d, z);
}

}  // namespace

#include "engine_host.hip.h"
#include "suite_host.hip.h"

namespace {
using fks_host::DeviceEngine;
using fks_host::DeviceSuite;

py::array_t<uint64_t> test_wave_ops(py::array_t<uint64_t, py::array::c_style | py::array::forcecast> vals) {
  if (vals.size() != 64) throw std::invalid_argument("need 64 values");
  uint64_t *din = nullptr, *dout = nullptr;
  HIP_OK(hipMalloc(&din, 64 * 8));
  HIP_OK(hipMalloc(&dout, 130 * 8));
  HIP_OK(hipMemcpy(din, vals.data(), 64 * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_test_wave_ops, dim3(1), dim3(64), 0, 0, din, dout);
  HIP_OK(hipGetLastError());
  py::array_t<uint64_t> out(130);
  HIP_OK(hipMemcpy(out.mutable_data(), dout, 130 * 8, hipMemcpyDeviceToHost));
  (void)hipFree(din);
  (void)hipFree(dout);
  return out;
}

// k_score_linear_mfma (screen_mfma.hip.h): signatures (and optionally the
// per-state decisions) of P linear-family candidates on S recorded states.
// X: float32 [S * 5 * 64], W: float32 [tiles * 5 * 64] in the kernel's layout
// (ops/screen.py arranges them).  Returns (sig uint64 [P], dec uint8 [P, S] or None, kernel ms).
// It runs beside the resident program grid (the family coupler calls it), so
// nothing here may wait for the whole device: a private non-blocking stream,
// buffers that only grow (a replaced one is parked by the FreeQueue while a
// grid runs), and a wait on that stream alone.
struct ScreenCtx {
  std::mutex mu;
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  fks_host::DevBuf x, w, sig, dec;
};
ScreenCtx& screen_ctx() {
  static ScreenCtx c;
  return c;
}

py::tuple screen_linear(py::array_t<float, py::array::c_style | py::array::forcecast> X,
                        py::array_t<float, py::array::c_style | py::array::forcecast> W, int S, int P, bool want_dec,
                        int device, int chunks) {
  using namespace fks_screen;
  const int tiles = (P + kScreenCands - 1) / kScreenCands;
  if (S < 1 || P < 1) throw std::invalid_argument("screen: empty");
  const size_t per = (size_t)kScreenSteps * 64;
  if ((size_t)X.size() != (size_t)S * per) throw std::invalid_argument("screen: X must be S * 5 * 64 floats");
  if ((size_t)W.size() != (size_t)tiles * per) throw std::invalid_argument("screen: W must be tiles * 5 * 64 floats");
  if (chunks < 1 || chunks > S) throw std::invalid_argument("screen: chunks must be in [1, S]");
  const int spc = (S + chunks - 1) / chunks;
  const int C = (S + spc - 1) / spc;   // chunks actually holding states
  ScreenCtx& c = screen_ctx();
  std::lock_guard<std::mutex> g(c.mu);
  HIP_OK(hipSetDevice(device));
  if (c.device != device) {
    if (c.stream) throw std::runtime_error("screen: one device per process");
    HIP_OK(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    HIP_OK(hipEventCreate(&c.e0));
    HIP_OK(hipEventCreate(&c.e1));
    c.device = device;
  }
  c.x.reserve((size_t)S * per * 4);
  c.w.reserve((size_t)tiles * per * 4);
  c.sig.reserve((size_t)P * C * 8);
  if (want_dec) c.dec.reserve((size_t)P * S);
  float ms = 0.f;
  py::array_t<uint64_t> sig(P);
  std::vector<uint64_t> sigc((size_t)P * C);
  py::array_t<uint8_t> decv;
  if (want_dec) decv = py::array_t<uint8_t>({(py::ssize_t)P, (py::ssize_t)S});
  uint8_t* dec_host = want_dec ? decv.mutable_data() : nullptr;
  uint64_t* sig_host = sigc.data();
  const float* xh = X.data();
  const float* wh = W.data();
  {
    py::gil_scoped_release rel;
    HIP_OK(hipMemcpyAsync(c.x.p, xh, (size_t)S * per * 4, hipMemcpyHostToDevice, c.stream));
    HIP_OK(hipMemcpyAsync(c.w.p, wh, (size_t)tiles * per * 4, hipMemcpyHostToDevice, c.stream));
    const int blocks = (tiles + kScreenWaves - 1) / kScreenWaves;
    HIP_OK(hipEventRecord(c.e0, c.stream));
    hipLaunchKernelGGL(k_score_linear_mfma, dim3(blocks, C), dim3(64 * kScreenWaves), 0, c.stream, c.x.as<float>(),
                       c.w.as<float>(), S, tiles, want_dec ? c.dec.as<uint8_t>() : nullptr, c.sig.as<uint64_t>(), P,
                       spc);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(c.e1, c.stream));
    HIP_OK(hipMemcpyAsync(sig_host, c.sig.p, (size_t)P * C * 8, hipMemcpyDeviceToHost, c.stream));
    if (want_dec) HIP_OK(hipMemcpyAsync(dec_host, c.dec.p, (size_t)P * S, hipMemcpyDeviceToHost, c.stream));
    HIP_OK(hipStreamSynchronize(c.stream));
    HIP_OK(hipEventElapsedTime(&ms, c.e0, c.e1));
  }
  // fold the chunk signatures in chunk order (ops/screen.py signature())
  uint64_t* out = sig.mutable_data();
  for (int p = 0; p < P; ++p) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (int k = 0; k < C; ++k) h = (h ^ sigc[(size_t)p * C + k]) * 0x100000001b3ull;
    out[p] = h;
  }
  py::object dec = py::none();
  if (want_dec) dec = decv;
  return py::make_tuple(sig, dec, (double)ms);
}

py::tuple test_heap(py::array_t<uint64_t, py::array::c_style | py::array::forcecast> init,
                    py::array_t<int64_t, py::array::c_style | py::array::forcecast> ops, int lb) {
  const int n0 = (int)init.size(), nops = (int)ops.size();
  if (n0 + nops > 4096) throw std::invalid_argument("test heap too large");
  uint64_t *di, *dout, *dpop;
  int64_t* dops;
  int* dn;
  HIP_OK(hipMalloc(&di, (n0 + 1) * 8));
  HIP_OK(hipMalloc(&dops, (nops + 1) * 8));
  HIP_OK(hipMalloc(&dout, 4096 * 8));
  HIP_OK(hipMalloc(&dpop, (nops + 2) * 8));
  HIP_OK(hipMalloc(&dn, 4));
  if (n0) HIP_OK(hipMemcpy(di, init.data(), n0 * 8, hipMemcpyHostToDevice));
  if (nops) HIP_OK(hipMemcpy(dops, ops.data(), nops * 8, hipMemcpyHostToDevice));
  const size_t lds = 4096 * 8 + 1024;
  HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_test_heap), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)lds));
  hipLaunchKernelGGL(k_test_heap, dim3(1), dim3(64), lds, 0, di, n0, dops, nops, lb, dout, dn, dpop);
  HIP_OK(hipGetLastError());
  int n = 0;
  HIP_OK(hipMemcpy(&n, dn, 4, hipMemcpyDeviceToHost));
  py::array_t<uint64_t> out(n), popped(nops + 2);
  if (n) HIP_OK(hipMemcpy(out.mutable_data(), dout, (size_t)n * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(popped.mutable_data(), dpop, (size_t)(nops + 2) * 8, hipMemcpyDeviceToHost));
  for (void* p : {(void*)di, (void*)dops, (void*)dout, (void*)dpop, (void*)dn}) (void)hipFree(p);
  return py::make_tuple(out, popped);
}

// ---- exact-arithmetic self-tests: host side -----------------------------------------
// device buffer of the self-tests: uploaded (or filled with `fill`) on
// construction, freed on scope exit
struct TestBuf {
  void* p = nullptr;
  size_t bytes = 0;
  TestBuf(size_t n, const void* src = nullptr, int fill = 0) : bytes(n) {
    HIP_OK(hipMalloc(&p, n ? n : 16));
    if (src && n) HIP_OK(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
    else HIP_OK(hipMemset(p, fill, n ? n : 16));
  }
  TestBuf(const TestBuf&) = delete;
  TestBuf& operator=(const TestBuf&) = delete;
  ~TestBuf() { (void)hipFree(p); }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
  void download(void* dst) const { if (bytes) HIP_OK(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost)); }
};
using ArrF64 = py::array_t<double, py::array::c_style | py::array::forcecast>;
using ArrI32 = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
using ArrI64 = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;
using ArrU64 = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>;

// offs: n + 1 non-decreasing offsets into an array of `total` entries, from 0 to total
void check_offsets(const ArrI32& offs, int64_t n, int64_t total) {
  if ((int64_t)offs.size() != n + 1) throw std::invalid_argument("offsets: need one more than sequences");
  const int32_t* o = offs.data();
  if (o[0] != 0 || o[n] != total) throw std::invalid_argument("offsets: must span the values");
  for (int64_t i = 0; i < n; ++i)
    if (o[i] > o[i + 1]) throw std::invalid_argument("offsets: decreasing");
}

// LaneAcc::add on 5 * G sequences (k_test_lane_acc): uint64 [5 * G, 4] = (lo, hi, count, inexact)
py::array_t<uint64_t> test_lane_acc(ArrF64 vals, ArrI32 offs) {
  const int64_t nseq = (int64_t)offs.size() - 1;
  if (nseq < 5 || nseq % 5) throw std::invalid_argument("lane acc: sequences come in fives");
  check_offsets(offs, nseq, (int64_t)vals.size());
  TestBuf dv((size_t)vals.size() * 8, vals.data()), doff((size_t)offs.size() * 4, offs.data());
  TestBuf dout((size_t)nseq * 4 * 8, nullptr, 0xFF);
  hipLaunchKernelGGL(k_test_lane_acc, dim3((unsigned)(nseq / 5)), dim3(64), 0, 0, dv.as<double>(), doff.as<int32_t>(),
                     dout.as<uint64_t>());
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  py::array_t<uint64_t> out({(py::ssize_t)nseq, (py::ssize_t)4});
  dout.download(out.mutable_data());
  return out;
}

// Row programs (k_test_row_acc) and both finalisers on their results:
// ops int32 (op | k << 8), vals, offs [S + 1]; inject uint64 [S, 5, 4] or
// empty; meta int64 [S, 5] = (processed, exc, n_repush, n_dropped, hash).
// Returns (raw uint64 [S, 16, 4], acc uint64 [S, 2, 5] (lo, hi), fields int64
// [S, 9] = (n_events, n_snap, n_frag, n_unplaced, n_repush, max_nodes, hash,
// exc, inexact) of the DevResults, write_row_result's table [S, 13],
// k_eval_reduce's table [S, 13] of those DevResults).
py::tuple test_row_acc(ArrI32 ops, ArrF64 vals, ArrI32 offs, ArrU64 inject, ArrI64 meta) {
  const int64_t S = (int64_t)offs.size() - 1;
  if (S < 1 || S > (1 << 20)) throw std::invalid_argument("row acc: 1 .. 2^20 row slots");
  if (ops.size() != vals.size()) throw std::invalid_argument("row acc: ops and vals differ in length");
  check_offsets(offs, S, (int64_t)ops.size());
  for (py::ssize_t i = 0; i < ops.size(); ++i) {
    const int32_t op = ops.data()[i] & 0xFF, k = ops.data()[i] >> 8;
    if (op > kTestStashDrop || k < 0 || k > 4) throw std::invalid_argument("row acc: bad op");
  }
  if (inject.size() != 0 && inject.size() != S * 20) throw std::invalid_argument("row acc: inject must be [S, 5, 4]");
  if (meta.size() != S * 5) throw std::invalid_argument("row acc: meta must be [S, 5]");
  TestBuf dops((size_t)ops.size() * 4, ops.data()), dv((size_t)vals.size() * 8, vals.data());
  TestBuf doff((size_t)offs.size() * 4, offs.data()), dinj((size_t)inject.size() * 8, inject.data());
  TestBuf dmeta((size_t)meta.size() * 8, meta.data());
  TestBuf draw((size_t)S * kRow * 4 * 8, nullptr, 0xFF), dres((size_t)S * sizeof(DevResult), nullptr, 0xFF);
  TestBuf dt1((size_t)S * 13 * 8, nullptr, 0xFF), dt2((size_t)S * 13 * 8, nullptr, 0xFF);
  hipLaunchKernelGGL(k_test_row_acc, dim3((unsigned)((S + kRowsPerWave - 1) / kRowsPerWave)), dim3(64), 0, 0,
                     dops.as<int32_t>(), dv.as<double>(), doff.as<int32_t>(),
                     inject.size() ? dinj.as<uint64_t>() : nullptr, dmeta.as<int64_t>(), (int)S, draw.as<uint64_t>(),
                     dres.as<DevResult>(), dt1.as<double>());
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(k_eval_reduce, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, 0, dres.as<DevResult>(),
                     dt2.as<double>(), (int)S);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  py::array_t<uint64_t> raw({(py::ssize_t)S, (py::ssize_t)kRow, (py::ssize_t)4});
  py::array_t<uint64_t> acc({(py::ssize_t)S, (py::ssize_t)2, (py::ssize_t)5});
  py::array_t<int64_t> fields({(py::ssize_t)S, (py::ssize_t)9});
  py::array_t<double> t1({(py::ssize_t)S, (py::ssize_t)13}), t2({(py::ssize_t)S, (py::ssize_t)13});
  std::vector<DevResult> res((size_t)S);
  draw.download(raw.mutable_data());
  dres.download(res.data());
  dt1.download(t1.mutable_data());
  dt2.download(t2.mutable_data());
  for (int64_t s = 0; s < S; ++s) {
    const DevResult& r = res[(size_t)s];
    for (int k = 0; k < 5; ++k) {
      acc.mutable_data()[s * 10 + k] = r.acc_lo[k];
      acc.mutable_data()[s * 10 + 5 + k] = r.acc_hi[k];
    }
    const int64_t f[9] = {r.n_events, r.n_snap, r.n_frag, r.n_unplaced, r.n_repush, r.max_nodes, (int64_t)r.hash,
                          r.exc, r.inexact};
    std::memcpy(fields.mutable_data() + s * 9, f, sizeof(f));
  }
  return py::make_tuple(raw, acc, fields, t1, t2);
}

// fixed_div_round_dev on (lo, hi, n) triples (k_test_fixed_div)
py::array_t<double> test_fixed_div(ArrU64 lo, ArrU64 hi, ArrU64 n) {
  const int64_t N = (int64_t)lo.size();
  if ((int64_t)hi.size() != N || (int64_t)n.size() != N) throw std::invalid_argument("fixed div: lengths differ");
  py::array_t<double> out(N);
  if (N == 0) return out;
  TestBuf dlo((size_t)N * 8, lo.data()), dhi((size_t)N * 8, hi.data()), dn((size_t)N * 8, n.data());
  TestBuf dout((size_t)N * 8, nullptr, 0xFF);
  hipLaunchKernelGGL(k_test_fixed_div, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, 0, dlo.as<uint64_t>(),
                     dhi.as<uint64_t>(), dn.as<uint64_t>(), dout.as<double>(), N);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  dout.download(out.mutable_data());
  return out;
}

// The reciprocal division of divisor d, as the engine sets it up: z =
// fks_recip_verified(d, hi) (0.0: not verified, the kernels divide), and
// div_by_recip(n, d, RN(1 / d)) on the host and on the device for the integers
// n in [start, start + count) within [0, hi].  Returns (z, host, device).
py::tuple test_div_by_recip(int64_t d, int64_t hi, int64_t start, int64_t count) {
  if (d < 1 || hi < 0 || hi >= (int64_t(1) << 31)) throw std::invalid_argument("div_by_recip: d >= 1, 0 <= hi < 2^31");
  if (count < 0) count = hi + 1 - start;
  if (start < 0 || count < 1 || start + count > hi + 1) throw std::invalid_argument("div_by_recip: range outside [0, hi]");
  std::vector<std::pair<std::pair<int64_t, int64_t>, double>> cache;
  const double z = fks_host::fks_recip_verified(d, hi, cache);
  const double dd = (double)d, zz = 1.0 / dd;
  py::array_t<double> host(count), dev(count);
  double* h = host.mutable_data();
  for (int64_t i = 0; i < count; ++i) h[i] = div_by_recip((double)(start + i), dd, zz);
  TestBuf dout((size_t)count * 8, nullptr, 0xFF);
  hipLaunchKernelGGL(k_test_div_by_recip, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, dd, zz, start, count,
                     dout.as<double>());
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  dout.download(dev.mutable_data());
  return py::make_tuple(z, host, dev);
}

// Loader state shared by every JIT module of a device: a private
// non-blocking stream and persistent buffers.  Loading a module must never
// synchronise with the replay slots' streams: no hipFree (which waits for the
// whole device), no legacy-null-stream copies or launches -- the steady-state
// search loads a module per batch while other batches replay.
struct JitLoader {
  std::mutex mu;
  hipStream_t stream = nullptr;
  uint64_t* dptrs = nullptr;     // program addresses written by fks_jit_table
  uint64_t* hptrs = nullptr;     // pinned mirror
  size_t cap = 0;
  void reserve(size_t n) {
    if (n <= cap) return;
    const size_t want = std::max<size_t>(n, std::max<size_t>(4096, 2 * cap));
    // the old buffers are kept (a hipFree would synchronise the device)
    HIP_OK(hipMalloc(&dptrs, want * 8));
    HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&hptrs), want * 8, hipHostMallocDefault));
    cap = want;
  }
};

JitLoader& jit_loader(int device) {
  static std::mutex mu;
  static std::map<int, std::unique_ptr<JitLoader>> loaders;
  std::lock_guard<std::mutex> g(mu);
  auto& p = loaders[device];
  if (!p) {
    p.reset(new JitLoader());
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  }
  return *p;
}

// A loaded JIT code object of natively compiled programs (ops/jit.py).
// Load: hipModuleLoadData.  With `probe` (LLVM-tier modules, and the first
// baseline module of each skeleton size) the module's `fks_rt_table` global
// receives the runtime-library addresses and the `fks_jit_table` kernel
// reports the program addresses, both on the loader's private stream.
// Without it (baseline modules: the runtime table is already written into
// the image, ops/gcnjit.py) nothing touches the device after the load: the
// only result is the device address of `fks_rt_table` (a host-side symbol
// lookup), from which the caller derives the program addresses with the
// image's fixed layout.  That matters at steady state: GPU_MAX_HW_QUEUES is 4,
// so the loader stream shares a hardware queue with a replay slot, and a
// probe kernel or copy queued there waits for that slot's whole batch.
class JitModule {
 public:
  JitModule(py::bytes image, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> rt, int n_programs,
            int device, bool probe)
      : device_(device), n_(n_programs) {
    if (n_programs < 1) throw std::invalid_argument("empty JIT module");
    const std::string img = image;
    std::vector<uint64_t> rtv(rt.data(), rt.data() + rt.size());
    py::gil_scoped_release rel;    // other islands / the tier-up thread keep running
    HIP_OK(hipSetDevice(device_));
    HIP_OK(hipModuleLoadData(&mod_, img.data()));
    if (!probe) {
      hipDeviceptr_t gp = nullptr;
      size_t gbytes = 0;
      HIP_OK(hipModuleGetGlobal(&gp, &gbytes, mod_, "fks_rt_table"));
      if (gbytes < rtv.size() * 8) throw std::runtime_error("fks_rt_table too small");
      n_ = 1;
      ptrs_.assign(1, reinterpret_cast<uint64_t>(gp));
      return;
    }
    JitLoader& L = jit_loader(device_);
    std::lock_guard<std::mutex> g(L.mu);   // the loader's stream and pointer buffers
    hipDeviceptr_t gp = nullptr;
    size_t gbytes = 0;
    HIP_OK(hipModuleGetGlobal(&gp, &gbytes, mod_, "fks_rt_table"));
    if (gbytes < rtv.size() * 8) throw std::runtime_error("fks_rt_table too small");
    HIP_OK(hipMemcpyHtoDAsync(gp, rtv.data(), rtv.size() * 8, L.stream));
    hipFunction_t f;
    HIP_OK(hipModuleGetFunction(&f, mod_, "fks_jit_table"));
    L.reserve((size_t)n_);
    uint64_t* d = L.dptrs;
    void* args[] = {&d};
    HIP_OK(hipModuleLaunchKernel(f, 1, 1, 1, 1, 1, 1, 0, L.stream, args, nullptr));
    HIP_OK(hipMemcpyAsync(L.hptrs, L.dptrs, (size_t)n_ * 8, hipMemcpyDeviceToHost, L.stream));
    HIP_OK(hipStreamSynchronize(L.stream));
    ptrs_.assign(L.hptrs, L.hptrs + n_);
    for (uint64_t p : ptrs_)
      if (p == 0) throw std::runtime_error("JIT module reported a null program address");
  }
  ~JitModule() {
    if (mod_) {
      (void)hipSetDevice(device_);
      (void)hipDeviceSynchronize();   // no launch may still call into the module
      (void)hipModuleUnload(mod_);
    }
  }
  // Retirement (ops/jit.py): the caller guarantees that every batch that
  // called into this module has completed (per-batch module references), so
  // no device-wide synchronisation is needed.
  void unload() {
    if (!mod_) return;
    hipModule_t m = mod_;
    mod_ = nullptr;
    py::gil_scoped_release rel;
    HIP_OK(hipSetDevice(device_));
    HIP_OK(hipModuleUnload(m));
  }
  bool loaded() const { return mod_ != nullptr; }
  uint64_t global_address(const std::string& name) {
    if (!mod_) throw std::runtime_error("module unloaded");
    hipDeviceptr_t gp = nullptr;
    size_t gbytes = 0;
    HIP_OK(hipModuleGetGlobal(&gp, &gbytes, mod_, name.c_str()));
    return reinterpret_cast<uint64_t>(gp);
  }
  // bytes of a module global read back from the device (layout checks: the
  // runtime table written into the image must be what the device sees)
  py::bytes read_global(const std::string& name, size_t nbytes) {
    if (!mod_) throw std::runtime_error("module unloaded");
    hipDeviceptr_t gp = nullptr;
    size_t gbytes = 0;
    HIP_OK(hipModuleGetGlobal(&gp, &gbytes, mod_, name.c_str()));
    if (nbytes > gbytes) throw std::invalid_argument("read past the global");
    std::string out(nbytes, '\0');
    {
      py::gil_scoped_release rel;
      HIP_OK(hipSetDevice(device_));
      HIP_OK(hipMemcpyDtoH(&out[0], gp, nbytes));
    }
    return py::bytes(out);
  }
  py::array_t<uint64_t> pointers() const {
    py::array_t<uint64_t> out(n_);
    std::memcpy(out.mutable_data(), ptrs_.data(), (size_t)n_ * 8);
    return out;
  }

 private:
  int device_ = 0, n_ = 0;
  hipModule_t mod_ = nullptr;
  std::vector<uint64_t> ptrs_;
};

// ---- glibc-exact math (glibc_math.h): self-check and device evaluation ----------------
// The host build of the port against the host libm (what CPython calls), on
// `n` arguments per function drawn to cover every branch of exp / log / pow
// (tiny, near 1, large, subnormal results, over- / underflow).  Returns the
// mismatch count per function and the first few mismatching arguments.
//
// The arguments of that draw, `n` per function (glibc_math_selfcheck_args
// hands the same ones to the device test: tests/test_gpu_glibc_math.py).
struct GmArgs {
  std::vector<double> exp_x, log_x, pow_x, pow_y;
};
GmArgs glibc_math_args(int64_t n, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  auto bits = [&](uint64_t lo_exp, uint64_t hi_exp) {
    const uint64_t e = lo_exp + rng() % (hi_exp - lo_exp + 1);
    return fksd::gm::asd((e << 52) | (rng() & ((1ull << 52) - 1)));
  };
  GmArgs a;
  const size_t cap = (size_t)(n > 0 ? n : 0);
  a.exp_x.reserve(cap); a.log_x.reserve(cap); a.pow_x.reserve(cap); a.pow_y.reserve(cap);
  for (int64_t i = 0; i < n; ++i) {
    const int c = (int)(rng() % 10);
    double x;
    if (c < 4) x = -745.2 + U(rng) * (709.8 + 745.2);
    else if (c < 6) x = 2.0 * U(rng) - 1.0;
    else if (c < 7) x = (rng() & 1 ? -1.0 : 1.0) * bits(0x3c0, 0x3fe);
    else if (c < 9) x = (rng() & 1 ? -1.0 : 1.0) * bits(0x3c4, 0x40a);
    else x = (rng() & 1) ? 700.0 + 10.0 * U(rng) : -760.0 + 60.0 * U(rng);
    a.exp_x.push_back(x);
  }
  for (int64_t i = 0; i < n; ++i) {
    const int c = (int)(rng() % 10);
    double x;
    if (c < 3) x = bits(0, 0x7fe);
    else if (c < 6) x = 1.0 + (U(rng) - 0.5) * 0.15;
    else if (c < 8) x = 100.0 * U(rng);
    else x = bits(1023 - 20, 1023 + 20);
    if (!(x > 0.0)) x = 0.5;
    a.log_x.push_back(x);
  }
  for (int64_t i = 0; i < n; ++i) {
    const int cx = (int)(rng() % 10), cy = (int)(rng() % 10);
    double x;
    if (cx < 4) x = 1.0 + (U(rng) - 0.5);
    else if (cx < 7) x = bits(0, 0x7fe);
    else x = 1e4 * U(rng);
    if (!(x > 0.0) || x == 1.0) x = 0.75;
    double y;
    if (cy < 3) y = 40.0 * U(rng) - 20.0;
    else if (cy < 5) y = (double)((int64_t)(rng() % 81) - 40) * 0.5;
    else if (cy < 7) y = 2000.0 * U(rng) - 1000.0;
    else if (cy < 8) y = (rng() & 1 ? -1.0 : 1.0) * ((rng() & 1) ? bits(0x3b8, 0x3c4) : bits(0x43a, 0x444));
    else {
      const double lx = ::log(x);
      y = lx != 0.0 ? (-760.0 + U(rng) * 1475.0) / lx : 3.0;
    }
    if (y == 0.0 || !std::isfinite(y)) y = 2.5;
    a.pow_x.push_back(x);
    a.pow_y.push_back(y);
  }
  return a;
}

py::tuple glibc_math_selfcheck_args(int64_t n, uint64_t seed) {
  const GmArgs a = glibc_math_args(n, seed);
  auto arr = [](const std::vector<double>& v) {
    py::array_t<double> out((py::ssize_t)v.size());
    if (!v.empty()) std::memcpy(out.mutable_data(), v.data(), v.size() * 8);
    return out;
  };
  return py::make_tuple(arr(a.exp_x), arr(a.log_x), arr(a.pow_x), arr(a.pow_y));
}

py::dict glibc_math_selfcheck(int64_t n, uint64_t seed) {
  auto same = [](double a, double b) { return fksd::gm::asu(a) == fksd::gm::asu(b); };
  int64_t bad_exp = 0, bad_log = 0, bad_pow = 0;
  std::vector<std::pair<double, double>> e1, e2, e3;
  {
    py::gil_scoped_release rel;
    const GmArgs a = glibc_math_args(n, seed);
    for (const double x : a.exp_x) {
      double o = 0.0;
      const int st = fksd::gm::exp(x, o);
      const double g = ::exp(x);
      if (!same(o, g) || (st == 1) != std::isinf(g)) { if (bad_exp++ < 8) e1.push_back({x, 0.0}); }
    }
    for (const double x : a.log_x) {
      double o = 0.0;
      fksd::gm::log(x, o);
      if (!same(o, ::log(x))) { if (bad_log++ < 8) e2.push_back({x, 0.0}); }
    }
    for (size_t i = 0; i < a.pow_x.size(); ++i) {
      const double x = a.pow_x[i], y = a.pow_y[i];
      double o = 0.0;
      const int st = fksd::gm::pow(x, y, o);
      const double g = ::pow(x, y);
      if (!same(o, g) || (st == 1) != std::isinf(g)) { if (bad_pow++ < 8) e3.push_back({x, y}); }
    }
  }
  py::list ex_exp, ex_log, ex_pow;
  for (auto& v : e1) ex_exp.append(v.first);
  for (auto& v : e2) ex_log.append(v.first);
  for (auto& v : e3) ex_pow.append(py::make_tuple(v.first, v.second));
  py::dict d;
  d["n"] = n;
  d["exp"] = bad_exp; d["log"] = bad_log; d["pow"] = bad_pow;
  d["exp_examples"] = ex_exp; d["log_examples"] = ex_log; d["pow_examples"] = ex_pow;
  return d;
}

// The device build on the MI355X: fn 0 exp(x), 1 log(x), 2 pow(x, y).  Returns
// (status, result) per argument (tests/test_gpu_glibc_math.py: == host build).
py::tuple gm_device_batch(int fn, py::array_t<double, py::array::c_style | py::array::forcecast> x,
                          py::array_t<double, py::array::c_style | py::array::forcecast> y, int device) {
  const int64_t n = (int64_t)x.size();
  if (fn < 0 || fn > 2) throw std::invalid_argument("fn: 0 exp, 1 log, 2 pow");
  if ((int64_t)y.size() != n) throw std::invalid_argument("x and y differ in length");
  py::array_t<double> out(n);
  py::array_t<int32_t> st(n);
  if (n == 0) return py::make_tuple(st, out);
  HIP_OK(hipSetDevice(device));
  double *dx = nullptr, *dy = nullptr, *dout = nullptr;
  int32_t* dst = nullptr;
  HIP_OK(hipMalloc(&dx, n * 8));
  HIP_OK(hipMalloc(&dy, n * 8));
  HIP_OK(hipMalloc(&dout, n * 8));
  HIP_OK(hipMalloc(&dst, n * 4));
  HIP_OK(hipMemcpy(dx, x.data(), n * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dy, y.data(), n * 8, hipMemcpyHostToDevice));
  HIP_OK(fksk::launch_gm_batch(fn, dx, dy, dout, dst, n));
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(out.mutable_data(), dout, n * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(st.mutable_data(), dst, n * 4, hipMemcpyDeviceToHost));
  for (void* p : {(void*)dx, (void*)dy, (void*)dout, (void*)dst}) (void)hipFree(p);
  return py::make_tuple(st, out);
}

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // namespace

#ifndef FKS_SOURCE_HASH
#define FKS_SOURCE_HASH ""
#endif
// provenance marker, found by ops/build.py without importing the module
extern "C" __attribute__((used, visibility("default"))) const char fks_source_mark[] = "FKS_SOURCE_HASH=" FKS_SOURCE_HASH;

PYBIND11_MODULE(_fks_hip, m) {
  m.attr("SOURCE_HASH") = FKS_SOURCE_HASH;
  m.doc() = "MI355X replay kernels of funsearch_kubernetes_simulator_amd";
  m.def("device_count", &device_count);
  m.def("test_wave_ops", &test_wave_ops);
  m.def("test_heap", &test_heap);
  m.def("test_lane_acc", &test_lane_acc, py::arg("vals"), py::arg("offs"));
  m.def("test_row_acc", &test_row_acc, py::arg("ops"), py::arg("vals"), py::arg("offs"), py::arg("inject"),
        py::arg("meta"));
  m.attr("TEST_ROW_OPS") = py::make_tuple("add", "add_unit", "stash_unit", "add_stash", "stash_drop");
  m.def("test_fixed_div", &test_fixed_div, py::arg("lo"), py::arg("hi"), py::arg("n"));
  m.def("test_div_by_recip", &test_div_by_recip, py::arg("d"), py::arg("hi"), py::arg("start") = 0,
        py::arg("count") = -1);
  m.def("screen_linear", &screen_linear, py::arg("X"), py::arg("W"), py::arg("S"), py::arg("P"),
        py::arg("want_dec") = false, py::arg("device") = 0, py::arg("chunks") = 1);
  py::class_<DeviceEngine>(m, "DeviceEngine")
      .def(py::init<py::dict, int, int>(), py::arg("workload"), py::arg("device") = 0, py::arg("n_slots") = 4)
      .def("set_options", &DeviceEngine::set_options)
      .def("evaluate_builtin", &DeviceEngine::evaluate_builtin)
      .def("evaluate_programs", &DeviceEngine::evaluate_programs)
      .def("submit_builtin", &DeviceEngine::submit_builtin)
      .def("submit_programs", &DeviceEngine::submit_programs)
      .def("service_start", &DeviceEngine::service_start, py::arg("slots") = 16384, py::arg("share") = 1.0,
           py::arg("idle_polls") = (int64_t)(1 << 24))
      .def("service_submit", &DeviceEngine::service_submit)
      .def("service_poll", &DeviceEngine::service_poll)
      .def("service_stop", &DeviceEngine::service_stop)
      .def("service_abort", &DeviceEngine::service_abort)
      .def("service_info", &DeviceEngine::service_info)
      .def("ready", &DeviceEngine::ready)
      .def("wait", &DeviceEngine::wait)
      .def("n_slots", &DeviceEngine::n_slots)
      .def("profile", &DeviceEngine::profile)
      .def("stage_builtin_only", &DeviceEngine::stage_builtin_only)
      .def("launch_builtin_async", &DeviceEngine::launch_builtin_async)
      .def("would_use_hbm", &DeviceEngine::would_use_hbm)
      .def("would_use_rows", &DeviceEngine::would_use_rows)
      .def("profile_rows", &DeviceEngine::profile_rows)
      .def("synchronize", &DeviceEngine::synchronize)
      .def("info", &DeviceEngine::info)
      .def("submit_native", &DeviceEngine::submit_native)
      .def("evaluate_native", &DeviceEngine::evaluate_native)
      .def("profile_native", &DeviceEngine::profile_native)
      .def("submit_builtin_schedule", &DeviceEngine::submit_builtin_schedule)
      .def("submit_native_schedule", &DeviceEngine::submit_native_schedule)
      .def("wait_schedule", &DeviceEngine::wait_schedule)
      .def("schedule_chunk", &DeviceEngine::schedule_chunk)
      .def("submit_builtin_time", &DeviceEngine::submit_builtin_time)
      .def("submit_native_time", &DeviceEngine::submit_native_time)
      .def("wait_time", &DeviceEngine::wait_time)
      .def("native_rt_table", &DeviceEngine::native_rt_table);
  py::class_<DeviceSuite>(m, "DeviceSuite")
      .def(py::init<py::list, int>(), py::arg("engines"), py::arg("n_slots") = 4)
      .def("submit_native", &DeviceSuite::submit_native)
      .def("ready", &DeviceSuite::ready)
      .def("wait", &DeviceSuite::wait)
      .def("n_slots", &DeviceSuite::n_slots)
      .def("info", &DeviceSuite::info);
  py::class_<JitModule>(m, "JitModule")
      .def(py::init<py::bytes, py::array_t<uint64_t, py::array::c_style | py::array::forcecast>, int, int, bool>(),
           py::arg("image"), py::arg("rt"), py::arg("n_programs"), py::arg("device") = 0, py::arg("probe") = true)
      .def("pointers", &JitModule::pointers)
      .def("unload", &JitModule::unload)
      .def("loaded", &JitModule::loaded)
      .def("read_global", &JitModule::read_global)
      .def("global_address", &JitModule::global_address);
  m.attr("JIT_VGPRS") = kJitVgprs;
  m.attr("JIT_SGPRS") = kJitSgprs;
  m.attr("WEIGHTS_PER_POLICY") = kWeights;
  // host builds of the device math (glibc_math.h), for differential tests against the libm CPython calls
  m.def("gm_exp_batch", [](py::array_t<double, py::array::c_style | py::array::forcecast> x) {
    const py::ssize_t n = x.size();
    py::array_t<double> out(n);
    py::array_t<int32_t> st(n);
    for (py::ssize_t i = 0; i < n; ++i) st.mutable_data()[i] = fksd::gm::exp(x.data()[i], out.mutable_data()[i]);
    return py::make_tuple(st, out);
  });
  m.def("gm_log_batch", [](py::array_t<double, py::array::c_style | py::array::forcecast> x) {
    const py::ssize_t n = x.size();
    py::array_t<double> out(n);
    py::array_t<int32_t> st(n);
    for (py::ssize_t i = 0; i < n; ++i) st.mutable_data()[i] = fksd::gm::log(x.data()[i], out.mutable_data()[i]);
    return py::make_tuple(st, out);
  });
  m.def("gm_pow_batch", [](py::array_t<double, py::array::c_style | py::array::forcecast> x,
                           py::array_t<double, py::array::c_style | py::array::forcecast> y) {
    const py::ssize_t n = x.size();
    if (y.size() != n) throw std::invalid_argument("x and y differ in length");
    py::array_t<double> out(n);
    py::array_t<int32_t> st(n);
    for (py::ssize_t i = 0; i < n; ++i)
      st.mutable_data()[i] = fksd::gm::pow(x.data()[i], y.data()[i], out.mutable_data()[i]);
    return py::make_tuple(st, out);
  });
  m.def("glibc_math_selfcheck", &glibc_math_selfcheck, py::arg("n"), py::arg("seed") = 1);
  m.def("glibc_math_selfcheck_args", &glibc_math_selfcheck_args, py::arg("n"), py::arg("seed") = 1);
  m.def("gm_device_batch", &gm_device_batch, py::arg("fn"), py::arg("x"), py::arg("y"), py::arg("device") = 0);

}
