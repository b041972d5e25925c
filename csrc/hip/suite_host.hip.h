// DeviceSuite: a native program batch on every trace of a suite in one launch.
//
// Built over the DeviceEngine objects of the suite's traces (one device): each
// trace's arrays stay resident in, and are prepared and gated by, its own
// engine; this object adds what one fused launch needs on top -- an HBM table
// of the T workloads, the block order, and per slot one copy of the batch's
// launch data, the [T, P] result buffers and one heap buffer with an area per
// trace.  The grid is T * P two-wave workgroups (replay_kernels.hip
// k_replay_native_duo_suite); JIT-compiled code does not depend on the
// workload, so fn / kc / koff are staged once and indexed by the program.
//
// Slots follow DeviceEngine's discipline: a non-blocking stream and a
// completion event each; a slot's previous batch is waited for before its
// buffers are restaged; a busy slot refuses a second batch.
#pragma once

#include "engine_host.hip.h"

namespace fks_host {

class DeviceSuite {
 public:
  DeviceSuite(py::list engines, int n_slots = 4) {
    if (n_slots < 1 || n_slots > 64) throw std::invalid_argument("n_slots must be in [1, 64]");
    if (engines.empty()) throw std::invalid_argument("a suite needs at least one engine");
    for (py::handle h : engines) {
      DeviceEngine* e = h.cast<DeviceEngine*>();
      if (!eng_.empty() && e->device_ != eng_[0]->device_)
        throw std::invalid_argument("the engines of a suite must share one device");
      if (!e->rows_ok_) throw std::invalid_argument("the suite launch needs the row-kernel layout (<= 16 nodes)");
      if (!e->use_rows())
        throw std::invalid_argument("the suite launch needs engines whose programs run on the row layout "
                                    "(row_kernel off, invariant checks or repush = earliest)");
      eng_.push_back(e);
      refs_.push_back(py::reinterpret_borrow<py::object>(h));
    }
    device_ = eng_[0]->device_;
    HIP_OK(hipSetDevice(device_));
    const int T = (int)eng_.size();
    // block order: traces by descending pod count (stable: equal counts keep suite order)
    order_.resize(T);
    for (int t = 0; t < T; ++t) order_[t] = t;
    std::stable_sort(order_.begin(), order_.end(),
                     [&](int a, int b) { return eng_[a]->W_.n_pods > eng_[b]->W_.n_pods; });
    slots_.resize(n_slots);
    for (auto& s : slots_) {
      s = std::make_unique<SuiteSlot>();
      HIP_OK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
      HIP_OK(hipEventCreateWithFlags(&s->done, hipEventDisableTiming));
    }
  }

  ~DeviceSuite() {
    (void)hipSetDevice(device_);
    for (auto& s : slots_) {
      if (s->stream) (void)hipStreamSynchronize(s->stream);
      for (DevBuf* b : {&s->res, &s->gheap, &s->meta}) b->release();
      s->h_in.release();
      s->h_tab.release();
      s->h_meta.release();
      if (s->done) (void)hipEventDestroy(s->done);
      if (s->stream) (void)hipStreamDestroy(s->stream);
    }
  }

  // fn / kc / koff as for DeviceEngine::submit_native, P programs: every trace replays all of them
  void submit_native(int slot, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> fn,
                     py::array_t<int64_t, py::array::c_style | py::array::forcecast> kc,
                     py::array_t<int32_t, py::array::c_style | py::array::forcecast> koff) {
    SuiteSlot& s = slot_at(slot);
    if (s.busy) throw std::runtime_error("slot busy: wait() for its batch first");
    const int P = (int)fn.size(), T = (int)eng_.size();
    if (P < 1) throw std::invalid_argument("empty batch");
    if ((int)koff.size() != P) throw std::invalid_argument("koff must have one entry per policy");
    for (int i = 0; i < P; ++i) {
      if (fn.at(i) == 0) throw std::invalid_argument("null program pointer");
      if (koff.at(i) < 0 || koff.at(i) >= (int64_t)kc.size()) throw std::invalid_argument("koff out of range");
    }
    if ((int64_t)T * P > (int64_t)(1 << 30)) throw std::invalid_argument("grid too large");
    const uint32_t max_events = eng_[0]->max_events_;
    for (const DeviceEngine* e : eng_)
      if (e->max_events_ != max_events) throw std::invalid_argument("the engines of a suite must share max_events");
    const int G = T * P;
    HIP_OK(hipSetDevice(device_));
    HIP_OK(hipStreamSynchronize(s.stream));   // the previous batch no longer reads the staging
    // layout: every trace's heap top by its engine's rule with the whole grid in
    // flight; one dynamic-LDS size for the grid, the largest trace's
    std::vector<int> tops(T);
    size_t lds = 0;
    for (int t = 0; t < T; ++t) {
      tops[t] = eng_[t]->duo_top(G);
      lds = std::max(lds, duo_lds_bytes(eng_[t]->W_.n_pods, tops[t]));
    }
    if (lds > DeviceEngine::kMaxLds) throw std::invalid_argument("suite layout exceeds the 160 KiB LDS");
    std::vector<uint64_t> heap_off(T);
    uint64_t words = 0;
    for (int t = 0; t < T; ++t) {
      heap_off[t] = words;
      words += (uint64_t)row_heap_entries(eng_[t]->W_.n_pods) * (uint64_t)P;
    }
    s.gheap.reserve((size_t)words * 8);
    s.res.reserve(sizeof(DevResult) * (size_t)G);
    s.h_tab.reserve(sizeof(double) * 13 * (size_t)G);
    // the workload table | order | heap offsets in HBM: rebuilt only when the layout changes
    const size_t tab_bytes = (sizeof(DevWorkload) * (size_t)T + 63) & ~size_t(63);
    const size_t ord_bytes = ((size_t)T * 4 + 63) & ~size_t(63);
    const size_t meta_bytes = tab_bytes + ord_bytes + (size_t)T * 8;
    if (tops != s.tops || P != s.meta_P) {
      s.h_meta.reserve(meta_bytes);
      s.meta.reserve(meta_bytes);
      char* h = s.h_meta.as<char>();
      std::memset(h, 0, meta_bytes);
      for (int t = 0; t < T; ++t) {
        DevWorkload Wl = eng_[t]->W_;
        Wl.heap_top = tops[t];
        std::memcpy(h + sizeof(DevWorkload) * (size_t)t, &Wl, sizeof(DevWorkload));
      }
      std::memcpy(h + tab_bytes, order_.data(), (size_t)T * 4);
      std::memcpy(h + tab_bytes + ord_bytes, heap_off.data(), (size_t)T * 8);
      HIP_OK(hipMemcpyAsync(s.meta.p, h, meta_bytes, hipMemcpyHostToDevice, s.stream));
      s.tops = tops;
      s.meta_P = P;
    }
    // fn | koff | kc, read by the kernel straight from pinned host memory (as DeviceEngine stages them;
    // the kernel reads kKcLds entries from every block start, hence the pad)
    const size_t fb = (size_t)P * 8, ob = (size_t)P * 4, kb = (size_t)kc.size() * 8;
    const size_t kco = (fb + ob + 63) & ~size_t(63);
    s.h_in.reserve(kco + kb + (size_t)kKcLds * 8 + 64);
    std::memcpy(s.h_in.as<char>(), fn.data(), fb);
    std::memcpy(s.h_in.as<char>() + fb, koff.data(), ob);
    std::memcpy(s.h_in.as<char>() + kco, kc.data(), kb);
    std::memset(s.h_in.as<char>() + kco + kb, 0, (size_t)kKcLds * 8);
    s.P = P;
    {
      py::gil_scoped_release rel;
      const char* m = s.meta.as<char>();
      const fksk::SuiteArgs a{reinterpret_cast<const DevWorkload*>(m), reinterpret_cast<const int32_t*>(m + tab_bytes),
                              T, P, reinterpret_cast<const uint64_t*>(m + tab_bytes + ord_bytes),
                              s.res.as<DevResult>(), s.gheap.as<uint64_t>(), s.h_tab.dev<double>()};
      const RowNativeArgs nat{s.h_in.dev<const uint64_t>(), reinterpret_cast<const int64_t*>(s.h_in.dev<char>() + kco),
                              reinterpret_cast<const int32_t*>(s.h_in.dev<char>() + fb), nullptr, max_events};
      if (std::getenv("FKS_DEBUG_LAUNCH"))
        std::fprintf(stderr, "[fks] native duo suite: T=%d P=%d lds=%zu stream=%p\n", T, P, lds, (void*)s.stream);
      s.range = roctxRangeStartA("fks.batch.native_suite");
      HIP_OK(fksk::launch_native_duo_suite(G, lds, s.stream, a, nat));
      HIP_OK(hipEventRecord(s.done, s.stream));
      s.busy = true;
    }
    last_tops_ = tops;
    last_lds_ = lds;
    last_grid_ = G;
  }

  bool ready(int slot) {
    SuiteSlot& s = slot_at(slot);
    if (!s.busy) return true;
    const hipError_t e = hipEventQuery(s.done);
    if (e == hipErrorNotReady) return false;
    HIP_OK(e);
    return true;
  }

  // [T, P, 13] result tables of the batch in flight on `slot`
  py::array_t<double> wait(int slot) {
    SuiteSlot& s = slot_at(slot);
    if (!s.busy) throw std::invalid_argument("slot has no batch in flight");
    {
      py::gil_scoped_release rel;
      HIP_OK(hipEventSynchronize(s.done));
    }
    s.busy = false;
    if (s.range) roctxRangeStop(s.range);
    s.range = 0;
    py::array_t<double> out({(py::ssize_t)eng_.size(), (py::ssize_t)s.P, (py::ssize_t)13});
    std::memcpy(out.mutable_data(), s.h_tab.p, sizeof(double) * 13 * eng_.size() * (size_t)s.P);
    return out;
  }

  py::dict info() const {
    py::dict d;
    d["T"] = (int)eng_.size();
    d["n_slots"] = (int)slots_.size();
    d["order"] = order_;
    d["tops"] = last_tops_;               // per trace, of the last launch
    d["lds"] = (int64_t)last_lds_;
    d["per_cu"] = last_grid_ ? fksk::native_duo_suite_blocks_per_cu(last_lds_) : 0;   // workgroups per CU at that LDS
    d["reg_cap"] = fksk::native_duo_suite_blocks_per_cu(0);
    d["grid"] = last_grid_;
    d["num_cus"] = eng_[0]->num_cus_;
    return d;
  }

  int n_slots() const { return (int)slots_.size(); }

 private:
  struct SuiteSlot {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    DevBuf res, gheap, meta;          // DevResult[T * P]; heap areas; workload table | order | heap offsets
    HostBuf h_in, h_tab, h_meta;      // fn | koff | kc; [T * P, 13]; staging of meta
    std::vector<int> tops;            // the layout `meta` holds
    int meta_P = 0;
    int P = 0;
    bool busy = false;
    roctx_range_id_t range = 0;
  };

  SuiteSlot& slot_at(int i) {
    if (i < 0 || i >= (int)slots_.size()) throw std::out_of_range("slot index");
    return *slots_[i];
  }

  int device_ = 0;
  std::vector<DeviceEngine*> eng_;
  std::vector<py::object> refs_;      // keep the engines (and the traces' device arrays) alive
  std::vector<int32_t> order_;
  std::vector<std::unique_ptr<SuiteSlot>> slots_;
  std::vector<int> last_tops_;
  size_t last_lds_ = 0;
  int last_grid_ = 0;
};

}  // namespace fks_host
