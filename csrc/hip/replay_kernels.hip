// Replay kernels: one wave64 workgroup per candidate policy.
//
// Compiled once per (FKS_KIND, FKS_NPASS) by ops/build.py:
//   FKS_KIND 0 -> built-in family kernels for FKS_NPASS (one instance per family + a mixed one)
//   FKS_KIND 1 -> bytecode-VM kernels for FKS_NPASS
//   FKS_KIND 2 -> phase-profiled diagnostics kernels (NPASS = 1)
//   FKS_KIND 3 -> row kernels (4 policies per wave, <= 16 nodes; replay_rows.hip.h)
//   FKS_KIND 4 -> native-program kernels (JIT-compiled scorers called through
//                 function pointers; jit_abi.h) for FKS_NPASS
// Each unit lists its kernels in tables ({key, kernel} rows, one table per
// group of instances) and defines the matching launchers of launch.h on them.
#include <hip/hip_runtime.h>

#include <array>

#include "launch.h"
#include "replay.hip.h"
#include "scorers.hip.h"
#include "vm_dev.hip.h"
#include "replay_rows.hip.h"
#include "replay_duo.hip.h"
#include "replay_wave_duo.hip.h"

namespace {
// The launch's workload struct as the kernel received it: every kernel's
// first parameter is an argument struct whose first member is the
// DevWorkload, so it sits at offset 0 of the kernarg segment.  The kernels
// re-read their cold fields from there with scalar loads -- no per-slot HBM
// copy, hence no copy kernel that would have to wait for a CU slot behind
// the other slots' persistent replay waves (~1 s at config-5 shape).
// (`&a.W` would not do: taking a by-value parameter's address makes clang
// copy the struct to scratch.)
__device__ __forceinline__ const fksd::DevWorkload* kernarg_workload() {
  // constant (4) -> flat: the same 64-bit address (the kernarg segment is ordinary global memory)
  return reinterpret_cast<const fksd::DevWorkload*>((uintptr_t)__builtin_amdgcn_kernarg_segment_ptr());
}
static_assert(offsetof(fksk::BuiltinArgs, W) == 0, "DevWorkload must open the kernel arguments");
static_assert(offsetof(fksk::VmArgs, W) == 0, "DevWorkload must open the kernel arguments");
static_assert(offsetof(fksk::NativeArgs, W) == 0, "DevWorkload must open the kernel arguments");
}  // namespace
#include "jit_abi.h"

#ifndef FKS_KIND
#define FKS_KIND 0
#endif
#ifndef FKS_NPASS
#define FKS_NPASS 1
#endif
#ifndef FKS_WAVE_FLAT
#define FKS_WAVE_FLAT 1   // HBM-heap wave kernels: flat heap accesses (heap_wave.h WaveHeapT)
#endif

using namespace fksd;

namespace {

// Where a policy's heap, deletion bitmap and VM registers live.
//   GHEAP = false: LDS = heap | bitmap | vregs (2 policies/CU on the 8k trace)
//   GHEAP = true : heap in its HBM slice, LDS = bitmap | heap top (W.heap_top
//                  slots) | vregs (16 policies/CU)
struct Slot {
  FKS_GLOBAL uint64_t* h;
  FKS_LDS uint64_t* top;
  int T;
  FKS_LDS uint32_t* delmap;
  uint64_t* vregs;
  FKS_LDS int32_t* inv;   // invariant-check scratch (debug; unused when off)
};
template <bool GHEAP>
__device__ __forceinline__ Slot policy_slot(const DevWorkload& W, uint64_t* gheap, int p) {
  extern __shared__ uint64_t lds_raw[];
  FKS_LDS uint64_t* lds0 = lds_ptr(lds_raw);
  // [invariant scratch | kWeights words (reserved) | policy layout]
  FKS_LDS uint64_t* lds = lds0 + W.inv_words + kWeights;
  const int N = W.n_pods;
  Slot s;
  s.inv = reinterpret_cast<FKS_LDS int32_t*>(lds0);
  if (GHEAP) {
    // the deletion bitmap covers the first W.delmap_slots slots (a multiple of 64)
    const int dw = W.delmap_slots >> 5;
    s.h = global_ptr(gheap + (size_t)p * lds_heap_entries(N));
    s.delmap = reinterpret_cast<FKS_LDS uint32_t*>(lds);
    s.top = lds + dw / 2;
    s.T = W.heap_top;
    s.vregs = lds_raw + W.inv_words + kWeights + dw / 2 + W.heap_top;
  } else {
    s.h = global_ptr(gheap);   // never dereferenced: T covers the whole heap
    s.top = lds;
    s.T = lds_heap_entries(N);
    s.delmap = reinterpret_cast<FKS_LDS uint32_t*>(lds + lds_heap_entries(N));
    s.vregs = lds_raw + W.inv_words + kWeights + lds_vreg_offset(N);
  }
  return s;
}

// Waves per SIMD the kernel is compiled for: the LDS-heap variant is LDS-bound at
// 2 waves/CU anyway; the HBM-heap variant trades registers for occupancy.
#define FKS_BOUNDS(G) __launch_bounds__(64, (G) ? 4 : 1)
#define FKS_VM_BOUNDS(G) __launch_bounds__(64, (G) ? FKS_VM_WAVES : 1)

// Prologue: the batch's family ids / weights live in pinned host memory
// (zero-copy, no copy kernel queued behind busy CUs); each policy moves its 16
// weights into its slot of a device buffer once, which the scorer then reads
// through the scalar cache.
template <int FAM>
__device__ __forceinline__ void load_policy(BuiltinScorerDev<FAM>& sc, const fksk::BuiltinArgs& a, int p) {
  const int lane = lane_id();
  double* wd = a.wdev + (size_t)p * kWeights;
  if (lane < kWeights) wd[lane] = a.weights[(size_t)p * kWeights + lane];
  const int fam = uni(lane == 0 ? a.fam[p] : 0);
  __threadfence();   // stores visible to the scalar loads that follow
  sc.load(fam, wd);
  sc.zp = a.W.node_recip;
  sc.capz = kernarg_workload()->cap_recip;
}

// ---- kernel tables ------------------------------------------------------------------------
// A group of kernel instances is a table of rows {key, kernel}; the key is the
// family code, the heap flag or the profiled flag.  A key the table does not
// have takes its last row.  Every launch, LDS-limit and occupancy call of this
// file goes through the three helpers below, so a kernel is named twice: where
// it is defined and in its table.
template <class... A>
struct Row {
  int key;
  void (*kernel)(A...);
};
template <class... A, size_t N>
auto row_kernel(const std::array<Row<A...>, N>& table, int key) {
  for (const Row<A...>& r : table)
    if (r.key == key) return r.kernel;
  return table.back().kernel;
}
template <class Table, class... A>
hipError_t launch_row(const Table& table, int key, dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
  const auto kernel = row_kernel(table, key);
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  return hipGetLastError();
}
// the dynamic-LDS limit of every kernel of the tables, up to the first error
template <class Table>
hipError_t raise_lds(int max_lds, const Table& table) {
  for (const auto& r : table) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(r.kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
template <class Table, class... More>
hipError_t raise_lds(int max_lds, const Table& table, const More&... more) {
  const hipError_t e = raise_lds(max_lds, table);
  return e != hipSuccess ? e : raise_lds(max_lds, more...);
}
// resident workgroups of `block` threads per CU for a key's kernel at `lds` bytes (-1: error)
template <class Table>
int blocks_per_cu(const Table& table, int key, int block, size_t lds) {
  int n = 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, row_kernel(table, key), block, lds) == hipSuccess ? n : -1;
}
// the keys of a table whose rows are the instances of one kernel template
template <int... K>
struct Keys {};
// the mixed-batch instance last: the row of an unknown family code
using Families = Keys<FAM_FIRST_FIT, FAM_BEST_FIT, FAM_RANDOM_LINEAR, FAM_FEATURE_LINEAR, FAM_COMPOSITE_LINEAR, -1>;
using Heaps = Keys<1, 0>;   // GHEAP: HBM heap, LDS heap

#if FKS_KIND == 0
#define FKS_FAM_BOUNDS(G, F, NP)                                                           \
  __launch_bounds__(64, !(G) ? 1 : (NP) >= 4 ? FKS_NP4_WAVES : (NP) == 2 ? FKS_NP2_WAVES   \
                           : (((F) == 3 || (F) == 4 || (F) < 0) ? FKS_HEAVY_WAVES : FKS_LIGHT_WAVES))
template <int NPASS, bool GHEAP, int FAM>
__global__ FKS_FAM_BOUNDS(GHEAP, FAM, NPASS) void k_replay_builtin(fksk::BuiltinArgs a) {
  const int p = blockIdx.x;
  const Slot s = policy_slot<GHEAP>(a.W, a.gheap, p);
  BuiltinScorerDev<FAM> sc;
  load_policy<FAM>(sc, a, p);
  replay_one<NPASS, BuiltinScorerDev<FAM>, NoProf, GHEAP && FKS_WAVE_FLAT>(a.W, kernarg_workload(), sc, s.h, s.top, s.T,
                                                                           s.delmap, s.inv, a.out + p);
}

template <bool GHEAP, int... F>
constexpr std::array<Row<fksk::BuiltinArgs>, sizeof...(F)> builtin_rows(Keys<F...>) {
  return {{{F, k_replay_builtin<FKS_NPASS, GHEAP, F>}...}};
}
#endif

#if FKS_KIND == 0
// Schedule mode: the mixed-family, HBM-heap instance that also stores every
// commit's record (rec: [P, n_pods], a trailing parameter -- the arguments of
// the instances above do not move).
template <int NPASS>
__global__ FKS_FAM_BOUNDS(true, -1, NPASS) void k_replay_builtin_sched(fksk::BuiltinArgs a, SchedRec* rec) {
  const int p = blockIdx.x;
  const Slot s = policy_slot<true>(a.W, a.gheap, p);
  BuiltinScorerDev<-1> sc;
  load_policy<-1>(sc, a, p);
  replay_one<NPASS, BuiltinScorerDev<-1>, NoProf, FKS_WAVE_FLAT != 0, SchedSink>(
      a.W, kernarg_workload(), sc, s.h, s.top, s.T, s.delmap, s.inv, a.out + p, nullptr,
      SchedSink{rec + (size_t)p * a.W.n_pods});
}
constexpr std::array<Row<fksk::BuiltinArgs, SchedRec*>, 1> kBuiltinSched = {
    {{0, k_replay_builtin_sched<FKS_NPASS>}}};
// Time-metrics mode: the mixed-family, HBM-heap instance that also carries the
// policy's TimeAcc and writes trec[p] (a trailing parameter, as above).
template <int NPASS>
__global__ FKS_FAM_BOUNDS(true, -1, NPASS) void k_replay_builtin_time(fksk::BuiltinArgs a, TimeRec* trec) {
  const int p = blockIdx.x;
  const Slot s = policy_slot<true>(a.W, a.gheap, p);
  BuiltinScorerDev<-1> sc;
  load_policy<-1>(sc, a, p);
  replay_one<NPASS, BuiltinScorerDev<-1>, NoProf, FKS_WAVE_FLAT != 0, NoSched, TimeSink>(
      a.W, kernarg_workload(), sc, s.h, s.top, s.T, s.delmap, s.inv, a.out + p, nullptr, NoSched{}, TimeSink{trec + p});
}
constexpr std::array<Row<fksk::BuiltinArgs, TimeRec*>, 1> kBuiltinTime = {
    {{0, k_replay_builtin_time<FKS_NPASS>}}};
#endif

#if FKS_KIND == 0 && FKS_NPASS == 4
// 256-node clusters, HBM heap: heap wave + scoring wave per policy
// (replay_wave_duo.hip.h); both waves share the register allocation of the
// scoring wave, FKS_NP4_DUO_WAVES waves per SIMD (launch.h)
template <int FAM>
__global__ __launch_bounds__(128, FKS_NP4_DUO_WAVES) void k_replay_builtin_duo(fksk::BuiltinArgs a) {
  const int p = blockIdx.x;
  const Slot s = policy_slot<true>(a.W, a.gheap, p);
  BuiltinScorerDev<FAM> sc;
  if (threadIdx.x >= kWave) load_policy<FAM>(sc, a, p);   // the scoring wave's weights
  FKS_LDS DuoBox* box = reinterpret_cast<FKS_LDS DuoBox*>(lds_ptr(s.vregs));
  replay_wave_duo<4, BuiltinScorerDev<FAM>, FKS_WAVE_FLAT>(a.W, kernarg_workload(), sc, s.h, s.top, s.T, s.delmap,
                                                            box, a.out + p);
}

template <int... F>
constexpr std::array<Row<fksk::BuiltinArgs>, sizeof...(F)> builtin_duo_rows(Keys<F...>) {
  return {{{F, k_replay_builtin_duo<F>}...}};
}
constexpr auto kBuiltinDuo = builtin_duo_rows(Families{});
#endif
#if FKS_KIND == 0
constexpr auto kBuiltinHbm = builtin_rows<true>(Families{});
constexpr auto kBuiltinLds = builtin_rows<false>(Families{});
#endif

#if FKS_KIND == 1
template <int NPASS, bool GHEAP>
__global__ FKS_VM_BOUNDS(GHEAP) void k_replay_vm(fksk::VmArgs a) {
  const int p = blockIdx.x;
  const Slot s = policy_slot<GHEAP>(a.W, a.gheap, p);
  VmScorerDev sc;
  sc.init(a.T, p, a.W, a.budget, s.vregs);
  replay_one<NPASS>(a.W, kernarg_workload(), sc, s.h, s.top, s.T, s.delmap, s.inv, a.out + p);
}
template <int... G>
constexpr std::array<Row<fksk::VmArgs>, sizeof...(G)> vm_rows(Keys<G...>) {
  return {{{G, k_replay_vm<FKS_NPASS, G != 0>}...}};
}
constexpr auto kVm = vm_rows(Heaps{});
#endif

#if FKS_KIND == 2
template <bool GHEAP>
__global__ FKS_BOUNDS(GHEAP) void k_replay_builtin_prof(fksk::BuiltinArgs a) {
  const int p = blockIdx.x;
  const Slot s = policy_slot<GHEAP>(a.W, a.gheap, p);
  BuiltinScorerDev<-1> sc;
  load_policy<-1>(sc, a, p);
  replay_one<1, BuiltinScorerDev<-1>, PhaseProf>(a.W, kernarg_workload(), sc, s.h, s.top, s.T, s.delmap, s.inv, a.out + p,
                                                 a.prof + (size_t)p * 8);
}

// 256-node clusters: the production composite instance (4 node slots per
// lane, HBM heap, same launch bounds) with the s_memtime phase profiler
__global__ __launch_bounds__(64, FKS_NP4_WAVES) void k_replay_c5_prof(fksk::BuiltinArgs a) {
  const int p = blockIdx.x;
  const Slot s = policy_slot<true>(a.W, a.gheap, p);
  BuiltinScorerDev<FAM_COMPOSITE_LINEAR> sc;
  load_policy<FAM_COMPOSITE_LINEAR>(sc, a, p);
  replay_one<4, BuiltinScorerDev<FAM_COMPOSITE_LINEAR>, PhaseProf, FKS_WAVE_FLAT>(
      a.W, kernarg_workload(), sc, s.h, s.top, s.T, s.delmap, s.inv, a.out + p, a.prof + (size_t)p * 8);
}

template <bool GHEAP>
__global__ FKS_VM_BOUNDS(GHEAP) void k_replay_vm_prof(fksk::VmArgs a) {
  const int p = blockIdx.x;
  const Slot s = policy_slot<GHEAP>(a.W, a.gheap, p);
  VmScorerDev sc;
  sc.init(a.T, p, a.W, a.budget, s.vregs);
  replay_one<1, VmScorerDev, PhaseProf>(a.W, kernarg_workload(), sc, s.h, s.top, s.T, s.delmap, s.inv, a.out + p, a.prof + (size_t)p * 8);
}
template <int... G>
constexpr std::array<Row<fksk::BuiltinArgs>, sizeof...(G)> builtin_prof_rows(Keys<G...>) {
  return {{{G, k_replay_builtin_prof<G != 0>}...}};
}
template <int... G>
constexpr std::array<Row<fksk::VmArgs>, sizeof...(G)> vm_prof_rows(Keys<G...>) {
  return {{{G, k_replay_vm_prof<G != 0>}...}};
}
constexpr auto kBuiltinProf = builtin_prof_rows(Heaps{});
constexpr auto kVmProf = vm_prof_rows(Heaps{});
constexpr std::array<Row<fksk::BuiltinArgs>, 1> kC5Prof = {{{0, k_replay_c5_prof}}};
#endif


#if FKS_KIND == 3
// Row kernels (waves per SIMD: FKS_ROW_WAVES / FKS_ROW_HEAVY_WAVES, launch.h)
template <int FAM>
__global__ __launch_bounds__(64, FAM < 0 ? 2 : (FAM == 3 || FAM == 4) ? FKS_ROW_HEAVY_WAVES : FKS_ROW_WAVES) void k_replay_rows(fksk::BuiltinArgs a, int P, uint32_t* queue, uint32_t qbase) {
  replay_rows<FAM>(a.W, kernarg_workload(), a.fam, a.weights, a.gheap, a.out, P, queue, qbase, nullptr,
                   RowNativeArgs{nullptr, nullptr, nullptr}, kRowsPerWave, a.table);
}
// The composite instance at 5 waves per SIMD (<= 96 VGPRs, a few loop-invariant
// spills): host family code kRowCompositeW5 (`row_composite_waves` option).
__global__ __launch_bounds__(64, 5) void k_replay_rows_c5(fksk::BuiltinArgs a, int P, uint32_t* queue, uint32_t qbase) {
  replay_rows<FAM_COMPOSITE_LINEAR>(a.W, kernarg_workload(), a.fam, a.weights, a.gheap, a.out, P, queue, qbase, nullptr,
                                    RowNativeArgs{nullptr, nullptr, nullptr}, kRowsPerWave, a.table);
}
__global__ __launch_bounds__(64, FKS_ROW_HEAVY_WAVES) void k_replay_rows_split(fksk::BuiltinArgs a, int P, uint32_t* queue,
                                                                               uint32_t qbase) {
  replay_rows<FAM_COMPOSITE_LINEAR, RowNoProf, false>(a.W, kernarg_workload(), a.fam, a.weights, a.gheap, a.out, P, queue,
                                                      qbase, nullptr, RowNativeArgs{nullptr, nullptr, nullptr}, kRowsPerWave,
                                                      a.table);
}
template <int FAM>
__global__ __launch_bounds__(64, FAM < 0 ? 2 : (FAM == 3 || FAM == 4) ? FKS_ROW_HEAVY_WAVES : FKS_ROW_WAVES)
void k_replay_rows_prof(fksk::BuiltinArgs a, int P, uint32_t* queue, uint32_t qbase) {
  replay_rows<FAM, RowProf>(a.W, kernarg_workload(), a.fam, a.weights, a.gheap, a.out, P, queue, qbase, a.prof,
                            RowNativeArgs{nullptr, nullptr, nullptr}, kRowsPerWave, a.table);
}
// Schedule mode: the mixed-family instance that also stores every commit's record (rec: [P, n_pods])
__global__ __launch_bounds__(64, 2) void k_replay_rows_sched(fksk::BuiltinArgs a, int P, uint32_t* queue, uint32_t qbase,
                                                             SchedRec* rec) {
  replay_rows<-1, RowNoProf, FKS_ROW_FLAT != 0, true>(a.W, kernarg_workload(), a.fam, a.weights, a.gheap, a.out, P, queue,
                                                      qbase, nullptr, RowNativeArgs{nullptr, nullptr, nullptr},
                                                      kRowsPerWave, a.table, rec);
}
constexpr std::array<Row<fksk::BuiltinArgs, int, uint32_t*, uint32_t, SchedRec*>, 1> kRowsSched = {
    {{0, k_replay_rows_sched}}};
// Time-metrics mode: every row carries its policy's TimeAcc and writes trec[p].
// The composite instance at the waves per SIMD of k_replay_rows_c5 (the default
// launch's composite instance), the mixed one as k_replay_rows<-1>.
#ifndef FKS_ROW_TIME_WAVES
#define FKS_ROW_TIME_WAVES 5
#endif
template <int FAM>
__global__ __launch_bounds__(64, FAM < 0 ? 2 : FKS_ROW_TIME_WAVES) void k_replay_rows_time(fksk::BuiltinArgs a, int P,
                                                                                         uint32_t* queue, uint32_t qbase,
                                                                                         TimeRec* trec) {
  replay_rows<FAM, RowNoProf, FKS_ROW_FLAT != 0, false, true>(a.W, kernarg_workload(), a.fam, a.weights, a.gheap, a.out, P,
                                                               queue, qbase, nullptr,
                                                               RowNativeArgs{nullptr, nullptr, nullptr}, kRowsPerWave,
                                                               a.table, nullptr, trec);
}
constexpr std::array<Row<fksk::BuiltinArgs, int, uint32_t*, uint32_t, TimeRec*>, 2> kRowsTime = {
    {{FAM_COMPOSITE_LINEAR, k_replay_rows_time<FAM_COMPOSITE_LINEAR>}, {-1, k_replay_rows_time<-1>}}};
using RowsRow = Row<fksk::BuiltinArgs, int, uint32_t*, uint32_t>;
template <int... F>
constexpr std::array<RowsRow, sizeof...(F) + 2> rows_rows(Keys<F...>) {
  return {{{kRowCompositeW5, k_replay_rows_c5}, {kRowCompositeSplit, k_replay_rows_split}, {F, k_replay_rows<F>}...}};
}
template <int... F>
constexpr std::array<RowsRow, sizeof...(F)> rows_prof_rows(Keys<F...>) {
  return {{{F, k_replay_rows_prof<F>}...}};
}
constexpr auto kRows = rows_rows(Families{});
// the profiled builds: random_linear, the one composite build, and the mixed instance for every other family
constexpr auto kRowsProf = rows_prof_rows(Keys<FAM_RANDOM_LINEAR, FAM_COMPOSITE_LINEAR, -1>{});
#endif


#if FKS_KIND == 4
// Scorer of natively compiled programs: one indirect call per node pass to the
// policy's JIT function (wave-uniform pointer -> a plain s_swappc).
struct NativeScorerDev {
  ProgFn fn;
  bool feas;             // the program opens with the feasibility prologue (jit_abi.h kFnFeasBit):
                         // called for feasible nodes only -- its JIT code may lack the prologue
  const int64_t* gmem;   // [node][kGmax] GPU memory MiB
  KcPtr kc;              // the policy's [budget, constants...], staged in LDS
  template <int NPASS, bool GP>
  __device__ int64_t score(int ps, const NodeRegs<NPASS, GP>& nr, const PodView& pod, int& exc) {
    if (feas && !feasible<NPASS, GP>(ps, nr, pod)) return 0;
    const int node = ps * kWave + lane_id();
    return call_prog(fn, nr, ps, pod, gmem + (size_t)node * kGmax, kc, exc);
  }
};

// Register floor: an address-taken function touching v127 / s101 raises this
// unit's amdgpu.max_num_vgpr / max_num_sgpr, and with them the allocation of
// every kernel here that makes an indirect call, to what JIT-compiled
// programs may use (kJitVgprs / kJitSgprs, checked by ops/jit.py).
__device__ __noinline__ int64_t fks_reg_floor(int64_t a) {
  asm volatile("" ::: "v127", "s101");
  return a;
}

// Runtime library of native programs (jit_abi.h rt_binop / rt_unop): the
// exact float //, %, **, math.log / exp / sqrt / pow of the device VM.
extern "C" __device__ __noinline__ Ret2 fks_rt_binop(int op, int64_t ab, int32_t afl, int64_t bb, int32_t bfl) {
  return d_binop_s(op, ab, afl, bb, bfl);
}
extern "C" __device__ __noinline__ Ret2 fks_rt_unop(int op, int64_t ab, int32_t afl) { return d_unop_s(op, ab, afl); }

__global__ void k_native_rt_table(uint64_t* out) {
  if (threadIdx.x == 0) {
    out[0] = (uint64_t)&fks_rt_binop;
    out[1] = (uint64_t)&fks_rt_unop;
    out[2] = (uint64_t)&fks_reg_floor;
    out[3] = 0;
  }
}

#if FKS_NPASS == 1
// Row kernel with natively compiled programs (replay_rows.hip.h, kFamNative):
// clusters of <= 16 nodes; `rows_active` rows per wave claim programs (1 for
// latency-bound LLM-sized batches, 4 for large ones).
__global__ __launch_bounds__(64, 1) void k_replay_rows_native(fksk::BuiltinArgs a, RowNativeArgs nat, int P,
                                                             uint32_t* queue, uint32_t qbase, int rows_active) {
  replay_rows<kFamNative>(a.W, kernarg_workload(), nullptr, nullptr, a.gheap, a.out, P, queue, qbase, nullptr, nat, rows_active,
                          a.table);
}
// s_memtime phase-profiled build (diagnostics): a.prof = [waves, 8] cycles
__global__ __launch_bounds__(64, 1) void k_replay_rows_native_prof(fksk::BuiltinArgs a, RowNativeArgs nat, int P,
                                                                  uint32_t* queue, uint32_t qbase, int rows_active) {
  replay_rows<kFamNative, RowProf>(a.W, kernarg_workload(), nullptr, nullptr, a.gheap, a.out, P, queue, qbase, a.prof, nat,
                                   rows_active, a.table);
}
// Two waves per program (wave 0: heap, wave 1: scoring; replay_duo.hip.h).
__global__ __launch_bounds__(128, 1) void k_replay_native_duo(fksk::BuiltinArgs a, RowNativeArgs nat) {
  replay_duo<false>(a.W, kernarg_workload(), a.gheap, a.out, nat, a.table);
}
// s_memtime-profiled build (diagnostics): a.prof = [blocks, 2 waves, 8] cycles
__global__ __launch_bounds__(128, 1) void k_replay_native_duo_prof(fksk::BuiltinArgs a, RowNativeArgs nat) {
  replay_duo<true>(a.W, kernarg_workload(), a.gheap, a.out, nat, a.table, a.prof);
}
// Schedule mode: the scoring wave also stores every placed pod's record (rec: [P, n_pods])
__global__ __launch_bounds__(128, 1) void k_replay_native_duo_sched(fksk::BuiltinArgs a, RowNativeArgs nat, SchedRec* rec) {
  replay_duo<false, true>(a.W, kernarg_workload(), a.gheap, a.out, nat, a.table, nullptr, -1, -1, rec);
}
// Time-metrics mode: the scoring wave carries the program's TimeAcc and writes trec[p]
__global__ __launch_bounds__(128, 1) void k_replay_native_duo_time(fksk::BuiltinArgs a, RowNativeArgs nat, TimeRec* trec) {
  replay_duo<false, false, true>(a.W, kernarg_workload(), a.gheap, a.out, nat, a.table, nullptr, -1, -1, nullptr, trec);
}
// ----------------------------------------------------------------------------
// The resident program service: a resident pool of two-wave workgroups that replays
// native programs from a ring the host keeps filling, one program after the
// other per workgroup -- a program's replay ends, its workgroup takes the next
// one.  A batch launch instead holds every one of its CU slots until its
// longest replay is done (the tail of a launch: ~40% mean occupancy on evolved
// programs, and one slow program pinned a 512-program slot in the steady loop).
//
// Host <-> device protocol (host memory: fine-grained, mapped; `claimed` in HBM):
//   the host writes program i into a free data slot s (fn, kc block, koff),
//   qslot[i % nq] = s, then publishes `published` = i + 1 (release); a
//   workgroup claims the next index from `claimed` (atomic), waits until it is
//   published, reads s, marks started[i % nq] = i + 1, replays slot s, writes
//   its result row and then done[s] = i + 1 (system-scope release).  The host
//   frees a slot when it consumed the row, and reuses a queue entry only once
//   it is marked started -- a straggler holds its slot, nothing else.
//   Exit: `stop` set and nothing left to claim, or `max_idle_polls` polls with
//   nothing published (a lost host: the whole grid drains instead of spinning
//   on; the host relaunches it from the lowest unstarted index).
//
// The replay is a call (service_replay, not inlined): inlined into the service
// loop, values of its prologue and epilogue were hoisted out of the loop and
// kept live across every event -- 144-156 VGPRs (6 workgroups per CU) against
// the 128 of the two-wave batch kernel.  Called, it reads every argument from the
// kernarg segment afresh and the kernel holds the two-wave kernel's 8 per CU
// (a 224 B stack frame: the callee-saved registers, saved once per program).
constexpr uint32_t kServiceExit = 0xFFFFFFFFu;

// The kernarg segment pointer exists in the kernel only (a callee reading
// __builtin_amdgcn_kernarg_segment_ptr gets null): the kernel passes it down,
// the callees make it wave-uniform again (scalar loads of the arguments).
__device__ __forceinline__ const FKS_CONST fksk::ServiceArgs* service_args(uint64_t kp) {
  return (const FKS_CONST fksk::ServiceArgs*)uniu64(kp);
}

__device__ __forceinline__ void service_replay_body(uint64_t kp, int slot) {
  const FKS_CONST fksk::ServiceArgs* A = service_args(kp);
  const fksd::DevWorkload& W = *(const fksd::DevWorkload*)&A->a.W;
  const RowNativeArgs nat{A->nat.fn, A->nat.kc, A->nat.koff, A->nat.abort, A->nat.max_events};
  replay_duo<false>(W, (const fksd::DevWorkload*)uniu64(kp), A->a.gheap, A->a.out, nat, A->a.table, nullptr, slot,
                    (int)blockIdx.x);
}

// Claim the next index and wait until it is published.  Only the workgroups
// at the front (within kServiceFront of the HBM mirror of `published`) read
// the host's counter -- thousands of waiting workgroups polling host memory
// (one PCIe read each) starved the link and the replays' own host traffic --
// and advance the mirror; the rest poll the mirror (HBM, device scope),
// sleeping longer the further their index lies ahead.  Every index below the
// mirror is published, and the lowest unprocessed index is always claimed by
// a front workgroup (claims are handed out in order), so the mirror advances
// whenever the host publishes.  `stop` propagates the same way.
constexpr uint32_t kServiceFront = 2;

__device__ __noinline__ void service_replay(uint64_t kp, int slot) { service_replay_body(kp, slot); }

// The queued program's data slot (its index-queue entry, then marked started
// so the host may reuse the entry), or kServiceExit; an index a previous
// launch already started (a relaunch after an idle drain) is skipped.
__device__ __forceinline__ uint32_t service_entry(const FKS_CONST ServiceCtl& c, uint32_t idx, uint32_t* slot) {
  const uint32_t e = idx % c.nq;
  if (__hip_atomic_load(&c.started[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == idx + 1u) return 0u;
  *slot = __hip_atomic_load(&c.qslot[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&c.started[e], idx + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return 1u;
}

__device__ __noinline__ uint32_t service_claim(uint64_t kp, uint32_t* slot) {
  const FKS_CONST ServiceCtl& c = service_args(kp)->c;
  uint32_t* mirror = c.claimed + 32;   // HBM: published (lower bound), then stop
  uint32_t* stopd = c.claimed + 64;
  uint32_t idx = __hip_atomic_fetch_add(c.claimed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t polls = 0;
  for (;;) {
    uint32_t pub = __hip_atomic_load(mirror, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    if ((int32_t)(idx - pub) < 0) {   // published (wrap-safe)
      // (the mirror's acquire orders this after the host's queue writes: the
      // front workgroup that advanced it acquired them at system scope)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
      if (service_entry(c, idx, slot)) return idx;
      idx = __hip_atomic_fetch_add(c.claimed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    if (__hip_atomic_load(stopd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return kServiceExit;
    if (idx - pub < kServiceFront) {
      const uint32_t hp = __hip_atomic_load(c.published, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
      if ((int32_t)(hp - pub) > 0) {
        __hip_atomic_fetch_max(mirror, hp, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        continue;   // published now: take it through the path above
      }
      if (__hip_atomic_load(c.stop, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) {
        __hip_atomic_store(stopd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return kServiceExit;
      }
    }
    const uint32_t d = idx - pub + 1u < 32u ? idx - pub + 1u : 32u;
    for (uint32_t z = d; z > 0; --z) __builtin_amdgcn_s_sleep(127);
    polls += d;
    if (polls > c.max_idle_polls) {
      // idle drain, all or nothing: every workgroup leaves (the stop mirror),
      // so the grid ends as a whole and the host's revive relaunches from the
      // lowest index no workgroup started -- an index claimed by a workgroup
      // that left while others stayed resident would never start
      __hip_atomic_store(stopd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return kServiceExit;
    }
  }
}

__global__ __launch_bounds__(128, 1) void k_native_service(fksk::ServiceArgs) {
  __shared__ uint32_t claim[2];   // index, data slot
  __shared__ uint64_t t_start;    // s_memtime when the program was claimed
  for (;;) {
    uint64_t kp = (uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));   // re-derived per program, not held across the replay
    if (threadIdx.x == 0) {
      uint32_t slot = 0;
      claim[0] = service_claim(kp, &slot);
      claim[1] = slot;
      t_start = __builtin_amdgcn_s_memtime();
    }
    __syncthreads();
    const uint32_t idx = claim[0];
    if (idx == kServiceExit) return;   // (uniform across the workgroup)
    service_replay(kp, (int)claim[1]);
    if (threadIdx.x >= kWave) {
      const FKS_CONST ServiceCtl& c = service_args((uint64_t)(uintptr_t)__builtin_amdgcn_kernarg_segment_ptr())->c;
      if (threadIdx.x == kWave) {
        // the replay's device cost (the search's parent sampling and bloat
        // control read it; never the score), covered by the release below
        const uint64_t dt = __builtin_amdgcn_s_memtime() - t_start;
        __hip_atomic_store(&c.cost[claim[1]], dt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      // the scoring wave wrote the result row: make it visible to the host, then flag it
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      if (threadIdx.x == kWave)
        __hip_atomic_store(&c.done[claim[1]], claim[0] + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads();   // both waves are done with the LDS (and with `claim`) before the next program
  }
}
// glibc-exact exp / log / pow (glibc_math.h) on device, one argument per lane:
// the device side of tests/test_gpu_glibc_math.py
__global__ __launch_bounds__(256) void k_gm_batch(int fn, const double* x, const double* y, double* out, int32_t* st,
                                                  int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double o = 0.0;
  int s = 0;
  if (fn == 0) s = gm::exp(x[i], o);
  else if (fn == 1) s = gm::log(x[i], o);
  else s = gm::pow(x[i], y[i], o);
  out[i] = o;
  st[i] = s;
}
// A trace suite's program batch in one grid (launch.h SuiteArgs): block b
// replays program b % P on trace order[b / P], two waves as k_replay_native_duo.
// The workload is an entry of an HBM table, so kernarg_workload() has no
// place here: the entry's address is made wave-uniform and read through the
// constant address space (scalar loads, as the service's replay reads its
// kernel arguments), for the hot scalars and the cold fields alike.
__global__ __launch_bounds__(128, 1) void k_replay_native_duo_suite(fksk::SuiteArgs s, RowNativeArgs nat) {
  const int g = (int)blockIdx.x / s.P;
  const int p = (int)blockIdx.x - g * s.P;
  const int t = uni(s.order[g]);
  const fksd::DevWorkload* Wt = (const fksd::DevWorkload*)uniu64((uint64_t)(uintptr_t)(s.tab + t));
  const FKS_CONST fksd::DevWorkload* Wc = const_ptr(Wt);
  const fksd::DevWorkload& W = *(const fksd::DevWorkload*)Wc;
  const uint64_t hoff = uniu64(const_ptr(s.heap_off)[t]);
  replay_duo<false>(W, Wt, s.gheap + hoff, s.out + (size_t)t * s.P, nat, s.table + (size_t)t * s.P * 13, nullptr, p, p);
}
#endif

template <int NPASS, bool GHEAP>
__global__ __launch_bounds__(64, GHEAP ? 2 : 1) void k_replay_native(fksk::NativeArgs a) {
  const int p = blockIdx.x;
  const Slot s = policy_slot<GHEAP>(a.W, a.gheap, p);
  NativeScorerDev sc;
  sc.fn = prog_of(uniu64(a.fn[p]));
  sc.feas = prog_feas(uniu64(a.fn[p]));
  sc.gmem = a.W.gmem_total;
  // the constant block moves into the slot's register area (the host reserves
  // kKcLds / 64 VM registers for it; the allocation is padded by kKcLds entries,
  // so the fixed-size copy never reads past it)
  const FKS_GLOBAL int64_t* ksrc = global_ptr(a.kc + a.koff[p]);
  FKS_LDS int64_t* kl = reinterpret_cast<FKS_LDS int64_t*>(lds_ptr(s.vregs));
  for (int i = lane_id(); i < kKcLds; i += kWave) kl[i] = ksrc[i];
  sc.kc = kl;
  replay_one<NPASS>(a.W, kernarg_workload(), sc, s.h, s.top, s.T, s.delmap, s.inv, a.out + p);
}
// Schedule mode: the HBM-heap instance that also stores every commit's record (rec: [P, n_pods])
template <int NPASS>
__global__ __launch_bounds__(64, 2) void k_replay_native_sched(fksk::NativeArgs a, SchedRec* rec) {
  const int p = blockIdx.x;
  const Slot s = policy_slot<true>(a.W, a.gheap, p);
  NativeScorerDev sc;
  sc.fn = prog_of(uniu64(a.fn[p]));
  sc.feas = prog_feas(uniu64(a.fn[p]));
  sc.gmem = a.W.gmem_total;
  const FKS_GLOBAL int64_t* ksrc = global_ptr(a.kc + a.koff[p]);   // as k_replay_native
  FKS_LDS int64_t* kl = reinterpret_cast<FKS_LDS int64_t*>(lds_ptr(s.vregs));
  for (int i = lane_id(); i < kKcLds; i += kWave) kl[i] = ksrc[i];
  sc.kc = kl;
  replay_one<NPASS, NativeScorerDev, NoProf, false, SchedSink>(a.W, kernarg_workload(), sc, s.h, s.top, s.T, s.delmap,
                                                                   s.inv, a.out + p, nullptr,
                                                                   SchedSink{rec + (size_t)p * a.W.n_pods});
}
constexpr std::array<Row<fksk::NativeArgs, SchedRec*>, 1> kNativeSched = {
    {{0, k_replay_native_sched<FKS_NPASS>}}};
// Time-metrics mode: the HBM-heap instance that also carries the program's TimeAcc and writes trec[p]
template <int NPASS>
__global__ __launch_bounds__(64, 2) void k_replay_native_time(fksk::NativeArgs a, TimeRec* trec) {
  const int p = blockIdx.x;
  const Slot s = policy_slot<true>(a.W, a.gheap, p);
  NativeScorerDev sc;
  sc.fn = prog_of(uniu64(a.fn[p]));
  sc.feas = prog_feas(uniu64(a.fn[p]));
  sc.gmem = a.W.gmem_total;
  const FKS_GLOBAL int64_t* ksrc = global_ptr(a.kc + a.koff[p]);   // as k_replay_native
  FKS_LDS int64_t* kl = reinterpret_cast<FKS_LDS int64_t*>(lds_ptr(s.vregs));
  for (int i = lane_id(); i < kKcLds; i += kWave) kl[i] = ksrc[i];
  sc.kc = kl;
  replay_one<NPASS, NativeScorerDev, NoProf, false, NoSched, TimeSink>(a.W, kernarg_workload(), sc, s.h, s.top, s.T,
                                                                      s.delmap, s.inv, a.out + p, nullptr, NoSched{},
                                                                      TimeSink{trec + p});
}
constexpr std::array<Row<fksk::NativeArgs, TimeRec*>, 1> kNativeTime = {
    {{0, k_replay_native_time<FKS_NPASS>}}};
template <int... G>
constexpr std::array<Row<fksk::NativeArgs>, sizeof...(G)> native_rows(Keys<G...>) {
  return {{{G, k_replay_native<FKS_NPASS, G != 0>}...}};
}
constexpr auto kNative = native_rows(Heaps{});
#if FKS_NPASS == 1
// key: the profiled flag
constexpr std::array<Row<fksk::BuiltinArgs, RowNativeArgs, int, uint32_t*, uint32_t, int>, 2> kRowsNative = {
    {{0, k_replay_rows_native}, {1, k_replay_rows_native_prof}}};
constexpr std::array<Row<fksk::BuiltinArgs, RowNativeArgs>, 2> kNativeDuo = {
    {{0, k_replay_native_duo}, {1, k_replay_native_duo_prof}}};
constexpr std::array<Row<fksk::BuiltinArgs, RowNativeArgs, SchedRec*>, 1> kNativeDuoSched = {
    {{0, k_replay_native_duo_sched}}};
constexpr std::array<Row<fksk::BuiltinArgs, RowNativeArgs, TimeRec*>, 1> kNativeDuoTime = {
    {{0, k_replay_native_duo_time}}};
constexpr std::array<Row<fksk::ServiceArgs>, 1> kService = {{{0, k_native_service}}};
constexpr std::array<Row<fksk::SuiteArgs, RowNativeArgs>, 1> kNativeDuoSuite = {{{0, k_replay_native_duo_suite}}};
#endif
#endif

}  // namespace

namespace fksk {

// Every unit defines unit_attrs for its (kind, NPASS): the LDS limit of all its
// tables.  The wave-kernel units also define the launchers of their NPASS.
template <int KIND, int NPASS> hipError_t unit_attrs(int max_lds);
template <int NPASS> hipError_t unit_launch_builtin(bool gheap, int fam, int P, size_t lds, hipStream_t s, const BuiltinArgs& a);
template <int NPASS> hipError_t unit_launch_vm(bool gheap, int P, size_t lds, hipStream_t s, const VmArgs& a);
template <int NPASS> hipError_t unit_launch_native(bool gheap, int P, size_t lds, hipStream_t s, const NativeArgs& a);
template <int NPASS> hipError_t unit_launch_builtin_sched(int P, size_t lds, hipStream_t s, const BuiltinArgs& a, SchedRec* rec);
template <int NPASS> hipError_t unit_launch_native_sched(int P, size_t lds, hipStream_t s, const NativeArgs& a, SchedRec* rec);
template <int NPASS> hipError_t unit_launch_builtin_time(int P, size_t lds, hipStream_t s, const BuiltinArgs& a, TimeRec* trec);
template <int NPASS> hipError_t unit_launch_native_time(int P, size_t lds, hipStream_t s, const NativeArgs& a, TimeRec* trec);

#if FKS_KIND == 0
template <>
hipError_t unit_launch_builtin<FKS_NPASS>(bool gheap, int fam, int P, size_t lds, hipStream_t s, const BuiltinArgs& a) {
  return launch_row(gheap ? kBuiltinHbm : kBuiltinLds, fam, dim3(P), dim3(64), lds, s, a);
}
#if FKS_NPASS == 4
hipError_t launch_builtin_wave_duo(int fam, int P, size_t lds, hipStream_t s, const BuiltinArgs& a) {
  return launch_row(kBuiltinDuo, fam, dim3(P), dim3(128), lds, s, a);
}
#endif
template <>
hipError_t unit_launch_builtin_sched<FKS_NPASS>(int P, size_t lds, hipStream_t s, const BuiltinArgs& a, SchedRec* rec) {
  return launch_row(kBuiltinSched, 0, dim3(P), dim3(64), lds, s, a, rec);
}
template <>
hipError_t unit_launch_builtin_time<FKS_NPASS>(int P, size_t lds, hipStream_t s, const BuiltinArgs& a, TimeRec* trec) {
  return launch_row(kBuiltinTime, 0, dim3(P), dim3(64), lds, s, a, trec);
}
template <>
hipError_t unit_attrs<0, FKS_NPASS>(int mx) {
  hipError_t e = raise_lds(mx, kBuiltinHbm, kBuiltinLds, kBuiltinSched, kBuiltinTime);
#if FKS_NPASS == 4
  if (e == hipSuccess) e = raise_lds(mx, kBuiltinDuo);
#endif
  return e;
}
#endif

#if FKS_KIND == 1
template <>
hipError_t unit_launch_vm<FKS_NPASS>(bool gheap, int P, size_t lds, hipStream_t s, const VmArgs& a) {
  return launch_row(kVm, gheap, dim3(P), dim3(64), lds, s, a);
}
template <>
hipError_t unit_attrs<1, FKS_NPASS>(int mx) { return raise_lds(mx, kVm); }
#endif

#if FKS_KIND == 2
hipError_t launch_builtin_prof(bool gheap, int P, size_t lds, hipStream_t s, const BuiltinArgs& a) {
  return launch_row(kBuiltinProf, gheap, dim3(P), dim3(64), lds, s, a);
}
hipError_t launch_c5_prof(int P, size_t lds, hipStream_t s, const BuiltinArgs& a) {
  return launch_row(kC5Prof, 0, dim3(P), dim3(64), lds, s, a);
}
hipError_t launch_vm_prof(bool gheap, int P, size_t lds, hipStream_t s, const VmArgs& a) {
  return launch_row(kVmProf, gheap, dim3(P), dim3(64), lds, s, a);
}
template <>
hipError_t unit_attrs<2, 1>(int mx) { return raise_lds(mx, kBuiltinProf, kVmProf, kC5Prof); }
#endif


#if FKS_KIND == 3
hipError_t launch_builtin_rows(int fam, int P, int waves, uint32_t* queue, uint32_t qbase, size_t lds, hipStream_t st,
                              const BuiltinArgs& a) {
  return launch_row(kRows, fam, dim3(waves), dim3(64), lds, st, a, P, queue, qbase);
}
int rows_waves_per_cu(int fam, size_t lds) { return blocks_per_cu(kRows, fam, 64, lds); }
hipError_t launch_builtin_rows_prof(int fam, int P, int waves, uint32_t* queue, uint32_t qbase, size_t lds, hipStream_t st,
                                   const BuiltinArgs& a) {
  // the three composite codes share the one profiled composite build
  const int key = fam == kRowCompositeW5 || fam == kRowCompositeSplit ? FAM_COMPOSITE_LINEAR : fam;
  return launch_row(kRowsProf, key, dim3(waves), dim3(64), lds, st, a, P, queue, qbase);
}
hipError_t launch_builtin_rows_sched(int P, int waves, uint32_t* queue, uint32_t qbase, size_t lds, hipStream_t st,
                                     const BuiltinArgs& a, SchedRec* rec) {
  return launch_row(kRowsSched, 0, dim3(waves), dim3(64), lds, st, a, P, queue, qbase, rec);
}
int rows_sched_waves_per_cu(size_t lds) { return blocks_per_cu(kRowsSched, 0, 64, lds); }
hipError_t launch_builtin_rows_time(int fam, int P, int waves, uint32_t* queue, uint32_t qbase, size_t lds, hipStream_t st,
                                    const BuiltinArgs& a, TimeRec* trec) {
  return launch_row(kRowsTime, fam, dim3(waves), dim3(64), lds, st, a, P, queue, qbase, trec);
}
int rows_time_waves_per_cu(int fam, size_t lds) { return blocks_per_cu(kRowsTime, fam, 64, lds); }
template <>
hipError_t unit_attrs<3, 1>(int mx) { return raise_lds(mx, kRowsProf, kRows, kRowsSched, kRowsTime); }
#endif


#if FKS_KIND == 4
template <>
hipError_t unit_launch_native<FKS_NPASS>(bool gheap, int P, size_t lds, hipStream_t s, const NativeArgs& a) {
  return launch_row(kNative, gheap, dim3(P), dim3(64), lds, s, a);
}
template <>
hipError_t unit_launch_native_sched<FKS_NPASS>(int P, size_t lds, hipStream_t s, const NativeArgs& a, SchedRec* rec) {
  return launch_row(kNativeSched, 0, dim3(P), dim3(64), lds, s, a, rec);
}
template <>
hipError_t unit_launch_native_time<FKS_NPASS>(int P, size_t lds, hipStream_t s, const NativeArgs& a, TimeRec* trec) {
  return launch_row(kNativeTime, 0, dim3(P), dim3(64), lds, s, a, trec);
}
#if FKS_NPASS == 1
hipError_t launch_native_duo_time(int P, size_t lds, hipStream_t st, const BuiltinArgs& a, const fksd::RowNativeArgs& nat,
                                  TimeRec* trec) {
  return launch_row(kNativeDuoTime, 0, dim3(P), dim3(128), lds, st, a, nat, trec);
}
int native_duo_time_blocks_per_cu(size_t lds) { return blocks_per_cu(kNativeDuoTime, 0, 128, lds); }
hipError_t launch_native_duo_sched(int P, size_t lds, hipStream_t st, const BuiltinArgs& a, const fksd::RowNativeArgs& nat,
                                   SchedRec* rec) {
  return launch_row(kNativeDuoSched, 0, dim3(P), dim3(128), lds, st, a, nat, rec);
}
int native_duo_sched_blocks_per_cu(size_t lds) { return blocks_per_cu(kNativeDuoSched, 0, 128, lds); }
hipError_t launch_native_rows(int P, int waves, int rows_active, uint32_t* queue, uint32_t qbase, size_t lds,
                              hipStream_t st, const BuiltinArgs& a, const fksd::RowNativeArgs& nat) {
  return launch_row(kRowsNative, a.prof != nullptr, dim3(waves), dim3(64), lds, st, a, nat, P, queue, qbase, rows_active);
}
hipError_t launch_native_duo(int P, size_t lds, hipStream_t st, const BuiltinArgs& a, const fksd::RowNativeArgs& nat) {
  return launch_row(kNativeDuo, a.prof != nullptr, dim3(P), dim3(128), lds, st, a, nat);
}
hipError_t launch_native_service(int blocks, size_t lds, hipStream_t st, const ServiceArgs& s) {
  return launch_row(kService, 0, dim3(blocks), dim3(128), lds, st, s);
}
int native_service_blocks_per_cu(size_t lds) { return blocks_per_cu(kService, 0, 128, lds); }
int native_duo_blocks_per_cu(size_t lds) { return blocks_per_cu(kNativeDuo, 0, 128, lds); }
hipError_t launch_native_duo_suite(int blocks, size_t lds, hipStream_t st, const SuiteArgs& s,
                                   const fksd::RowNativeArgs& nat) {
  return launch_row(kNativeDuoSuite, 0, dim3(blocks), dim3(128), lds, st, s, nat);
}
int native_duo_suite_blocks_per_cu(size_t lds) { return blocks_per_cu(kNativeDuoSuite, 0, 128, lds); }
int native_rows_waves_per_cu(size_t lds) { return blocks_per_cu(kRowsNative, 0, 64, lds); }
hipError_t native_rt_table(uint64_t* dev_out, hipStream_t s) {
  hipLaunchKernelGGL(k_native_rt_table, dim3(1), dim3(64), 0, s, dev_out);
  return hipGetLastError();
}
hipError_t launch_gm_batch(int fn, const double* x, const double* y, double* out, int32_t* st, int64_t n) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gm_batch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn, x, y, out, st, n);
  return hipGetLastError();
}
#endif
template <>
hipError_t unit_attrs<4, FKS_NPASS>(int mx) {
  hipError_t e = raise_lds(mx, kNative, kNativeSched, kNativeTime);
#if FKS_NPASS == 1
  if (e == hipSuccess) e = raise_lds(mx, kRowsNative, kNativeDuo, kNativeDuoSched, kNativeDuoTime, kNativeDuoSuite);
  // (the service kernel's static LDS -- the claim word -- counts against the 160 KiB too)
  if (e == hipSuccess) e = raise_lds(mx - 64, kService);
#endif
  return e;
}
#endif

#if FKS_KIND == 0 && FKS_NPASS == 1
// ---- NPASS -> translation unit ------------------------------------------------------------
// The one place that maps an NPASS value to the unit compiled for it (this
// unit carries it for all of them), and the list of all units, which follows
// HIP_UNITS of ops/build.py.
template <class F>
hipError_t for_npass(int npass, F f) {
  switch (npass) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return hipErrorInvalidValue;
  }
}
hipError_t launch_builtin(int npass, bool gheap, int fam, int P, size_t lds, hipStream_t s, const BuiltinArgs& a) {
  return for_npass(npass, [&](auto n) { return unit_launch_builtin<decltype(n)::value>(gheap, fam, P, lds, s, a); });
}
hipError_t launch_vm(int npass, bool gheap, int P, size_t lds, hipStream_t s, const VmArgs& a) {
  return for_npass(npass, [&](auto n) { return unit_launch_vm<decltype(n)::value>(gheap, P, lds, s, a); });
}
hipError_t launch_native(int npass, bool gheap, int P, size_t lds, hipStream_t s, const NativeArgs& a) {
  return for_npass(npass, [&](auto n) { return unit_launch_native<decltype(n)::value>(gheap, P, lds, s, a); });
}
hipError_t launch_builtin_sched(int npass, int P, size_t lds, hipStream_t s, const BuiltinArgs& a, SchedRec* rec) {
  return for_npass(npass, [&](auto n) { return unit_launch_builtin_sched<decltype(n)::value>(P, lds, s, a, rec); });
}
hipError_t launch_native_sched(int npass, int P, size_t lds, hipStream_t s, const NativeArgs& a, SchedRec* rec) {
  return for_npass(npass, [&](auto n) { return unit_launch_native_sched<decltype(n)::value>(P, lds, s, a, rec); });
}
hipError_t launch_builtin_time(int npass, int P, size_t lds, hipStream_t s, const BuiltinArgs& a, TimeRec* trec) {
  return for_npass(npass, [&](auto n) { return unit_launch_builtin_time<decltype(n)::value>(P, lds, s, a, trec); });
}
hipError_t launch_native_time(int npass, int P, size_t lds, hipStream_t s, const NativeArgs& a, TimeRec* trec) {
  return for_npass(npass, [&](auto n) { return unit_launch_native_time<decltype(n)::value>(P, lds, s, a, trec); });
}
hipError_t set_all_attrs(int max_lds) {
  for (auto unit : {unit_attrs<0, 1>, unit_attrs<0, 2>, unit_attrs<0, 4>, unit_attrs<1, 1>, unit_attrs<1, 2>,
                    unit_attrs<1, 4>, unit_attrs<2, 1>, unit_attrs<3, 1>, unit_attrs<4, 1>, unit_attrs<4, 2>,
                    unit_attrs<4, 4>}) {
    const hipError_t e = unit(max_lds);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
#endif

}  // namespace fksk
