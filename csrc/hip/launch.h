// Host-side launch API of the replay kernels.
//
// The kernels are compiled in separate translation units (one per kind and
// NPASS, see replay_kernels.hip and ops/build.py) so the many template
// instances build in parallel; module.hip only sees these launchers.
//
// Behind this header every group of kernel instances is one table of
// {key, kernel} rows in replay_kernels.hip; the key is the family code, the
// heap flag or the profiled flag.  Launches, the dynamic-LDS limit and the
// occupancy queries all go through a table (launch_row / raise_lds /
// blocks_per_cu there), and set_all_attrs() walks every table of every unit.
// To add an instance: define the kernel and add its row to the table of its
// group -- nothing else.  The waves per SIMD that an instance is compiled for
// are defined below, for its __launch_bounds__ and for the host's LDS sizing.
#pragma once

#include <hip/hip_runtime.h>

#include "replay.hip.h"
#include "vm_dev.hip.h"
#include "replay_rows.hip.h"
#include "replay_wave_duo.hip.h"

// Waves per SIMD of the kernel instances (__launch_bounds__ in replay_kernels.hip)
// and of the host's LDS share per policy (engine_host.hip.h heap_top_for).
// Build-time knobs for A/B runs; the assertions pin the defaults to the shares
// the host was tuned with (16, 12, 8 policies per CU: 4 SIMDs x waves per SIMD).
// NPASS 1, HBM heap: the feature families carry ~40 more live values through
// scoring: 3 waves/SIMD without spills beats 4 with scratch traffic
#ifndef FKS_LIGHT_WAVES
#define FKS_LIGHT_WAVES 4   // first-fit / best-fit / random_linear
static_assert(4 * FKS_LIGHT_WAVES == 16, "the NPASS-1 LDS share is 16 policies per CU");
#endif
#ifndef FKS_HEAVY_WAVES
#define FKS_HEAVY_WAVES 3   // feature / composite families and mixed batches
#endif
// 128 nodes (NPASS 2): 2 node slots per lane
#ifndef FKS_NP2_WAVES
#define FKS_NP2_WAVES 3
static_assert(4 * FKS_NP2_WAVES == 12, "the NPASS-2 LDS share is 12 policies per CU");
#endif
// 256 nodes (NPASS 4): 4 node slots per lane
#ifndef FKS_NP4_WAVES
#define FKS_NP4_WAVES 4     // packed GPU milli + node constants on demand: <= 128 VGPRs
#endif
// the two-wave (heap wave + scoring wave) NPASS-4 kernel: 5 (96 VGPRs, a few
// spills) measured above 4 (124 VGPRs), profiles/r5_config5_wave_duo_ab.txt
#ifndef FKS_NP4_DUO_WAVES
#define FKS_NP4_DUO_WAVES 5
#endif
// The VM keeps its hot virtual registers in VGPRs (vm_dev.hip.h)
#ifndef FKS_VM_WAVES
#define FKS_VM_WAVES 2
static_assert(4 * FKS_VM_WAVES == 8, "the VM LDS share is 8 policies per CU");
#endif
// Row kernels: the LDS share per wave (4 heap tops + bitmaps) is what bounds
// residency; registers are capped so LDS, not VGPRs, stays the limit.
#ifndef FKS_ROW_WAVES
#define FKS_ROW_WAVES 5        // first-fit / best-fit / random_linear
#endif
#ifndef FKS_ROW_HEAVY_WAVES
#define FKS_ROW_HEAVY_WAVES 4  // feature / composite families (composite: only loop-invariant snapshot
                               // divisors spill, reloaded on the rare snapshot path)
#endif

namespace fksk {

using fksd::DevProgramTable;
using fksd::DevResult;
using fksd::DevWorkload;

struct BuiltinArgs {
  DevWorkload W;
  const DevWorkload* Wc = nullptr;   // unused (once an HBM copy of W; the kernels read W from their kernarg segment).
                                     // Kept: without it the arguments behind it move by 8 bytes, and the scratch
                                     // frame of k_replay_vm<4, *> changed with them (800 -> 784 bytes)
  const int32_t* fam;     // [P] family id per policy
  const double* weights;  // [P, kWeights] (pinned host memory, device-mapped)
  double* wdev;           // [P, kWeights] device copy written by the kernel prologue
  DevResult* out;
  uint64_t* gheap;        // HBM heap slices (GHEAP) or nullptr
  uint64_t* prof;         // [P, 8] phase cycles (profiling launches only)
  double* table = nullptr;  // row kernels: [P, 13] result table written by the kernel (k_eval_reduce fused)
};

struct VmArgs {
  DevWorkload W;
  const DevWorkload* Wc = nullptr;   // unused, see BuiltinArgs
  DevProgramTable T;
  DevResult* out;
  int64_t budget;
  int32_t nregs;          // max virtual registers over the batch's programs
  uint64_t* gheap;
  uint64_t* prof;
};

// Native programs (FKS_KIND 4): fn[p] = device address of policy p's
// JIT-compiled scorer (jit_abi.h ProgFn), kc + koff[p] its constant block.
struct NativeArgs {
  DevWorkload W;
  const DevWorkload* Wc = nullptr;   // unused, see BuiltinArgs
  const uint64_t* fn;     // [P] function pointers (pinned host memory, device-mapped)
  const int64_t* kc;      // concatenated constant blocks
  const int32_t* koff;    // [P] offsets into kc
  DevResult* out;
  uint64_t* gheap;
};

// Raise the dynamic-LDS limit of every kernel instance of every unit.
hipError_t set_all_attrs(int max_lds);

// The wave kernels exist once per NPASS (1, 2, 4: node slots per lane).
// fam_spec >= 0: every policy of the batch has that family (specialised
// kernel); anything else: the mixed-batch instance.
hipError_t launch_builtin(int npass, bool gheap, int fam_spec, int P, size_t lds, hipStream_t s, const BuiltinArgs& a);
hipError_t launch_vm(int npass, bool gheap, int P, size_t lds, hipStream_t s, const VmArgs& a);
hipError_t launch_native(int npass, bool gheap, int P, size_t lds, hipStream_t s, const NativeArgs& a);
// NPASS 4, HBM heap: one policy per 128-thread workgroup of a heap wave and a
// scoring wave (replay_wave_duo.hip.h); lds includes fksd::wave_duo_box_bytes()
hipError_t launch_builtin_wave_duo(int fam_spec, int P, size_t lds, hipStream_t s, const BuiltinArgs& a);

// row kernels: 4 policies per wave (clusters of <= 16 nodes, replay_rows.hip.h)
// `waves` persistent waves drain the P-policy queue: claims are
// atomicAdd(queue) - qbase (the counter runs on across launches; a launch
// makes exactly P + 4 * waves claims).
hipError_t launch_builtin_rows(int fam_spec, int P, int waves, uint32_t* queue, uint32_t qbase, size_t lds, hipStream_t s,
                              const BuiltinArgs& a);
// s_memtime phase-profiled variant (random_linear / composite_linear / mixed); a.prof: [waves, 8]
hipError_t launch_builtin_rows_prof(int fam_spec, int P, int waves, uint32_t* queue, uint32_t qbase, size_t lds, hipStream_t s,
                                   const BuiltinArgs& a);
// resident row-kernel waves per CU for a family's instance at `lds` bytes (-1: error)
int rows_waves_per_cu(int fam_spec, size_t lds);

// row kernel over natively compiled programs (fn / kc / koff as in NativeArgs);
// rows_active rows per wave claim programs, so a launch makes P + rows_active * waves claims;
// a.prof != nullptr: the s_memtime phase-profiled build ([waves, 8] cycles)
hipError_t launch_native_rows(int P, int waves, int rows_active, uint32_t* queue, uint32_t qbase, size_t lds,
                              hipStream_t s, const BuiltinArgs& a, const fksd::RowNativeArgs& nat);
// two-wave native replay (replay_duo.hip.h): one program per 128-thread workgroup;
// a.prof != nullptr: the s_memtime phase-profiled build ([P, 2, 8] cycles)
hipError_t launch_native_duo(int P, size_t lds, hipStream_t stream, const BuiltinArgs& a,
                             const fksd::RowNativeArgs& nat);
int native_rows_waves_per_cu(size_t lds);
int native_duo_blocks_per_cu(size_t lds);   // resident two-wave workgroups per CU
// A trace suite's program batch in one grid of T * P two-wave workgroups
// (replay_kernels.hip k_replay_native_duo_suite): block b replays program
// b % P on trace order[b / P].  The workloads come from an HBM table, not from
// the kernel arguments; fn / kc / koff of `nat` are indexed by the program
// alone, so one copy of the batch's launch data serves every trace.
struct SuiteArgs {
  const DevWorkload* tab;     // [T] one entry per trace (heap_top set per launch layout)
  const int32_t* order;       // [T] traces by descending pod count: the longest replays start first
  int T, P;
  const uint64_t* heap_off;   // [T] u64-word offset of trace t's heap area (P slices) inside gheap
  DevResult* out;             // [T, P]
  uint64_t* gheap;
  double* table;              // [T, P, 13]
};
hipError_t launch_native_duo_suite(int blocks, size_t lds, hipStream_t stream, const SuiteArgs& s,
                                   const fksd::RowNativeArgs& nat);
int native_duo_suite_blocks_per_cu(size_t lds);
// the resident program service (replay_kernels.hip k_native_service): its one
// kernel argument, read back through the kernarg segment pointer
struct ServiceArgs {
  BuiltinArgs a;
  fksd::RowNativeArgs nat;
  fksd::ServiceCtl c;
};
static_assert(offsetof(ServiceArgs, a) == 0, "BuiltinArgs (and its DevWorkload) must open the service arguments");
hipError_t launch_native_service(int blocks, size_t lds, hipStream_t stream, const ServiceArgs& s);
int native_service_blocks_per_cu(size_t lds);

// Schedule mode: separate instances that also store one fksd::SchedRec per
// placed pod into rec[p * n_pods + rank] (device_common.h; the host fills the
// buffer with 0xFF bytes first).  One row each in a table of its own: the
// mixed-family HBM-heap one-wave kernel per NPASS, the mixed-family row kernel,
// the HBM-heap one-wave native kernel per NPASS and the two-wave native kernel.
// rec is a trailing kernel parameter, so no argument of the other instances moves.
hipError_t launch_builtin_sched(int npass, int P, size_t lds, hipStream_t s, const BuiltinArgs& a, fksd::SchedRec* rec);
hipError_t launch_builtin_rows_sched(int P, int waves, uint32_t* queue, uint32_t qbase, size_t lds, hipStream_t s,
                                     const BuiltinArgs& a, fksd::SchedRec* rec);
int rows_sched_waves_per_cu(size_t lds);
hipError_t launch_native_sched(int npass, int P, size_t lds, hipStream_t s, const NativeArgs& a, fksd::SchedRec* rec);
hipError_t launch_native_duo_sched(int P, size_t lds, hipStream_t stream, const BuiltinArgs& a,
                                   const fksd::RowNativeArgs& nat, fksd::SchedRec* rec);
int native_duo_sched_blocks_per_cu(size_t lds);

// Time-metrics mode: separate instances that carry one fksd::TimeRec of
// lane-resident accumulators through the replay and write it to trec[p]
// (device_common.h).  Tables of their own: the composite and the mixed-family
// row kernel (fam: FAM_COMPOSITE_LINEAR or anything else), the mixed-family
// HBM-heap one-wave kernel per NPASS, the two-wave native kernel and the
// HBM-heap one-wave native kernel per NPASS.  trec is a trailing kernel parameter.
hipError_t launch_builtin_time(int npass, int P, size_t lds, hipStream_t s, const BuiltinArgs& a, fksd::TimeRec* trec);
hipError_t launch_builtin_rows_time(int fam, int P, int waves, uint32_t* queue, uint32_t qbase, size_t lds, hipStream_t s,
                                    const BuiltinArgs& a, fksd::TimeRec* trec);
int rows_time_waves_per_cu(int fam, size_t lds);
hipError_t launch_native_time(int npass, int P, size_t lds, hipStream_t s, const NativeArgs& a, fksd::TimeRec* trec);
hipError_t launch_native_duo_time(int P, size_t lds, hipStream_t stream, const BuiltinArgs& a,
                                  const fksd::RowNativeArgs& nat, fksd::TimeRec* trec);
int native_duo_time_blocks_per_cu(size_t lds);

// addresses of the native programs' runtime library (fks_rt_binop, fks_rt_unop, register floor)
hipError_t native_rt_table(uint64_t* dev_out, hipStream_t s);
// glibc_math.h on the device (tests): fn 0 exp, 1 log, 2 pow; n arguments, one per lane
hipError_t launch_gm_batch(int fn, const double* x, const double* y, double* out, int32_t* st, int64_t n);

// phase-profiled variants (NPASS = 1)
hipError_t launch_builtin_prof(bool gheap, int P, size_t lds, hipStream_t s, const BuiltinArgs& a);
hipError_t launch_vm_prof(bool gheap, int P, size_t lds, hipStream_t s, const VmArgs& a);
// composite family, 4 node slots per lane, HBM heap (config-5 shape)
hipError_t launch_c5_prof(int P, size_t lds, hipStream_t s, const BuiltinArgs& a);

}  // namespace fksk
