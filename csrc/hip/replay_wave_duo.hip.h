// k_replay_builtin_duo: the 256-node (NPASS 4) builtin-family replay split
// over TWO waves of one workgroup -- replay_one's event loop with its heap and
// its nodes on different waves.
//
// On 256-node clusters one event of the one-wave kernel runs the CPython
// heappop (5.4k cycles: four 5-level subtree gathers, the last from HBM) and
// the scoring of the four node slots per lane (5.3k) back to back
// (profiles/r3_config5_wave_phase_split.json), although the sift of the
// heap's last entry and the scoring of the popped pod are independent.  Here,
// with the handshake of replay_duo.hip.h (DuoBox: LDS ring of popped keys,
// S -> H verdicts),
//   * wave H owns the heap (WaveHeapT: LDS top + HBM slice, deletion bitmap):
//     it pops, publishes the key, sifts; deletions need nothing back, so H runs
//     ahead through them; for a creation it waits for S's verdict and pushes
//     the placement's deletion entry or -- computing the repush time itself
//     (repush_anchor) -- the re-queued pod;
//   * wave S owns the node side (WaveNodes<4>: node registers, waiting-class
//     histogram, utilisation totals, exact accumulators) and runs the scorer,
//     the argmax, the GPU pick and the snapshot schedule.
// This file holds what is the two-wave kernel's own: the H-wave loop, the
// S wave's sequencing of the event steps, and where in it S answers H (before
// the commit, and before the fragmentation sum of a failure, so H's push or
// scan runs meanwhile).  The steps are those of replay.hip.h (WaveNodes,
// decode_pod, repush_anchor).  replay_one calls the same decode, deletion,
// repush-time, snapshot and write-back code; scoring, failed placement and GPU
// pick / commit it spells out in copies of its own, so for those, equal event
// order and arithmetic (bit-identical results) rest on the tests:
// tests/test_gpu_engine.py compares the two kernels row for row,
// tests/test_gpu_shapes.py both with the CPU oracle.
// Not covered: the invariant check (it reads heap and nodes together; the
// host keeps replay_one for check_invariants runs).
#pragma once

#include "replay.hip.h"
#include "replay_duo.hip.h"

namespace fksd {

__host__ __device__ inline size_t wave_duo_box_bytes() { return (sizeof(DuoBox) + 15) & ~size_t(15); }

template <int NPASS, class Scorer, bool FLAT>
__device__ void replay_wave_duo(const DevWorkload& W, const DevWorkload* Wcold, Scorer& scorer,
                                FKS_GLOBAL uint64_t* hbuf, FKS_LDS uint64_t* htop, int T, FKS_LDS uint32_t* delmap,
                                FKS_LDS DuoBox* box, DevResult* out) {
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);   // 0: H (heap), 1: S (nodes, scorer, evaluator)
  const int lb = W.low_bits, nb = W.node_bits, rb = W.rank_bits;
  const int tshift = rb + lb;
  const uint64_t time_max = (W.time_bits >= 63) ? ~0ull : ((1ull << W.time_bits) - 1);
  const int N = W.n_pods;

  if (wave == 0) {
    // ================= H: the heap
    // (replay_duo's H loop with WaveHeapT, both repush rules and no profiling)
    WaveHeapT<FLAT> heap;
    heap.h = hbuf;
    heap.top = htop;
    heap.bind();
    heap.T = T;
    heap.delmap = delmap;
    heap.M = W.delmap_slots;
    heap.lb = lb;
    heap.lane = lane;
    for (int i = lane; i < N; i += kWave) heap.st(i, W.heap0[i]);
    for (int i = lane; i < (W.delmap_slots >> 5); i += kWave) heap.delmap[i] = 0u;
    if (lane == 0) duo_reset(box);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    const bool earliest = cold_ptr(Wcold)->repush_earliest != 0;
    int n = N, n_repush = 0, n_dropped = 0;
    int32_t hexc = EXC_NONE;
    uint32_t k = 0, tail_seen = 0;
    bool published = false;   // event k already published (the previous push's forecast)
    uint64_t top = 0;
    while (n > 0) {
      {   // lane-derived predicates recomputed per event (replay_one)
        int ol = lane;
        asm volatile("" : "+v"(ol));
        heap.lane = ol;
      }
      if (!published) {
        top = uniu64(heap.ld_u(0));
        if (!duo_publish(box, lane == 0, k, tail_seen, top, hexc)) break;
      }
      published = false;
      const uint64_t last = uniu64(heap.ld_u(n - 1));
      --n;
      if (n > 0) heap.pop_reinsert(n, last);
      if ((int)(top & 3) != kDelete) {
        if (!duo_verdict(box, k, hexc)) break;
        const int code = box->code;
        if (code == DUO_ABORT) break;   // S holds the exception
        uint64_t item = box->item;
        if (code == DUO_FAIL) {
          item = 0;
          const int64_t anchor = repush_anchor(heap, n, earliest, tshift, lane);
          if (anchor >= 0) {
            const uint64_t nt = (uint64_t)(anchor + 1);
            if (nt > time_max) { hexc = EXC_UNSUPPORTED; break; }
            item = (nt << tshift) | ((uint64_t)key_rank(top, lb, rb) << lb) | kRetry;
            ++n_repush;
          } else {
            ++n_dropped;
          }
        }
        if (item != 0) {
          // the next pop returns min(root, item) ((time, rank) keys are
          // unique): publish it before the push, S starts on it meanwhile
          const uint64_t root = n > 0 ? uniu64(heap.ld_u(0)) : ~0ull;
          const uint64_t next = item < root ? item : root;
          ++k;
          if (!duo_publish(box, lane == 0, k, tail_seen, next, hexc)) break;
          published = true;
          top = next;
          heap.push(n, item);
          ++n;
          continue;
        }
      }
      ++k;
    }
    if (lane == 0) duo_term(box, hexc, n_repush, n_dropped);
    return;
  }

  // ================= S: nodes, scorer, evaluator
  NodeRegs<NPASS> nr;
  int32_t wcnt[kWaitSlots];
  WaveNodes<NPASS> ns{lane, nr, wcnt};
  ns.init(W);
  __syncthreads();
  auto reply = [&](int code, uint64_t item, uint32_t kk) { duo_reply(box, lane == 0, code, item, kk); };
  uint32_t k = 0;
  for (;;) {
    const FKS_CONST DevWorkload* Wc = cold_ptr(Wcold);
    {
      const int4* c = reinterpret_cast<const int4*>(uniu64(reinterpret_cast<uint64_t>(nr.cst)));
      asm volatile("" : "+s"(c));
      nr.cst = c;
    }
    if (!duo_next(box, k, ns.exc)) break;
    const uint64_t top = duo_take(box, lane == 0, k);
    const int rank = key_rank(top, lb, rb);
    const int4 precv = load_vgpr(&W.pod[rank]);
    const int kind = (int)(top & 3);
    const PodView pod = decode_pod(W, top, rank, precv, tshift);
    const int64_t t = pod.ctime;

    if (kind == kDelete) {
      ns.remove(W, top, pod);
    } else {
      int best_node;
      if (!ns.place(W, scorer, pod, best_node)) { reply(DUO_ABORT, 0, k); break; }
      if (best_node < 0) {
        // failed placement: S keeps the metrics, H computes the repush
        reply(DUO_FAIL, 0, k);
        ns.fail(Wc, kind, pod);
        if (W.trace_hash) ns.hsh = mix_event(ns.hsh, ((uint64_t)(uint32_t)rank << 2) | 2, (uint64_t)t);
      } else {
        int gmask;
        if (!ns.pick(Wc, pod, best_node, gmask)) { reply(DUO_ABORT, 0, k); break; }
        const uint64_t dt = (uint64_t)(t + pod.dur);
        if (t + pod.dur < 0 || dt > time_max) { ns.exc = EXC_UNSUPPORTED; reply(DUO_ABORT, 0, k); break; }
        // answer first: H's push runs while S commits
        reply(DUO_PLACED, (dt << tshift) | ((uint64_t)rank << lb) | ((uint64_t)gmask << (2 + nb)) |
                              ((uint64_t)best_node << 2) | kDelete, k);
        ns.commit(kind, pod, best_node, gmask);
        if (W.trace_hash) ns.hsh = mix_event(ns.hsh, ((uint64_t)(uint32_t)rank << 2), ((uint64_t)t << 8) ^ (uint64_t)best_node);
      }
    }
    ns.snapshot(Wc, N);
    ++k;
  }
  int n_repush, n_dropped;
  if (duo_join(box, ns.exc, n_repush, n_dropped)) --ns.processed;
  ns.write(out, n_repush, n_dropped);
}

}  // namespace fksd
