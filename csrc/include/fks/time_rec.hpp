// Time metrics of one replay (host twin of fksd::TimeRec, csrc/hip/device_common.h):
// sums and maxima over the pods the replay placed.  Every placed pod is later
// deleted (the event loop drains the heap), so busy[] is the time integral of
// the cluster's usage.  All integer; a replay that raises reports all zeros.
#pragma once

#include <cstdint>

namespace fks {

struct TimeRec {
  int64_t wait_sum = 0;    // sum of start - pod_ctime
  int64_t wait_max = 0;    // max of the same (0 if none placed)
  int64_t end_max = 0;     // max of start + dur (0 if none placed)
  int64_t busy[4] = {0, 0, 0, 0};   // sum of cpu*dur, mem*dur, ngpu*dur, ngpu*gmilli*dur
  int64_t n_placed = 0;
  uint32_t hist[32] = {};  // hist[b]: pods with bit_length(wait) == b, clamped at 31
};
static_assert(sizeof(TimeRec) == 192, "eight 64-bit slots and 32 buckets");

inline int wait_bucket(int64_t wait) {
  int b = 0;
  for (uint64_t v = (uint64_t)wait; v != 0; v >>= 1) ++b;
  return b < 31 ? b : 31;
}

// one placed pod: it starts at `start`, was created at `ctime`
inline void record_time_metrics(TimeRec& r, int64_t start, int64_t ctime, int64_t dur, int64_t cpu, int64_t mem,
                                int64_t ngpu, int64_t gmilli) {
  const int64_t wait = start - ctime, end = start + dur;
  r.wait_sum += wait;
  if (wait > r.wait_max) r.wait_max = wait;
  if (end > r.end_max) r.end_max = end;
  r.busy[0] += cpu * dur;
  r.busy[1] += mem * dur;
  r.busy[2] += ngpu * dur;
  r.busy[3] += ngpu * gmilli * dur;
  r.n_placed += 1;
  r.hist[wait_bucket(wait)] += 1;
}

}  // namespace fks
