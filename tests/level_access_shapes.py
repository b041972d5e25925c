"""Workloads for the row kernel's heap accesses by level.

A pop of the row kernel (csrc/hip/replay_rows.hip.h, `RowHeapT::pop_reinsert`)
walks the heap four levels per round, and each round reads and writes a fixed
range of slots: round 0 children 1-30, round 1 children 31-510, round 2
children from 511 up.  Against the number T of heap slots kept in LDS a round
takes a plain LDS access, a plain HBM access or the general one, and a failed
placement's first scan step (slots below 31) does the same.

The small workloads of `scan_deletion_shapes` keep their heaps below 512
entries, so no pop of theirs reaches round 2.  `large()` does: 1,200 pods on 12
nodes (a row with four idle lanes), 300 of them created within the first three
ticks, which overload the cluster while the heap still holds more than 1,023
entries, 820 spread thinly over the rest of the trace, so the replay stays
short, and 80 more within three ticks near its end, which overload the cluster
again when the heap is down to a few levels; it then drains to nothing.
`tests/test_rows_level_access_shapes.py` checks those properties on the CPU;
`tests/test_gpu_rows_level_access.py` holds the device to the CPU oracle.
"""
import functools

import numpy as np

import device_shapes as ds
import scan_deletion_shapes as sd
from funsearch_kubernetes_simulator_amd.core.arrays import Workload

#: heap slots kept in LDS: every pair of neighbours puts one round (or the first
#: scan step) once wholly in LDS and once not -- 15 | 31: round 0 and the first
#: scan step; 127 | 511: round 1; 511 | 1023: round 2; 1: all of it in HBM
TOPS = (1, 15, 31, 127, 511, 1023)

N_BURST, N_REST, N_LATE = 300, 820, 80
SPAN = 30000


@functools.lru_cache(maxsize=None)
def large() -> Workload:
    rng = np.random.default_rng(11)
    nodes = ds._nodes(rng, 12, gpus=(4, 2, 8, 1, 0))
    pods = ds._pods(rng, N_BURST, 3, dur=(30, 200), prefix="b")
    pods += ds._pods(rng, N_REST, SPAN, dur=(20, 120), prefix="r")
    late = ds._pods(rng, N_LATE, 3, dur=(30, 200), prefix="l")
    for p in late:
        p.creation_time += SPAN - 600
    pods += late
    return ds._workload(nodes, pods, "level_access_large")


#: the large workload and one small shape of the scan-deletion tests
WORKLOADS = {"large": large, "b_hogs": sd.workload}

#: the 37-policy batches of the scan-deletion tests
P = sd.P
batches = sd.batches
