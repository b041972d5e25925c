"""Workload and batches for the row kernel's first-pending-deletion scan.

A failed placement re-queues its pod one tick after the first DELETION of the
event heap in array order.  The row kernel (csrc/hip/replay_rows.hip.h,
`RowHeapT::scan_deletion`) keeps no bitmap of those: it reads the keys, 32
slots per step, one aligned pair per lane, across the boundary between the
LDS heap top and the HBM slice.  The workload here is `frag_reuse_shapes`'
overloaded workload B (4 nodes, 360 pods, tens of thousands of failed
placements with up to ~190 retries waiting in front of the first deletion)
plus four pods that fit no node, so that some failures find no deletion at
all: one at time 0 (the heap still holds every other pod) and three after
everything else has run (2, 1 and 0 entries left).
Two queue workloads add the one position that replay does not reach: a heap
of n = 32 k entries whose only deletion sits in slot n - 1, the slot that opens
a scan step of its own.  One node, one pod running at a time and 70 or 153
identical pods waiting behind it: a placed pod's deletion is pushed below
every retry, and the next pop sinks it along the leftmost path to the last
slot at n = 32 and 64 (70 waiting) and n = 64 and 128 (153 waiting).
`tests/test_rows_scan_deletion_shapes.py` records on the CPython object engine
where the first deletion lies at every failure;
`tests/test_gpu_rows_scan_deletion.py` holds the device to the CPU oracle.
"""
import functools

import numpy as np

import device_shapes as ds
from funsearch_kubernetes_simulator_amd.core.arrays import Workload
from funsearch_kubernetes_simulator_amd.core.model import Pod
from funsearch_kubernetes_simulator_amd.models import families as fam

P = 37
#: creation time of the three late pods: past every deletion of the replay
LATE = 1_000_000


@functools.lru_cache(maxsize=None)
def workload() -> Workload:
    """`frag_reuse_shapes.workload_b` plus four CPU-only pods no node can hold."""
    rng = np.random.default_rng(7)
    nodes = ds._nodes(rng, 4, gpus=(4, 2, 8, 1))
    pods = ds._pods(rng, 360, 400, dur=(50, 400))
    most = max(n.cpu_milli_total for n in nodes.values())
    pods.insert(0, Pod("hog00000", most + 1, 0, 0, 0, "", 0, 50))
    pods += [Pod(f"hog{k:05d}", most + 1, 0, 0, 0, "", LATE + k, 50) for k in (1, 2, 3)]
    return ds._workload(nodes, pods, "scan_deletion_b_hogs")


#: waiting pods of the two queue workloads -> heap lengths n = 32 k at which
#: the only deletion is found in slot n - 1
QUEUES = {70: (32, 64), 153: (64, 128)}


@functools.lru_cache(maxsize=None)
def queue(waiting: int) -> Workload:
    """One CPU-only node; a pod at time 0 and `waiting` identical pods at time
    1, each asking for 60 % of the node's cpu and running 7 ticks."""
    nodes = ds._nodes(np.random.default_rng(1), 1, gpus=(0,))
    need = int(0.6 * min(n.cpu_milli_total for n in nodes.values()))
    pods = [Pod(f"q{k:05d}", need, 1, 0, 0, "", 0 if k < 1 else 1, 7) for k in range(waiting + 1)]
    return ds._workload(nodes, pods, f"scan_deletion_queue{waiting}")


WORKLOADS = {"b_hogs": workload, "queue70": functools.partial(queue, 70), "queue153": functools.partial(queue, 153)}


@functools.lru_cache(maxsize=None)
def batches() -> dict:
    """name -> (family or per-policy families, weights [37, 16])"""
    rng = np.random.default_rng(4)
    comp = fam.pad_weights(fam.sample_composite_linear(P, np.random.default_rng(3)))
    rand = fam.pad_weights(fam.sample_random_linear(P, rng))
    feat = fam.pad_weights(fam.sample_feature_linear(P, rng))
    order = ("first_fit", "composite_linear", "best_fit", "feature_linear", "random_linear")
    names = [order[i % 5] for i in range(P)]
    mixed = np.zeros((P, 16))
    for i, f in enumerate(names):
        mixed[i] = {"composite_linear": comp, "random_linear": rand, "feature_linear": feat}.get(f, mixed)[i]
    out = {"composite_linear": ("composite_linear", comp), "random_linear": ("random_linear", rand),
           "mixed": (names, mixed)}
    for _, w in out.values():
        w.setflags(write=False)
    return out


#: scores every node it is called for -1: nothing is ever placed, so every pod
#: fails once with no deletion pending, at every heap length from N - 1 down to 0
NEVER = "return -1"
#: places a pod only on a node with more than three GPUs left: feasible nodes
#: score <= 0 too, and the pods they turn away retry behind the deletions
PICKY = "return node.gpu_left - 3"


@functools.lru_cache(maxsize=None)
def program_texts():
    """Two corpus programs and the two above (feasibility prologue first)."""
    from program_corpus import PROLOGUE
    corpus = [c for c in ds.program_groups()["corpus"]][:2]
    return corpus + [PROLOGUE + NEVER + "\n", PROLOGUE + PICKY + "\n"]


@functools.lru_cache(maxsize=None)
def programs():
    from funsearch_kubernetes_simulator_amd.policy.compiler import compile_policy
    return [compile_policy(c) for c in program_texts()]
