"""Workloads for the row kernel's fragmentation-sample reuse.

A failed placement samples fragmentation from the row's per-GPU milli left
and its smallest waiting gpu_milli class.  The row kernel keeps the last
sample and reuses it while neither can have changed: no deletion, no
placement and no first failure of a GPU pod in between.  The two workloads
here are small clusters (3 and 4 nodes) under so much load that pods retry
thousands of times, with every kind of event between two failures;
`tests/test_rows_frag_reuse_shapes.py` counts those on the CPython object
engine and `tests/test_gpu_rows_frag_reuse.py` holds the device to the CPU
oracle on them.
"""
import functools

import numpy as np

import device_shapes as ds
from funsearch_kubernetes_simulator_amd.core.arrays import Workload
from funsearch_kubernetes_simulator_amd.core.model import Pod
from funsearch_kubernetes_simulator_amd.models import families as fam

N_CANDIDATES = 12
#: gpu_milli of workload A's one-GPU pods by fifth of the creation span: later
#: arrivals lower the smallest waiting class
A_MILLI = (1000, 750, 500, 250, 100)


def _a_objects():
    rng = np.random.default_rng(21)
    nodes = ds._nodes(rng, 3, gpus=(2, 4, 1))
    pods = ds._pods(rng, 300, 300, dur=(40, 300), ngpu=(0, 1, 1, 1, 1, 1, 2), gmilli=(1000,))
    for p in pods:
        if p.num_gpu == 1:
            p.gpu_milli = A_MILLI[min(4, p.creation_time * 5 // 301)]
    return nodes, pods


@functools.lru_cache(maxsize=None)
def workload_a() -> Workload:
    """3 nodes (2 / 4 / 1 GPUs), 300 pods."""
    nodes, pods = _a_objects()
    return ds._workload(nodes, pods, "frag_reuse_a")


@functools.lru_cache(maxsize=None)
def workload_b() -> Workload:
    """4 nodes (4 / 2 / 8 / 1 GPUs), 360 pods with the catalogue's gpu_milli mix."""
    rng = np.random.default_rng(7)
    nodes = ds._nodes(rng, 4, gpus=(4, 2, 8, 1))
    return ds._workload(nodes, ds._pods(rng, 360, 400, dur=(50, 400)), "frag_reuse_b")


@functools.lru_cache(maxsize=None)
def workload_a_cpu_hog() -> Workload:
    """Workload A plus one pod at time 0 that asks for no GPU and for more cpu
    than any node has: its first failure adds no waiting class, so only the
    reset at the start of a replay keeps a row from reusing what the policy
    before it left behind."""
    nodes, pods = _a_objects()
    most = max(n.cpu_milli_total for n in nodes.values())
    pods.insert(0, Pod("hog00000", most + 1, 0, 0, 0, "", 0, 50))
    return ds._workload(nodes, pods, "frag_reuse_a_cpu_hog")


P_SWITCH = 37


@functools.lru_cache(maxsize=None)
def switch_batch():
    """(weights [37, 16], marked [37]): ordinary composite candidates alternate
    with marked ones that overflow mid-replay on a weight of 1e308: weight 13
    (GPU slack; fires on the first shared-GPU pod that fits, before any
    sample is above 0) and weight 12 (nearly full node; fires later, with a
    sample above 0 in the row) in turn."""
    w = fam.pad_weights(fam.sample_composite_linear(P_SWITCH, np.random.default_rng(5)))
    marked = np.arange(P_SWITCH) % 2 == 1
    w[1::4, 13] = 1e308
    w[3::4, 12] = 1e308
    w.setflags(write=False)
    marked.setflags(write=False)
    return w, marked


@functools.lru_cache(maxsize=None)
def composite_candidates() -> np.ndarray:
    w = fam.pad_weights(fam.sample_composite_linear(N_CANDIDATES, np.random.default_rng(3)))
    w.setflags(write=False)
    return w
