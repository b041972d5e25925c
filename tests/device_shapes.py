"""Catalogue of cluster / trace shapes for the device engines.

The shipped cluster has 16 nodes and the synthetic 256-node one tiles them, so
on both every 64-lane pass of the replay kernels is full, every 16-lane row is
full and every host gate (`rows_ok_`, `fast_div`, `cap_recips`, `frag_recip`,
the `tot_gcnt` test, the packed key widths) takes one side only.  The shapes
here sit on the other sides.  Each is a deterministic, seeded `Workload`
that builds in well under a second; `tests/test_device_shapes.py` holds the
CPU preconditions (the oracle equals the CPython object engine on them, the
candidates are told apart, placements fail) and `tests/test_gpu_shapes.py`
holds the device to the oracle on them.

Two groups:

* `sweep(N)`: `synthetic_workload(n_nodes=N, ...)` with compressed creation
  times, N over every lane boundary (`SWEEP_NODES`);
* hand-built shapes from `core.model` objects (`HAND_BUILT`).
"""
import functools

import numpy as np

from funsearch_kubernetes_simulator_amd.core import load_default_workload, synthetic_workload
from funsearch_kubernetes_simulator_amd.core.arrays import Workload
from funsearch_kubernetes_simulator_amd.core.model import GPU, Cluster, Node, Pod
from funsearch_kubernetes_simulator_amd.models import families as fam

#: row kernel with partly filled rows | NPASS 1 wave kernel | NPASS 2 | NPASS 4 with a
#: partly filled last pass (129: one node in pass 2, pass 3 empty)
SWEEP_NODES = (1, 2, 5, 15, 17, 33, 63, 64, 65, 100, 127, 128, 129, 193, 255)

#: (pods, creation-time divisor) of the smallest sweep shapes: at 40 pods per
#: node and // 32 these clusters are so overloaded that every candidate drops
#: the same pods; a longer, less compressed trace lets the node choice matter
_SMALL_SWEEP = {1: (120, 4), 2: (300, 4), 5: (500, 16)}

FAMILIES = ("random_linear", "feature_linear", "composite_linear")
#: weighted candidates per family; the batches add rows so that no batch size is
#: a multiple of 4 (the last row-kernel wave keeps idle rows)
N_CANDIDATES = 12


def expected_npass(n_nodes: int) -> int:
    return 1 if n_nodes <= 64 else (2 if n_nodes <= 128 else 4)


@functools.lru_cache(maxsize=None)
def _base() -> Workload:
    return load_default_workload()


@functools.lru_cache(maxsize=None)
def sweep(n_nodes: int) -> Workload:
    n_pods, div = _SMALL_SWEEP.get(n_nodes, (max(300, 40 * n_nodes), 32))
    w = synthetic_workload(n_nodes=n_nodes, n_pods=n_pods, seed=n_nodes, base=_base())
    w.pods.pod_ctime[:] = w.pods.pod_ctime // div
    w.name = f"sweep{n_nodes:03d}"
    return w


# ---- hand-built shapes ----------------------------------------------------------------

def _nodes(rng, n, gpus=(0, 1, 2, 4, 8), milli=1000, cpu=(8000, 64000), mem=(16384, 262144)):
    """n heterogeneous nodes; `gpus` is cycled, cpu / mem are drawn per node."""
    nodes = {}
    for i in range(n):
        ng = gpus[i % len(gpus)]
        c, m = int(rng.integers(*cpu)), int(rng.integers(*mem))
        nodes[f"n{i:03d}"] = Node(f"n{i:03d}", c, c, m, m, ng, [GPU(16384, 16384, milli, milli) for _ in range(ng)])
    return nodes


def _pods(rng, n, span, dur=(20, 600), ngpu=(0, 0, 1, 1, 1, 1, 2, 4, 8), gmilli=(100, 250, 500, 750, 1000),
          whole=1000, cpu=(200, 24000), mem=(0, 90000), prefix="p"):
    """n pods created over [0, span]; one-GPU pods ask for a share out of
    `gmilli`, multi-GPU pods for `whole` GPUs (as in the OpenB trace)."""
    pods = []
    for j in range(n):
        g = int(rng.choice(ngpu))
        gm = int(rng.choice(gmilli)) if g == 1 else (whole if g > 1 else 0)
        pods.append(Pod(f"{prefix}{j:05d}", int(rng.integers(*cpu)), int(rng.integers(*mem)), g, gm, "",
                        int(rng.integers(0, span + 1)), int(rng.integers(*dur))))
    return pods


def _workload(nodes, pods, name) -> Workload:
    return Workload.from_objects(Cluster(nodes), pods, name)


def one_node_one_pod() -> Workload:
    """(a)"""
    node = Node("n000", 32000, 32000, 65536, 65536, 2, [GPU(16384, 16384, 1000, 1000) for _ in range(2)])
    return _workload({"n000": node}, [Pod("p00000", 1000, 2048, 1, 500, "", 3, 10)], "a_one_node_one_pod")


def no_gpu_cluster() -> Workload:
    """(b) tot_gcnt == 0 and tot_gmilli == 0; the GPU pods can never be placed."""
    rng = np.random.default_rng(102)
    return _workload(_nodes(rng, 20, gpus=(0,)), _pods(rng, 500, 400, ngpu=(0, 0, 0, 0, 1, 2)), "b_no_gpu_cluster")


def hetero100() -> Workload:
    """(c) 100 nodes (NPASS 2; pass 1 holds lanes 0..35), 0 / 1 / 2 / 4 / 8 GPUs,
    cpu and mem per node; node 99 -- the last occupied lane -- has no GPU."""
    rng = np.random.default_rng(103)
    nodes = _nodes(rng, 100, gpus=(2, 0, 8, 1, 4, 4, 0))
    last = nodes["n099"]
    last.gpus, last.gpu_left = [], 0
    return _workload(nodes, _pods(rng, 3000, 10000), "c_hetero100")


def partly_used() -> Workload:
    """(d) the cluster starts with cpu, memory, whole GPUs and GPU shares taken
    (used_* totals non-zero); every GPU has a milli total of 1000."""
    rng = np.random.default_rng(104)
    nodes = _nodes(rng, 12, gpus=(4, 2, 0, 8))
    for i, n in enumerate(nodes.values()):
        n.cpu_milli_left -= int(rng.integers(0, n.cpu_milli_total // 2))
        n.memory_mib_left -= int(rng.integers(0, n.memory_mib_total // 2))
        if n.gpus and i % 3 != 2:
            n.gpu_left -= 1
            n.gpus[0].gpu_milli_left = 0
            if len(n.gpus) > 2:
                n.gpus[2].gpu_milli_left = 400
    return _workload(nodes, _pods(rng, 400, 4000), "d_partly_used")


def all_at_time_zero() -> Workload:
    """(e) every pod is created at time 0."""
    rng = np.random.default_rng(105)
    return _workload(_nodes(rng, 9, gpus=(2, 8, 0, 4)), _pods(rng, 300, 0), "e_all_at_time_zero")


def zero_durations() -> Workload:
    """(f) every third pod has duration 0."""
    rng = np.random.default_rng(106)
    pods = _pods(rng, 600, 300)
    for p in pods[::3]:
        p.duration_time = 0
    return _workload(_nodes(rng, 24), pods, "f_zero_durations")


def zero_requests(n_nodes: int, with_zero_pods: bool = True) -> Workload:
    """(g) pods that request nothing among normal pods.  A padding lane holds
    all-zero capacity, so such a pod is feasible there: only the `n_nodes`
    guard keeps it on a real node.  `with_zero_pods=False`: the same trace
    without them (the CPU precondition shows that they matter)."""
    rng = np.random.default_rng(107 + n_nodes)
    nodes = _nodes(rng, n_nodes, gpus=(1, 0, 2, 8))
    pods = _pods(rng, 30 * n_nodes, 2400 if n_nodes <= 16 else 6000)
    if with_zero_pods:
        for p in pods[::4]:
            p.cpu_milli, p.memory_mib, p.num_gpu, p.gpu_milli = 0, 0, 0, 0
    else:
        pods = [p for j, p in enumerate(pods) if j % 4]
    return _workload(nodes, pods, f"g_zero_requests{n_nodes}" + ("" if with_zero_pods else "_removed"))


def no_gpu_pods() -> Workload:
    """(h) no pod asks for a GPU (no gpu_milli class at all)."""
    rng = np.random.default_rng(108)
    return _workload(_nodes(rng, 10), _pods(rng, 350, 1600, ngpu=(0,), cpu=(2000, 40000)), "h_no_gpu_pods")


def rank_boundary(n_pods: int) -> Workload:
    """(i) 255 / 256 / 257 pods on one cluster: rank_bits goes from 8 to 9."""
    pods = _pods(np.random.default_rng(109), 257, 1500)[:n_pods]
    return _workload(_nodes(np.random.default_rng(1090), 10, gpus=(2, 8, 0)), pods, f"i_pods{n_pods}")


def many_classes() -> Workload:
    """(j) more than 64 distinct gpu_milli requests on 8 nodes: no row kernel."""
    rng = np.random.default_rng(110)
    pods = _pods(rng, 420, 300, ngpu=(0, 1, 1, 1, 1, 2), gmilli=tuple(range(10, 1000, 11)))
    assert len({p.gpu_milli for p in pods if p.num_gpu}) > 64
    return _workload(_nodes(rng, 8, gpus=(2, 8, 4)), pods, "j_many_classes")


def big_gpu_milli() -> Workload:
    """(k) 40 nodes x 8 GPUs x 60,000 milli: tot_gmilli > 2^24 (no reciprocal for
    the fragmentation share), per-GPU total < 2^16."""
    rng = np.random.default_rng(111)
    pods = _pods(rng, 1600, 6000, gmilli=(6000, 15000, 30000, 45000, 60000), whole=60000)
    return _workload(_nodes(rng, 40, gpus=(8,), milli=60000), pods, "k_big_gpu_milli")


def wide_gpu_milli(n_nodes: int = 12) -> Workload:
    """(l) GPU milli totals of 70,000 (>= 2^16) next to nodes with 1,000: no
    16-bit halves (row kernel off, unpacked registers), no common capacity
    divisor.  Above 128 nodes the device layout refuses it."""
    rng = np.random.default_rng(112)
    nodes = _nodes(rng, n_nodes, gpus=(4, 2, 0, 8), milli=70000)
    for i, n in enumerate(nodes.values()):
        if i % 3 == 1:
            n.gpus = [GPU(16384, 16384, 1000, 1000) for _ in n.gpus]
    pods = _pods(rng, 35 * n_nodes, 2400, gmilli=(500, 1000, 20000, 35000, 65000), whole=1000)
    return _workload(nodes, pods, f"l_wide_gpu_milli{n_nodes}")


def big_totals() -> Workload:
    """Three nodes with 2^31 / 3 MiB of memory among 10: the cluster total does
    not fit the row kernel's int32 totals (`rows_ok_` false), the wave kernel's
    64-bit ones hold it."""
    rng = np.random.default_rng(113)
    nodes = _nodes(rng, 10, gpus=(2, 0, 8))
    for n in list(nodes.values())[:3]:
        n.memory_mib_total = n.memory_mib_left = 2 ** 31 // 3 + 5
    return _workload(nodes, _pods(rng, 350, 4000, cpu=(2000, 40000)), "m_big_totals")


def left_over_total() -> Workload:
    """Two nodes that report more free cpu and memory than their totals: used
    amounts go negative, so the row kernel (unsigned utilisation accumulators)
    is not taken, and the host cannot bound the divisions' numerators, so no
    reciprocal is used (`fast_div` 0) and every division runs as a division."""
    rng = np.random.default_rng(114)
    nodes = _nodes(rng, 7, gpus=(2, 8, 0, 4))
    for n in list(nodes.values())[1:5:2]:
        n.cpu_milli_left += 1500
        n.memory_mib_left += 4096
    return _workload(nodes, _pods(rng, 300, 2400), "n_left_over_total")


HAND_BUILT = {
    "a_one_node_one_pod": one_node_one_pod,
    "b_no_gpu_cluster": no_gpu_cluster,
    "c_hetero100": hetero100,
    "d_partly_used": partly_used,
    "e_all_at_time_zero": all_at_time_zero,
    "f_zero_durations": zero_durations,
    "g_zero_requests13": functools.partial(zero_requests, 13),
    "g_zero_requests70": functools.partial(zero_requests, 70),
    "h_no_gpu_pods": no_gpu_pods,
    "i_pods255": functools.partial(rank_boundary, 255),
    "i_pods256": functools.partial(rank_boundary, 256),
    "i_pods257": functools.partial(rank_boundary, 257),
    "j_many_classes": many_classes,
    "k_big_gpu_milli": big_gpu_milli,
    "l_wide_gpu_milli12": wide_gpu_milli,
    "m_big_totals": big_totals,
    "n_left_over_total": left_over_total,
}

SWEEP = {f"sweep{n:03d}": functools.partial(sweep, n) for n in SWEEP_NODES}

#: every catalogue shape by name (the > 128-node variant of (l), which the
#: device refuses, is `wide_gpu_milli(130)`)
SHAPES = {**SWEEP, **HAND_BUILT}

#: shapes whose candidates need not be told apart (N < 5, (a), (b), (h)):
#: their expected rows are still compared
DISTINCT_EXEMPT = ("sweep001", "sweep002", "a_one_node_one_pod", "b_no_gpu_cluster", "h_no_gpu_pods")

#: what `DeviceEvaluator.info()` must report per shape (keys left out: either)
INFO = {
    "a_one_node_one_pod": {"row_kernel_ok": True, "frag_recip": True},
    "b_no_gpu_cluster": {"row_kernel_ok": False, "cap_recips": False, "frag_recip": False},
    "c_hetero100": {"npass": 2, "cap_recips": True, "frag_recip": True},
    "d_partly_used": {"row_kernel_ok": True, "fast_div": 1},
    "j_many_classes": {"row_kernel_ok": False},
    "k_big_gpu_milli": {"row_kernel_ok": False, "cap_recips": True, "frag_recip": False},
    "l_wide_gpu_milli12": {"row_kernel_ok": False, "cap_recips": False, "frag_recip": True},
    "m_big_totals": {"row_kernel_ok": False},
    "n_left_over_total": {"row_kernel_ok": False, "fast_div": 0},
}


@functools.lru_cache(maxsize=None)
def shape(name: str) -> Workload:
    return SHAPES[name]()


def n_nodes(name: str) -> int:
    return shape(name).cluster.n_nodes


def rows_expected(name: str) -> bool:
    """The row kernel takes the shape: <= 16 nodes and none of its gates closed."""
    return n_nodes(name) <= 16 and INFO.get(name, {}).get("row_kernel_ok", True)


def expected_info(name: str) -> dict:
    """The `DeviceEvaluator.info()` flags that name the path a shape takes:
    the rules of `DeviceEngine`, read off the workload, with `INFO` on top."""
    c = shape(name).cluster
    gpu_nodes = c.node_ngpus > 0
    per_node = c.gpu_milli_total[c.gpu_start[:-1][gpu_nodes]]
    tot = int(c.gpu_milli_total.astype(np.int64).sum())
    out = {"npass": expected_npass(c.n_nodes), "row_kernel_ok": rows_expected(name), "fast_div": 1,
           "cap_recips": bool(gpu_nodes.any() and len(set(per_node.tolist())) == 1),
           "frag_recip": 0 < tot <= 2 ** 24}
    out.update(INFO.get(name, {}))
    return out


#: families with an "aborts_<family>" batch (`abort_rows` of the family's first candidate)
ABORT_FAMILIES = ("random_linear", "feature_linear")
ABORT_BATCHES = tuple(f"aborts_{f}" for f in ABORT_FAMILIES)


def abort_rows(row: np.ndarray) -> np.ndarray:
    """Five rows: `row`, `row` with w[0] = inf, with w[0] = nan, `row` scaled
    by 1e290 and by 1e306 -- a clean replay beside three exception classes."""
    out = np.tile(np.asarray(row, dtype=np.float64), (5, 1))
    out[1, 0], out[2, 0] = np.inf, np.nan
    out[3] *= 1e290
    with np.errstate(over="ignore"):   # weights above 1e2 become inf
        out[4] *= 1e306
    return out


@functools.lru_cache(maxsize=None)
def candidates():
    """The builtin batches every shape is scored on: name -> (family or list
    of families, weights [P, 16] or None).  The first `N_CANDIDATES` rows of a
    weighted family are its candidates; the composite batch adds an all-zero
    row and a -0.0 row; the "aborts" batches hold rows that raise; no batch
    size is a multiple of 4."""
    rng = np.random.default_rng(2024)
    out = {"first_fit": ("first_fit", np.zeros((3, 16))), "best_fit": ("best_fit", np.zeros((3, 16)))}
    for f in FAMILIES:
        w = fam.pad_weights(fam.SAMPLERS[f](N_CANDIDATES + 1, rng))
        if f == "composite_linear":
            w = np.concatenate([w, np.zeros((2, 16))])
            w[-1, :] = -0.0
        out[f] = (f, w)
    order = ("first_fit", "composite_linear", "best_fit", "feature_linear", "random_linear")
    names = [order[i % 5] for i in range(11)]
    W = np.zeros((11, 16))
    for i, f in enumerate(names):
        if f in FAMILIES:
            W[i] = out[f][1][i]
    out["mixed"] = (names, W)
    # rows that raise: the sampled candidates never do, so these alone reach the
    # kernels' first-exception selection and the two-wave kernels' abort replies
    for f in ABORT_FAMILIES:
        out[f"aborts_{f}"] = (f, abort_rows(out[f][1][0]))
    assert all(len(w) % 4 for _, w in out.values())
    for _, w in out.values():
        w.setflags(write=False)
    return out


# ---- programs for the device VM and the native-program kernels --------------------------

#: one sweep shape per lane class, and hand-built (b), (c), (g)
PROGRAM_SHAPES = ("sweep005", "sweep015", "sweep033", "sweep064", "sweep065", "sweep128", "sweep129", "sweep255",
                  "b_no_gpu_cluster", "c_hetero100", "g_zero_requests13", "g_zero_requests70")
N_CORPUS = 16
#: programs replay the first pods of a shape only.  Some corpus programs score
#: most feasible nodes 0 and turn a whole compressed trace into a retry storm
#: (10^6 events and minutes of CPU VM time at 255 nodes; 14 s per device VM launch
#: at 33 nodes with 600 pods); on this prefix the CPU VM needs under 1 s per
#: shape for all programs, and 14 or more of the 35 still record fragmentation
#: events on every shape
PROGRAM_PODS = 400


@functools.lru_cache(maxsize=None)
def program_workload(name: str) -> Workload:
    w = shape(name)
    return Workload(w.cluster, w.pods.subset(np.arange(min(PROGRAM_PODS, w.pods.n_pods))), name + "_programs")


@functools.lru_cache(maxsize=None)
def program_groups():
    """Program texts by group: the reference policies, the seed policies, 3
    candidates of each weighted family as `fam.to_program` text, and the
    first 16 programs of `program_corpus` whose own code (after the
    feasibility prologue) loops over `node.gpus`, indexes it or takes
    `len(node.gpus)` -- the constructs whose result depends on the node's
    real GPU count, which a padding lane does not have."""
    from funsearch_kubernetes_simulator_amd.models.library import reference_policies, seed_policies
    from funsearch_kubernetes_simulator_amd.policy.compiler import CompileError, compile_policy
    from program_corpus import PROLOGUE, program_codes
    groups = {"reference": list(reference_policies().values()), "seed": list(seed_policies().values())}
    cands = candidates()
    groups["family"] = [fam.to_program(f, cands[f][1][i]) for f in FAMILIES for i in (0, 5, 11)]
    corpus = []
    for code in program_codes():
        if not code.startswith(PROLOGUE) or "node.gpus" not in code[len(PROLOGUE):]:
            continue
        try:
            compile_policy(code)
        except CompileError:
            continue
        corpus.append(code)
    groups["corpus"] = corpus[:N_CORPUS]
    return groups


@functools.lru_cache(maxsize=None)
def programs():
    """(group of each program, compiled programs), in group order."""
    from funsearch_kubernetes_simulator_amd.policy.compiler import compile_policy
    groups = program_groups()
    names = [g for g, codes in groups.items() for _ in codes]
    return names, [compile_policy(c) for codes in groups.values() for c in codes]


@functools.lru_cache(maxsize=None)
def program_oracle(name: str) -> np.ndarray:
    """CPU VM rows of `programs()` on `program_workload(name)`, computed once."""
    from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
    tab = ce.simulate_program_batch(program_workload(name), programs()[1])
    tab.setflags(write=False)
    return tab
