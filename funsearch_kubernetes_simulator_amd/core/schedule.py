"""What a replay did: each pod's node, GPUs and start time.

Every engine answers "how good is this policy?" with a 13-column row; a
`ScheduleBatch` answers "what did it do?" for the same replays.  The CPU
oracle (`ops.cpu_engine.schedule_*`) and the device's schedule launches
(`ops.hip_engine.DeviceEvaluator.schedule_*`) both return one, in trace pod
order, so two engines' replays are compared with one array comparison
(`Schedule.first_difference`), and a schedule is checked against the workload
alone, without any engine (`Schedule.validate`).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .arrays import Workload

#: columns of the result rows used here (ops.cpu_engine.RESULT_COLUMNS)
_N_UNPLACED, _EXC = 9, 10


class ScheduleError(ValueError):
    """`Schedule.validate` found a violation; `pod` is the trace index of the
    pod it names (None for a count that names no pod)."""

    def __init__(self, message: str, pod: Optional[int] = None):
        super().__init__(message)
        self.pod = pod


def _running(keys: np.ndarray, delta: np.ndarray) -> np.ndarray:
    """Running sum of `delta` within each `keys` group, in array order."""
    o = np.argsort(keys, kind="stable")
    d, k = delta[o], keys[o]
    cs = np.cumsum(d)
    first = np.ones(len(k), dtype=bool)
    first[1:] = k[1:] != k[:-1]
    base = (cs - d)[first]
    run = cs - base[np.cumsum(first) - 1]
    out = np.empty_like(run)
    out[o] = run
    return out


def _time_record_ints(node: np.ndarray, start: np.ndarray, workload: Workload) -> np.ndarray:
    """One schedule's record with Python ints throughout (any magnitude short of the record's 64 bits)."""
    from .time_metrics import RECORD_WORDS, wait_bucket
    p = workload.pods
    slots = [0] * 8
    hist = [0] * 32
    for i in np.flatnonzero(node >= 0):
        t, dur = int(start[i]), int(p.pod_dur[i])
        wait = t - int(p.pod_ctime[i])
        ngpu = int(p.pod_ngpu[i])
        slots[0] += wait
        slots[1] = max(slots[1], wait)
        slots[2] = max(slots[2], t + dur)
        slots[3] += int(p.pod_cpu[i]) * dur
        slots[4] += int(p.pod_mem[i]) * dur
        slots[5] += ngpu * dur
        slots[6] += ngpu * int(p.pod_gmilli[i]) * dur
        slots[7] += 1
        hist[wait_bucket(wait)] += 1
    rec = np.zeros(RECORD_WORDS, dtype=np.int64)
    rec[:8] = slots
    rec[8:] = np.array(hist, dtype=np.uint32).view(np.int64)
    return rec


def _time_records(node: np.ndarray, start: np.ndarray, workload: Workload, chunk: int = 128) -> np.ndarray:
    """Time-metrics records [P, 24] int64 of schedules `node`, `start` [P, n_pods]
    (`core.time_metrics`), from the schedules and the workload alone.  int64
    numpy sums where Python ints show that none can overflow (every term is
    >= 0 for a valid schedule, so the sums over all pods bound them), else
    Python ints pod by pod."""
    from .time_metrics import RECORD_WORDS
    p = workload.pods
    P, n = node.shape
    rec = np.zeros((P, RECORD_WORDS), dtype=np.int64)
    if P == 0 or n == 0:
        return rec
    dur = p.pod_dur.astype(np.int64)
    ctime = p.pod_ctime.astype(np.int64)
    ngpu = p.pod_ngpu.astype(np.int64)
    cols = (p.pod_cpu.astype(np.int64), p.pod_mem.astype(np.int64), ngpu, ngpu * p.pod_gmilli.astype(np.int64))
    t_hi = max(int(start.max()), 0)
    bound = max([n * t_hi + sum(int(d) for d in dur)] + [sum(abs(int(x)) * abs(int(d)) for x, d in zip(c, dur)) for c in cols])
    if bound >= 2 ** 62 or int(min(c.min() for c in cols + (dur,))) < 0:
        for i in range(P):
            rec[i] = _time_record_ints(node[i], start[i], workload)
        return rec
    prods = [c * dur for c in cols]
    edges = np.int64(1) << np.arange(63, dtype=np.int64)   # bit_length(w) = edges <= w, counted
    for lo in range(0, P, chunk):
        placed = node[lo:lo + chunk] >= 0
        st = start[lo:lo + chunk].astype(np.int64)
        wait = np.where(placed, st - ctime, 0)
        rec[lo:lo + chunk, 0] = wait.sum(axis=1)
        rec[lo:lo + chunk, 1] = wait.max(axis=1)
        rec[lo:lo + chunk, 2] = np.where(placed, st + dur, 0).max(axis=1)
        for k, pr in enumerate(prods):
            rec[lo:lo + chunk, 3 + k] = np.where(placed, pr, 0).sum(axis=1)
        rec[lo:lo + chunk, 7] = placed.sum(axis=1)
        bucket = np.minimum(np.searchsorted(edges, wait.ravel(), side="right"), 31).reshape(wait.shape)
        bucket = np.where(placed, bucket, 32)   # (a pod never placed: counted nowhere)
        hist = np.zeros((len(placed), 33), dtype=np.int64)
        np.add.at(hist, (np.arange(len(placed))[:, None], bucket), 1)
        rec[lo:lo + chunk, 8:] = hist[:, :32].astype(np.uint32).view(np.int64)
    return rec


@dataclass
class Schedule:
    """One policy's schedule, in trace pod order."""

    node: np.ndarray       # int32 [n_pods], node index, -1 never placed
    gpu_mask: np.ndarray   # uint8 [n_pods], bit j = GPU j of that node
    start: np.ndarray      # int64 [n_pods], time of the creation event that placed the pod, -1 never placed
    row: np.ndarray        # the replay's 13-column result row
    engine: str = ""
    node_ids: Optional[List[str]] = None   # the cluster's node ids (set by ScheduleBatch; `apply` needs them)

    @property
    def n_pods(self) -> int:
        return len(self.node)

    def gpus(self, pod: int) -> Tuple[int, ...]:
        """The pod's GPU indexes on its node, ascending."""
        m = int(self.gpu_mask[pod])
        return tuple(j for j in range(8) if (m >> j) & 1)

    def wait(self, workload: Workload) -> np.ndarray:
        """Start minus original creation time per pod (trace seconds; -1 for a pod never placed)."""
        w = self.start - workload.pods.pod_ctime.astype(np.int64)
        return np.where(self.node >= 0, w, -1)

    def time_record(self, workload: Workload) -> np.ndarray:
        """The schedule's time-metrics record (`core.time_metrics`: 24 int64
        words) from the schedule and the workload alone -- plain numpy and
        Python ints, no engine."""
        return _time_records(self.node[None], self.start[None], workload)[0]

    def time_metrics(self, workload: Workload):
        """`TimeMetricsBatch` of this one schedule (all zero if its replay raised)."""
        from .time_metrics import TimeMetricsBatch
        return TimeMetricsBatch.from_records(np.asarray(self.row)[None], self.time_record(workload)[None],
                                             self.engine, workload)

    def first_difference(self, other: "Schedule", workload: Optional[Workload] = None) -> Optional[int]:
        """Trace index of the first pod, in (start, rank) order, whose record
        differs between the two schedules, or None.  A pod's place in that
        order is the earlier of its two starts (a pod one side never placed
        counts by the other side's start; placed by neither, it comes last).
        Without a workload the trace index stands in for the rank."""
        diff = (self.node != other.node) | (self.gpu_mask != other.gpu_mask) | (self.start != other.start)
        idx = np.flatnonzero(diff)
        if idx.size == 0:
            return None
        big = np.iinfo(np.int64).max
        a = np.where(self.start[idx] < 0, big, self.start[idx])
        b = np.where(other.start[idx] < 0, big, other.start[idx])
        rank = workload.pods.pod_rank[idx] if workload is not None else idx
        return int(idx[np.lexsort((rank, np.minimum(a, b)))[0]])

    def apply(self, pods: Sequence) -> None:
        """Set `assigned_node` (the node id), `assigned_gpus` and
        `creation_time` on `core.model.Pod` objects, as a reference run leaves
        them on placed pods; pods never placed are left alone.
        `assigned_gpus` is ascending here; the reference's best-fit allocation
        lists them in allocation order (by milli left).  Nothing reads the
        order of that list."""
        if self.node_ids is None:
            raise ValueError("apply() needs the node ids: take the schedule from a ScheduleBatch")
        if len(pods) != self.n_pods:
            raise ValueError("pods do not match the schedule")
        for i, pod in enumerate(pods):
            if self.node[i] < 0:
                continue
            pod.assigned_node = self.node_ids[int(self.node[i])]
            pod.assigned_gpus = list(self.gpus(i))
            pod.creation_time = int(self.start[i])

    def validate(self, workload: Workload) -> Dict[str, int]:
        """Check the schedule against the workload alone (no engine): raises
        `ScheduleError` with the first violation, returns counts otherwise.

        * every placed pod's mask has `num_gpu` bits, all below its node's GPU
          count, and the pod starts at or after its creation time;
        * sweeping the start and end (start + duration) events of the placed
          pods in (time, rank, kind) order, start before end -- the event
          heap's order --, no node's cpu / memory / GPU count and no GPU's
          milli goes below zero from the workload's initial `*_left`;
        * the pods at node -1 are as many as the row's `n_unplaced`.
        """
        c, p = workload.cluster, workload.pods
        n = p.n_pods
        if not (len(self.node) == len(self.gpu_mask) == len(self.start) == n):
            raise ScheduleError(f"schedule of {len(self.node)} pods, workload of {n}")
        node = self.node.astype(np.int64)
        mask = self.gpu_mask.astype(np.int64)
        start = self.start.astype(np.int64)

        def name(i):
            return f"pod {p.pod_ids[i]} (trace index {i}, rank {int(p.pod_rank[i])})"

        def fail(i, what):
            raise ScheduleError(f"{name(int(i))}: {what}", int(i))

        placed = node >= 0
        bad = np.flatnonzero((node < -1) | (node >= c.n_nodes))
        if bad.size:
            fail(bad[0], f"node {node[bad[0]]} is not one of the cluster's {c.n_nodes}")
        bad = np.flatnonzero(~placed & ((mask != 0) | (start != -1)))
        if bad.size:
            fail(bad[0], f"never placed, yet GPU mask {mask[bad[0]]:#x} and start {start[bad[0]]}")
        pi = np.flatnonzero(placed)
        pn = node[pi]
        bits = np.array([bin(int(m)).count("1") for m in mask[pi]], dtype=np.int64)
        bad = np.flatnonzero(bits != p.pod_ngpu[pi])
        if bad.size:
            i = pi[bad[0]]
            fail(i, f"GPU mask {mask[i]:#x} holds {bits[bad[0]]} GPUs, the pod asks for num_gpu = {int(p.pod_ngpu[i])}")
        bad = np.flatnonzero((mask[pi] >> c.node_ngpus[pn].astype(np.int64)) != 0)
        if bad.size:
            i = pi[bad[0]]
            fail(i, f"GPU mask {mask[i]:#x} has a bit past the GPU count {int(c.node_ngpus[node[i]])} of node {node[i]}")
        bad = np.flatnonzero(start[pi] < p.pod_ctime[pi])
        if bad.size:
            i = pi[bad[0]]
            fail(i, f"starts at {start[i]}, before its creation time {int(p.pod_ctime[i])}")

        # ---- the sweep: start (kind 0) and end (kind 1) events in heap order
        k = len(pi)
        ev_pod = np.concatenate([pi, pi])
        ev_kind = np.concatenate([np.zeros(k, np.int64), np.ones(k, np.int64)])
        ev_time = np.concatenate([start[pi], start[pi] + p.pod_dur[pi].astype(np.int64)])
        order = np.lexsort((ev_kind, p.pod_rank[ev_pod], ev_time))
        ev_pod, ev_kind, ev_time = ev_pod[order], ev_kind[order], ev_time[order]
        sign = np.where(ev_kind == 0, -1, 1).astype(np.int64)
        ev_node = node[ev_pod]
        worst: Optional[Tuple[int, int, str]] = None   # (event position, pod, what)

        def check(keys, delta, left0, pos, what):
            nonlocal worst
            if len(keys) == 0:
                return
            left = left0[keys] + _running(keys, delta)
            b = np.flatnonzero(left < 0)
            if b.size and (worst is None or pos[b[0]] < worst[0]):
                j = b[0]
                worst = (int(pos[j]), int(ev_pod[pos[j]]), what(int(keys[j]), int(left[j])))

        pos = np.arange(2 * k)
        for label, req, left0 in (("cpu", p.pod_cpu, c.node_cpu_left), ("memory", p.pod_mem, c.node_mem_left),
                                  ("GPU count", p.pod_ngpu, c.node_gpu_left)):
            check(ev_node, sign * req[ev_pod].astype(np.int64), left0.astype(np.int64), pos,
                  lambda nd, left, label=label: f"node {nd} has {label} {left} left, below zero")
        # per-GPU milli: one event per bit of the mask
        gk, gd, gp = [], [], []
        for j in range(8):
            sel = np.flatnonzero((mask[ev_pod] >> j) & 1)
            gk.append(c.gpu_start[ev_node[sel]].astype(np.int64) + j)
            gd.append(sign[sel] * p.pod_gmilli[ev_pod[sel]].astype(np.int64))
            gp.append(sel)
        gk, gd, gp = np.concatenate(gk), np.concatenate(gd), np.concatenate(gp)
        o = np.argsort(gp, kind="stable")
        gpu_node = np.repeat(np.arange(c.n_nodes), np.diff(c.gpu_start))
        check(gk[o], gd[o], c.gpu_milli_left.astype(np.int64), gp[o],
              lambda g, left: f"GPU {g - int(c.gpu_start[gpu_node[g]])} of node {int(gpu_node[g])} has milli {left} "
                              f"left, below zero")
        if worst is not None:
            when = int(ev_time[worst[0]])
            fail(worst[1], f"at its {'start' if ev_kind[worst[0]] == 0 else 'end'} (t = {when}) {worst[2]}")

        unplaced = int((node == -1).sum())
        want = int(self.row[_N_UNPLACED])
        if unplaced != want:
            raise ScheduleError(f"{unplaced} pods at node -1, the row's n_unplaced is {want}")
        return {"pods": n, "placed": int(k), "unplaced": unplaced, "events": int(2 * k),
                "gpu_pods": int((p.pod_ngpu[pi] > 0).sum()), "delayed": int((start[pi] > p.pod_ctime[pi]).sum())}


@dataclass
class ScheduleBatch:
    """The schedules of a policy batch, in trace pod order.  Rows with
    `exc != 0` have every pod at -1 / 0 / -1, whatever an engine had recorded
    before the replay stopped."""

    node: np.ndarray       # int32 [P, n_pods]
    gpu_mask: np.ndarray   # uint8 [P, n_pods]
    start: np.ndarray      # int64 [P, n_pods]
    rows: np.ndarray       # float64 [P, 13]
    engine: List[str]
    node_ids: Optional[List[str]] = None

    def __post_init__(self):
        self.node = np.ascontiguousarray(self.node, dtype=np.int32)
        self.gpu_mask = np.ascontiguousarray(self.gpu_mask, dtype=np.uint8)
        self.start = np.ascontiguousarray(self.start, dtype=np.int64)
        raised = np.flatnonzero(np.asarray(self.rows)[:, _EXC] != 0) if len(self.rows) else []
        for i in raised:
            self.node[i], self.gpu_mask[i], self.start[i] = -1, 0, -1

    def __len__(self) -> int:
        return len(self.rows)

    def __getitem__(self, i: int) -> Schedule:
        i = range(len(self))[i]
        return Schedule(self.node[i], self.gpu_mask[i], self.start[i], self.rows[i], self.engine[i], self.node_ids)

    def time_metrics(self, workload: Workload):
        """`TimeMetricsBatch` derived from the schedules and the workload alone
        (no engine): the reference every engine's time mode is held to."""
        from .time_metrics import TimeMetricsBatch
        rec = _time_records(self.node, self.start, workload)
        return TimeMetricsBatch.from_records(self.rows, rec, list(self.engine), workload)

    @classmethod
    def empty(cls, n: int, n_pods: int, node_ids=None) -> "ScheduleBatch":
        """`n` policies with nothing placed and zero rows, to be filled by `put`."""
        return cls(np.full((n, n_pods), -1, np.int32), np.zeros((n, n_pods), np.uint8),
                   np.full((n, n_pods), -1, np.int64), np.zeros((n, 13)), [""] * n, node_ids)

    def put(self, idx, other: "ScheduleBatch", sel=None) -> None:
        """Copy `other`'s policies `sel` (default: all) to positions `idx`."""
        sel = list(range(len(other))) if sel is None else list(sel)
        for i, j in zip(idx, sel):
            self.node[i], self.gpu_mask[i], self.start[i] = other.node[j], other.gpu_mask[j], other.start[j]
            self.rows[i] = other.rows[j]
            self.engine[i] = other.engine[j]

    @classmethod
    def from_ranked(cls, rows: np.ndarray, rec: np.ndarray, order: np.ndarray, engine: str,
                    node_ids=None) -> "ScheduleBatch":
        """From device records `rec` [P, n_pods, 4] int32 (start lo, start hi,
        node, GPU mask) indexed by pod rank; `order[r]` is the trace index of
        rank r (`prepare_device_workload`'s pod order)."""
        P, n = rec.shape[0], rec.shape[1]
        rec = np.ascontiguousarray(rec, dtype=np.int32)
        start_r = rec[:, :, 0:2].copy().view(np.int64).reshape(P, n)
        node = np.empty((P, n), np.int32)
        mask = np.empty((P, n), np.uint8)
        start = np.empty((P, n), np.int64)
        node[:, order] = rec[:, :, 2]
        unplaced = rec[:, :, 2] < 0
        mask[:, order] = np.where(unplaced, 0, rec[:, :, 3]).astype(np.uint8)
        start[:, order] = start_r
        return cls(node, mask, start, np.array(rows, dtype=np.float64), [engine] * P, node_ids)
