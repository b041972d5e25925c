"""CPU preconditions of the device shape tests (tests/test_gpu_shapes.py).

The reference side alone, on every shape of `device_shapes`:

* the device layout accepts the shape with the NPASS the catalogue claims
  (and refuses shape (l) above 128 nodes);
* the C++ oracle equals the CPython object engine there, so the rows the
  device is held to are the reference's;
* the candidates are told apart and placements fail, so a device that
  ignored the weights or never retried a pod could not pass;
* the zero-request pods of (g) change the outcome;
* the programs picked for the device VM / native tests are ones the CPU VM
  scores itself on every shape they run on.

Oracle time of the slowest shape (sweep255, 10,200 pods, 13 candidates of one
family, 16 threads): 0.5 s.
"""
import numpy as np
import pytest

import device_shapes as ds
from funsearch_kubernetes_simulator_amd.engine import object_engine_eval
from funsearch_kubernetes_simulator_amd.models import families as fam
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce
from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
from funsearch_kubernetes_simulator_amd.policy.bytecode import Exc

SMALL = [n for n in ds.SHAPES if n in ds.HAND_BUILT or ds.n_nodes(n) <= 17]


@pytest.mark.parametrize("name", list(ds.SHAPES))
def test_device_layout_accepts_shape(name):
    w = ds.shape(name)
    lay = he.prepare_device_workload(w)
    n = w.cluster.n_nodes
    assert lay["npass"] == ds.expected_npass(n) and lay["n_nodes"] == n and lay["n_pods"] == w.pods.n_pods
    assert lay["cpu_total"].size == 64 * lay["npass"] and not lay["cpu_total"][n:].any()   # padding lanes hold 0
    assert not lay["ngpus"][n:].any() and not lay["gml_total"][n:].any()


def test_sweep_covers_every_lane_class():
    ns = [ds.n_nodes(k) for k in ds.SWEEP]
    assert ns == list(ds.SWEEP_NODES)
    assert {ds.expected_npass(n) for n in ns} == {1, 2, 4}
    assert any(n < 16 for n in ns) and any(16 < n < 64 for n in ns) and any(128 < n < 192 for n in ns)


def test_layout_facts_the_shapes_are_built_for():
    lay = {k: he.prepare_device_workload(ds.shape(k)) for k in ds.HAND_BUILT}
    assert lay["b_no_gpu_cluster"]["tot_gcnt"] == 0 and lay["b_no_gpu_cluster"]["tot_gmilli"] == 0
    c = ds.shape("c_hetero100").cluster
    assert set(c.node_ngpus.tolist()) == {0, 1, 2, 4, 8} and c.node_ngpus[-1] == 0
    assert len(set(c.node_cpu_total.tolist())) > 90 and len(set(c.node_mem_total.tolist())) > 90
    d = lay["d_partly_used"]
    assert min(d["used_cpu"], d["used_mem"], d["used_gcnt"], d["used_gmilli"]) > 0
    assert not ds.shape("e_all_at_time_zero").pods.pod_ctime.any()
    assert (ds.shape("f_zero_durations").pods.pod_dur == 0).sum() >= 200
    for k in ("g_zero_requests13", "g_zero_requests70"):
        p = ds.shape(k).pods
        assert ((p.pod_cpu == 0) & (p.pod_mem == 0) & (p.pod_ngpu == 0)).sum() >= p.n_pods // 4
    # no GPU pod: the layout keeps one placeholder class
    assert not ds.shape("h_no_gpu_pods").pods.pod_ngpu.any() and lay["h_no_gpu_pods"]["n_classes"] == 1
    assert [lay[f"i_pods{n}"]["rank_bits"] for n in (255, 256, 257)] == [8, 8, 9]
    assert lay["j_many_classes"]["n_classes"] > 64 and ds.n_nodes("j_many_classes") <= 16
    k = ds.shape("k_big_gpu_milli").cluster
    assert lay["k_big_gpu_milli"]["tot_gmilli"] > 2 ** 24 and k.gpu_milli_total.max() < 2 ** 16
    assert ds.shape("l_wide_gpu_milli12").cluster.gpu_milli_total.max() >= 2 ** 16
    assert lay["m_big_totals"]["tot_mem"] >= 2 ** 31 and ds.n_nodes("m_big_totals") <= 16
    assert {lay[k]["node_bits"] for k in lay} >= {1, 4, 7}


def test_wide_gpu_milli_is_refused_above_128_nodes():
    assert he.prepare_device_workload(ds.wide_gpu_milli(128))["npass"] == 2
    with pytest.raises(he.UnsupportedWorkload):
        he.prepare_device_workload(ds.wide_gpu_milli(130))


@pytest.mark.parametrize("name", SMALL)
def test_oracle_equals_object_engine(name):
    """score, exception, snapshot and fragmentation counts of the C++ oracle ==
    the CPython object engine running `fam.to_program` of the same weights.
    The object engine needs seconds per replay, so each shape takes one family
    and one candidate, rotating over the catalogue."""
    w = ds.shape(name)
    cands = ds.candidates()
    k = SMALL.index(name)
    for family in ds.FAMILIES[k % 3:k % 3 + 1]:
        weights = cands[family][1][k % ds.N_CANDIDATES]
        ref = object_engine_eval(fam.to_program(family, weights), w)
        got = ce.simulate_builtin(w, family, list(weights))
        assert got["exc"] == ref.exc and got["score"] == ref.score, (family, got["score"], ref.score)
        assert ref.results is not None
        assert got["n_snapshots"] == ref.results.num_snapshots, family
        assert got["n_frag_events"] == ref.results.num_fragmentation_events, family


@pytest.mark.parametrize("name", [n for n in ds.SHAPES if n not in ds.DISTINCT_EXEMPT])
def test_candidates_are_told_apart_and_placements_fail(name):
    """At least half of each family's candidates have pairwise-distinct trace
    hashes and at least a quarter record fragmentation events."""
    w = ds.shape(name)
    for family in ds.FAMILIES:
        tab = ce.simulate_builtin_batch(w, family, ds.candidates()[family][1][:ds.N_CANDIDATES])
        assert not tab[:, 10].any(), family
        distinct, frag = len(set(tab[:, 12].tolist())), int((tab[:, 7] > 0).sum())
        assert 2 * distinct >= ds.N_CANDIDATES and 4 * frag >= ds.N_CANDIDATES, (family, distinct, frag)


@pytest.mark.parametrize("name", ("sweep129", "sweep255"))
def test_abort_batches_raise_three_exception_classes(name):
    """The "aborts" batches on the shapes the two-wave builtin kernel takes: the
    sampled row replays clean and scores, the other four raise, in at least
    three exception classes."""
    for batch in ds.ABORT_BATCHES:
        family, weights = ds.candidates()[batch]
        tab = ce.simulate_builtin_batch(ds.shape(name), family, weights)
        assert tab[0, 10] == 0 and tab[0, 0] > 0, (batch, tab[0].tolist())
        assert tab[1:, 10].all() and len(set(tab[1:, 10].tolist())) >= 3, (batch, tab[:, 10].tolist())
        assert not tab[1:, 0].any(), batch


@pytest.mark.parametrize("n", (13, 70))
def test_zero_request_pods_matter(n):
    a, b = ds.zero_requests(n), ds.zero_requests(n, with_zero_pods=False)
    assert a.pods.n_pods > b.pods.n_pods
    for family in ds.FAMILIES:
        weights = ds.candidates()[family][1][:ds.N_CANDIDATES]
        ta, tb = ce.simulate_builtin_batch(a, family, weights), ce.simulate_builtin_batch(b, family, weights)
        assert (ta[:, 0] != tb[:, 0]).all() and (ta[:, 1:6] != tb[:, 1:6]).any(axis=1).all(), family


def test_program_pick():
    codes = ds.program_groups()
    assert [len(codes[g]) for g in ("reference", "seed", "family")] == [5, 5, 9] and len(codes["corpus"]) == 16
    body = [c.split("return 0\n    ", 2)[-1] for c in codes["corpus"]]
    assert all("node.gpus" in b for b in body)
    assert sum("for " in b for b in body) >= 4 and sum("len(node.gpus)" in b for b in body) >= 4


@pytest.mark.parametrize("name", ds.PROGRAM_SHAPES)
def test_cpu_vm_scores_every_picked_program(name):
    """No picked program is deferred (UNSUPPORTED) or cut (BUDGET) by the CPU VM
    on a shape the device runs it on; the programs are told apart and a third
    of them meet failed placements."""
    tab = ds.program_oracle(name)
    assert not np.isin(tab[:, 10], (Exc.UNSUPPORTED, Exc.BUDGET)).any(), tab[:, 10]
    assert 3 * int((tab[:, 7] > 0).sum()) >= len(tab)
    if name not in ds.DISTINCT_EXEMPT:
        assert len(set(tab[:, 12].tolist())) * 2 >= len(tab)
