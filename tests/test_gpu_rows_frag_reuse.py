"""Row kernel vs the CPU oracle where it reuses a row's stashed fragmentation sample.

A failed placement of the row kernel (csrc/hip/replay_rows.hip.h) adds the
row's last fragmentation sample again unless a deletion, a placement, the
first failure of a GPU pod or the start of a policy came in between.  The
workloads of `frag_reuse_shapes` fail tens of thousands of placements with
every such order between them (`tests/test_rows_frag_reuse_shapes.py` counts
them on the CPU); every comparison here is `np.array_equal` on whole
13-column tables, trace hash included.  Batches hold 37 policies: with the
default launch the last wave holds one policy and three empty rows, with
`row_wave_share` 1e-6 one wave's four rows chain nine or ten policies each.
"""
import numpy as np
import pytest

import device_shapes as ds
import frag_reuse_shapes as fr
from funsearch_kubernetes_simulator_amd.core.arrays import Workload
from funsearch_kubernetes_simulator_amd.models import families as fam
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce

pytestmark = pytest.mark.gpu

P = fr.P_SWITCH
ONE_WAVE = {"row_wave_share": 1e-6}
WORKLOADS = {"a": fr.workload_a, "b": fr.workload_b}
#: (id, batch, options)
LAYOUTS = (("composite-w5", "composite_linear", {"row_composite_waves": 5}),
           ("composite-w5-one-wave", "composite_linear", {"row_composite_waves": 5, **ONE_WAVE}),
           ("composite-w4-one-wave", "composite_linear", {"row_composite_waves": 4, **ONE_WAVE}),
           ("composite-split-one-wave", "composite_linear", {"row_composite_waves": 4, "row_flat": False, **ONE_WAVE}),
           ("random-linear-one-wave", "random_linear", ONE_WAVE),
           ("mixed-one-wave", "mixed", ONE_WAVE))


def _device(workload, options):
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    if not he.device_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    return he.DeviceEvaluator(workload, options={"trace_hash": True, "row_kernel": "on", **options})


_batches = {}


def batch(name):
    """(family or families, weights [37, 16]) of a batch, built once."""
    if name not in _batches:
        rng = np.random.default_rng(4)
        comp = np.concatenate([fr.composite_candidates(),
                               fam.pad_weights(fam.sample_composite_linear(P - fr.N_CANDIDATES, rng))])
        rand = fam.pad_weights(fam.sample_random_linear(P, rng))
        feat = fam.pad_weights(fam.sample_feature_linear(P, rng))
        order = ("first_fit", "composite_linear", "best_fit", "feature_linear", "random_linear")
        names = [order[i % 5] for i in range(P)]
        mixed = np.zeros((P, 16))
        for i, f in enumerate(names):
            mixed[i] = {"composite_linear": comp, "random_linear": rand, "feature_linear": feat}.get(f, mixed)[i]
        _batches.update({"composite_linear": ("composite_linear", comp), "random_linear": ("random_linear", rand),
                         "mixed": (names, mixed)})
        for _, w in _batches.values():
            w.setflags(write=False)
    return _batches[name]


_oracle = {}


def oracle(wname, bname):
    if (wname, bname) not in _oracle:
        w = WORKLOADS[wname]()
        family, weights = batch(bname)
        if isinstance(family, str):
            tab = ce.simulate_builtin_batch(w, family, weights)
        else:
            tab = np.zeros((len(family), 13))
            for f in sorted(set(family)):
                idx = [i for i, g in enumerate(family) if g == f]
                tab[idx] = ce.simulate_builtin_batch(w, f, weights[idx])
        tab.setflags(write=False)
        _oracle[(wname, bname)] = tab
    return _oracle[(wname, bname)]


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8].tolist())


@pytest.mark.parametrize("wname", list(WORKLOADS))
@pytest.mark.parametrize("layout", LAYOUTS, ids=[lay[0] for lay in LAYOUTS])
def test_row_kernel_matches_oracle_where_failures_repeat(wname, layout):
    lid, bname, options = layout
    dev = _device(WORKLOADS[wname](), options)
    info = dev.info()
    assert info["row_kernel_ok"] and dev._eng.would_use_rows(P)
    if "row_composite_waves" in options:
        assert info["row_composite_waves"] == options["row_composite_waves"]
        assert info["row_flat"] == options.get("row_flat", True)
    family, weights = batch(bname)
    want = oracle(wname, bname)
    assert not want[:, 10].any() and (want[:, 7] >= 10000).all()   # every row fails placements all along
    _same(dev.evaluate_builtin(family, weights), want, (wname, lid))


def test_stash_does_not_survive_a_policy_switch():
    """Workload A with a CPU-only pod at time 0 that fits no node: every replay
    opens with a first failure that changes no waiting class, so the reuse rule
    alone would take over what the row's previous policy left, where the right
    sample is 0.  Every other candidate aborts mid-replay on a weight of 1e308,
    several of them right after a failed placement with a sample above 0
    (counted in tests/test_rows_frag_reuse_shapes.py), and the four rows of
    one wave chain all 37."""
    w = fr.workload_a_cpu_hog()
    weights, marked = fr.switch_batch()
    want = ce.simulate_builtin_batch(w, "composite_linear", weights)
    assert (want[marked, 10] != 0).all() and not want[~marked, 10].any()
    assert (want[~marked, 7] >= 1).all()
    for waves in (5, 4):
        dev = _device(w, {"row_composite_waves": waves, **ONE_WAVE})
        assert dev._eng.would_use_rows(P)
        _same(dev.evaluate_builtin("composite_linear", weights), want, ("policy switch", waves))


def test_native_program_rows_match_cpu_vm():
    """Four corpus programs through the native-program row kernel, four per
    wave: once as one batch of four and once as ten replays chained on one
    wave's rows.  A program fails a placement whenever its best score is <= 0,
    feasible nodes included."""
    groups, progs = ds.programs()
    corpus = [p for g, p in zip(groups, progs) if g == "corpus"][:4]
    b = fr.workload_b()
    w = Workload(b.cluster, b.pods.subset(np.arange(min(ds.PROGRAM_PODS, b.pods.n_pods))), "frag_reuse_b_programs")
    want = ce.simulate_program_batch(w, corpus)
    assert not want[:, 10].any() and (want[:, 7] >= 10000).all()
    dev = _device(w, {"native_rows": 4, **ONE_WAVE})
    _same(dev.evaluate_native(corpus), want, "native rows, four programs")
    assert dev.info()["native_rows_last"] == 4
    pick = [i % 4 for i in range(10)]
    _same(dev.evaluate_native([corpus[i] for i in pick]), want[pick], "native rows, ten replays on one wave")
    assert dev.info()["native_rows_last"] == 4
