"""Row kernel vs the CPU oracle where it scans the heap for the first pending deletion.

A failed placement of the row kernel (csrc/hip/replay_rows.hip.h) anchors its
retry to the first DELETION of the heap in array order, found by reading the
keys 32 slots per step (`RowHeapT::scan_deletion`); the entry found also
supplies the retry's time, which the trace hash folds in, so a wrong anchor
shows in column 12 at once.  The workload of `scan_deletion_shapes` puts that
entry in slot 0, in either half of a lane's pair, on both sides of a 32-slot
step, in the last live slot, beyond slot 64 and slot 128, and nowhere; its
queue workloads put it in slot n - 1 of heaps of n = 32, 64 and 128 entries
(`tests/test_rows_scan_deletion_shapes.py` counts them on the CPU).  Every
kernel variant replays it with 1, 63 and 127 heap slots in LDS and with the
host's own choice, so the scan crosses from LDS into the HBM slice at every
place it can; every comparison is `np.array_equal` on whole 13-column tables.
Batches hold 37 policies: with the default launch the last wave holds one
policy and three empty rows, with `row_wave_share` 1e-6 one wave's four rows
chain nine or ten policies each.
"""
import numpy as np
import pytest

import scan_deletion_shapes as sd
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce

pytestmark = pytest.mark.gpu

ONE_WAVE = {"row_wave_share": 1e-6}
#: (id, batch, options)
LAYOUTS = (("composite-w5", "composite_linear", {"row_composite_waves": 5}),
           ("composite-w4", "composite_linear", {"row_composite_waves": 4}),
           ("composite-split", "composite_linear", {"row_composite_waves": 4, "row_flat": False}),
           ("random-linear", "random_linear", {}),
           ("mixed", "mixed", {}))
TOPS = (1, 63, 127, None)   # None: the host's choice


def _device(wname, options):
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    if not he.device_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    return he.DeviceEvaluator(sd.WORKLOADS[wname](), options={"trace_hash": True, "row_kernel": "on", **options})


_oracle = {}


def oracle(wname, bname):
    if (wname, bname) not in _oracle:
        w = sd.WORKLOADS[wname]()
        family, weights = sd.batches()[bname]
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


def _top_options(top):
    return {} if top is None else {"row_heap_top": top}


@pytest.mark.parametrize("top", TOPS, ids=[f"top{t}" if t else "auto" for t in TOPS])
@pytest.mark.parametrize("layout", LAYOUTS, ids=[lay[0] for lay in LAYOUTS])
def test_row_kernel_matches_oracle_wherever_the_first_deletion_lies(layout, top):
    lid, bname, options = layout
    family, weights = sd.batches()[bname]
    for wname in sd.WORKLOADS:
        want = oracle(wname, bname)
        assert not want[:, 10].any()
        if wname == "b_hogs":   # every replay fails placements all along and drops the four pods that fit nowhere
            assert (want[:, 7] >= 10000).all() and (want[:, 9] == 4).all()
        else:
            assert (want[:, 8] >= 2000).all() and not want[:, 9].any()
        for launch in ({}, ONE_WAVE):
            dev = _device(wname, {**options, **_top_options(top), **launch})
            info = dev.info()
            assert info["row_kernel_ok"] and dev._eng.would_use_rows(sd.P)
            if top is not None:
                assert info["row_heap_top"] == top
            if "row_composite_waves" in options:
                assert info["row_composite_waves"] == options["row_composite_waves"]
                assert info["row_flat"] == options.get("row_flat", True)
            _same(dev.evaluate_builtin(family, weights), want, (wname, lid, top, sorted(launch)))


@pytest.mark.parametrize("top", TOPS, ids=[f"top{t}" if t else "auto" for t in TOPS])
def test_native_program_rows_match_cpu_vm(top):
    """Four programs through the native-program row kernel, four per wave: two
    of the corpus, one that places nothing (every failure scans the whole heap
    and finds no deletion, at every heap length down to 0) and one that turns
    most feasible nodes away; once as one batch of four and once as ten replays
    chained on one wave's rows."""
    progs = sd.programs()
    want = ce.simulate_program_batch(sd.workload(), progs)
    assert not want[:, 10].any() and want[2, 9] == sd.workload().pods.n_pods and want[3, 7] >= 1000
    dev = _device("b_hogs", {"native_rows": 4, **_top_options(top), **ONE_WAVE})
    _same(dev.evaluate_native(progs), want, ("native rows, four programs", top))
    info = dev.info()
    assert info["native_rows_last"] == 4
    if top is not None:
        assert info["native_rows_top_last"] == top
    pick = [i % 4 for i in range(10)]
    _same(dev.evaluate_native([progs[i] for i in pick]), want[pick], ("native rows, ten replays on one wave", top))
    assert dev.info()["native_rows_last"] == 4
