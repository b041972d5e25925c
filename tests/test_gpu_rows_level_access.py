"""Row kernel vs the CPU oracle over every access path of its heap.

A pop of the row kernel (csrc/hip/replay_rows.hip.h, `RowHeapT::pop_reinsert`)
walks the heap four levels per round; against the number T of heap slots kept
in LDS each round reads and writes its slots with a plain LDS access, a plain
HBM access or the general one, and so does the first step of a failed
placement's scan for the first pending deletion.  The pops also rely on every
slot from the heap's length up holding ~0.  `level_access_shapes.TOPS` forces
T to 1, 15, 31, 127, 511 and 1,023 (and leaves it to the host once), which puts
every round once wholly in LDS, once wholly in HBM and once across T:
15 | 31 decides round 0 and the first scan step, 127 | 511 round 1, 511 | 1,023
round 2.  The large workload starts with 1,200 heap entries, so its pops reach
round 2, fails placements while the heap is above 1,023 entries and then
shrinks to nothing (`tests/test_rows_level_access_shapes.py` checks that on the
CPU); the small one is a shape of the scan-deletion tests whose heap stays
below 512 entries.  Every kernel variant replays both, with the default launch
(the last wave holds one policy and three empty rows) and with
`row_wave_share` 1e-6 (one wave's four rows chain nine or ten replays each);
every comparison is `np.array_equal` on whole 13-column tables, trace hash
included.  One case sends native programs through the two-wave kernels, which
share the heap structure.
"""
import numpy as np
import pytest

import level_access_shapes as la
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
TOPS = la.TOPS + (None,)   # None: the host's choice


def _device(wname, options):
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    if not he.device_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    return he.DeviceEvaluator(la.WORKLOADS[wname](), options={"trace_hash": True, "row_kernel": "on", **options})


_oracle = {}


def oracle(wname, bname):
    if (wname, bname) not in _oracle:
        w = la.WORKLOADS[wname]()
        family, weights = la.batches()[bname]
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


def forced_top(top, n_pods):
    """The heap top `row_heap_top` = top gives (engine_host row_layout): the
    largest 2^k - 1 <= top, and no level more than covers the whole heap."""
    entries = (n_pods + 2 + 63) & ~63
    t = 1
    while 2 * t + 1 <= top and t < entries:
        t = 2 * t + 1
    return t


@pytest.mark.parametrize("top", TOPS, ids=[f"top{t}" if t else "auto" for t in TOPS])
@pytest.mark.parametrize("layout", LAYOUTS, ids=[lay[0] for lay in LAYOUTS])
def test_row_kernel_matches_oracle_at_every_heap_top(layout, top):
    lid, bname, options = layout
    family, weights = la.batches()[bname]
    for wname in la.WORKLOADS:
        n_pods = la.WORKLOADS[wname]().pods.n_pods
        want = oracle(wname, bname)
        assert not want[:, 10].any() and (want[:, 7] > 0).all()
        if top is not None and wname == "large":
            assert forced_top(top, n_pods) == top   # the large heap is deeper than every forced top
        for launch in ({}, ONE_WAVE):
            dev = _device(wname, {**options, **({} if top is None else {"row_heap_top": top}), **launch})
            info = dev.info()
            assert info["row_kernel_ok"] and dev._eng.would_use_rows(la.P)
            if top is not None:
                assert info["row_heap_top"] == forced_top(top, n_pods)
            if "row_composite_waves" in options:
                assert info["row_composite_waves"] == options["row_composite_waves"]
                assert info["row_flat"] == options.get("row_flat", True)
            _same(dev.evaluate_builtin(family, weights), want, (wname, lid, top, sorted(launch)))


def test_two_wave_kernels_still_match_cpu_vm():
    """The two-wave kernels (replay_duo.hip.h) use the same heap structure with
    the deletion bitmap: four native programs on the large workload, one
    program per pair of waves, with the whole heap in LDS and with 127 slots."""
    progs = sd.programs()
    w = la.large()
    want = ce.simulate_program_batch(w, progs)
    assert not want[:, 10].any() and want[2, 9] == w.pods.n_pods and (want[[0, 1, 3], 7] > 0).all()
    dev = _device("large", {"native_rows": 1, "native_duo": True})
    _same(dev.evaluate_native(progs), want, "two-wave kernel, host's heap top")
    assert dev.info()["native_rows_last"] == 0   # 0: the two-wave kernel ran
    dev.set_options(native_duo_top=127)
    try:
        _same(dev.evaluate_native(progs), want, "two-wave kernel, 127 slots in LDS")
        assert dev.info()["native_duo_top_last"] == 127
    finally:
        dev.set_options(native_duo_top=-1)
