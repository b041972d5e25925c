"""The device's exact arithmetic on the catalogue of tests/exact_arith_cases.py:
LaneAcc, RowAcc (add, add_unit, the fragmentation stash), fixed_div_round_dev,
both score finalisers and div_by_recip, through the one-wave test kernels of
`_fks_hip` (csrc/hip/module.hip), which call the production code unchanged.
Everything is bit equality with the Python references (CPU preconditions of
the catalogue: tests/test_exact_arith_cases.py)."""
import numpy as np
import pytest

import exact_arith_cases as ea

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def hip():
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    if not he.device_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    return he.native()


def signed128(lo: int, hi: int) -> int:
    v = (hi << 64) | lo
    return v - (1 << 128) if v >> 127 else v


def agrees(got, ref) -> bool:
    """count always, flag always, sum whenever the flag is clear"""
    return got[1] == ref[1] and got[2] == ref[2] and (ref[2] or got[0] == ref[0])


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run_rows(hip, programs, inject=None, meta=None):
    """One launch: program s on row slot s.  Returns (raw lanes as Python ints
    [S][16] of (lo, hi, count, inexact), DevResult words, DevResult fields,
    write_row_result's table, k_eval_reduce's table)."""
    code = {name: i for i, name in enumerate(hip.TEST_ROW_OPS)}
    S = len(programs)
    ops = np.array([code[o] | (k << 8) for p in programs for o, k, _ in p], dtype=np.int32)
    vals = np.array([v for p in programs for _, _, v in p], dtype=np.float64)
    offs = np.cumsum([0] + [len(p) for p in programs]).astype(np.int32)
    inject = np.zeros(0, dtype=np.uint64) if inject is None else np.asarray(inject, dtype=np.uint64).reshape(S, 5, 4)
    meta = np.zeros((S, 5), dtype=np.int64) if meta is None else np.asarray(meta, dtype=np.int64).reshape(S, 5)
    raw, acc, fields, t_row, t_reduce = hip.test_row_acc(ops, vals, offs, inject, meta)
    assert raw.shape == (S, 16, 4) and t_row.shape == t_reduce.shape == (S, 13)
    lanes = [[tuple(int(x) for x in raw[s, j]) for j in range(16)] for s in range(S)]
    return lanes, acc, fields, t_row, t_reduce


def lane_state(lane):
    """(unsigned sum, count, flag) of a raw RowAcc lane"""
    lo, hi, count, inexact = lane
    return (hi << 64) | lo, count, bool(inexact & 1)


def arrangements(n):
    """Two orders of n sequences over the slots: each sequence meets other
    neighbours (and another accumulator index) the second time."""
    first = list(range(n))
    second = first[1::2] + first[0::2][::-1]
    return first, second


def test_lane_acc(hip):
    """LaneAcc::add: 144 sequences, each in two launches on different accumulators beside different neighbours."""
    names = list(ea.acc_cases())
    seqs = [ea.acc_cases()[k] for k in names]
    seen = {}
    for order in arrangements(len(seqs)):
        order = order + [None] * (-len(order) % 5)
        chosen = [() if i is None else seqs[i] for i in order]
        vals = np.array([v for s in chosen for v in s], dtype=np.float64)
        offs = np.cumsum([0] + [len(s) for s in chosen]).astype(np.int32)
        out = hip.test_lane_acc(vals, offs)
        assert out.shape == (len(chosen), 4)
        for slot, i in enumerate(order):
            lo, hi, count, inexact = (int(x) for x in out[slot])
            if i is None:
                assert (lo, hi, count, inexact) == (0, 0, 0, 0), slot
                continue
            got = (signed128(lo, hi), count, inexact != 0)
            assert inexact in (0, 1)
            assert agrees(got, ea.acc_reference(seqs[i], "lane")), (names[i], got)
            assert seen.setdefault(i, got) == got, names[i]          # whatever the neighbours
    print(f"LaneAcc::add: {len(seqs)} sequences x 2 arrangements, no disagreement")


@pytest.mark.parametrize("op,contract", [("add", "row_add"), ("add_unit", "unit")])
def test_row_acc_add(hip, op, contract):
    """RowAcc::add / add_unit: every sequence on a row of its own, four rows per
    wave, twice with other neighbours and another accumulator index."""
    names = list(ea.acc_cases())
    seqs = [ea.acc_cases()[k] for k in names]
    seen = {}
    for turn, order in enumerate(arrangements(len(seqs))):
        ks = [(slot + turn) % 5 for slot in range(len(order))]
        lanes, acc, fields, _, _ = run_rows(hip, [[(op, k, v) for v in seqs[i]] for i, k in zip(order, ks)])
        for slot, (i, k) in enumerate(zip(order, ks)):
            got = lane_state(lanes[slot][k])
            ref = ea.acc_reference(seqs[i], contract)
            assert agrees(got, ref), (names[i], got)
            assert seen.setdefault(i, got) == got, names[i]          # whatever the neighbours
            for j in range(16):                                      # and nothing else in the row moved
                assert j == k or lanes[slot][j] == (0, 0, 0, 0), (names[i], j)
            # the DevResult carries the words, the snapshot count and the flag
            assert (int(acc[slot, 0, k]), int(acc[slot, 1, k])) == lanes[slot][k][:2]
            assert fields[slot, 8] == ref[2] and fields[slot, 1] == (ref[1] if k == 0 else 0), names[i]
    print(f"RowAcc::{op}: {len(seqs)} sequences x 2 arrangements, no disagreement")


def test_row_stash_programs(hip):
    """stash_unit / add_stash / stash_drop against accumulator 4 with snapshots
    on accumulators 0-3 in between: the five accumulators hold what the
    program added to each, the same with other rows beside it, accumulators 0-3
    are what the program without its stash ops leaves, and the flag the row
    reports is that of lanes 0-4 alone."""
    names = list(ea.acc_cases())
    seqs = [ea.acc_cases()[k] for k in names]
    progs = [ea.stash_program(s, len(s)) for s in seqs]
    seen = {}
    for order in arrangements(len(seqs)):
        lanes, _, fields, _, _ = run_rows(hip, [progs[i][0] for i in order])
        for slot, i in enumerate(order):
            refs = [ea.acc_reference(progs[i][1][k], "unit") for k in range(5)]
            got = [lane_state(lanes[slot][k]) for k in range(5)]
            assert all(agrees(g, r) for g, r in zip(got, refs)), (names[i], got)
            assert seen.setdefault(i, got) == got, names[i]
            assert fields[slot, 8] == any(r[2] for r in refs), names[i]
            assert all(lanes[slot][k][3] in (0, 1, 2, 3) for k in range(16))
    plain, _, _, _, _ = run_rows(hip, [[o for o in p[0] if o[0] == "add_unit"] for p in progs])
    lanes, _, _, _, _ = run_rows(hip, [p[0] for p in progs])
    for i in range(len(seqs)):
        assert [x[:3] for x in lanes[i][:4]] == [x[:3] for x in plain[i][:4]], names[i]
        assert [x[3] & 1 for x in lanes[i][:4]] == [x[3] & 1 for x in plain[i][:4]], names[i]
    print(f"RowAcc stash programs: {len(seqs)} programs x 2 arrangements, no disagreement")


def test_row_stash_flag_stays_in_the_stash(hip):
    """A sample outside the band that is stashed and never added: lanes 5-15
    carry its flag in bit 0, accumulator 4 and the reported flag stay clear;
    bit 1 (stash valid) is set by stash_unit and cleared by stash_drop in
    every lane of the row."""
    stash = lambda v: ("stash_unit", 4, v)
    add, drop = ("add_stash", 4, 0.0), ("stash_drop", 4, 0.0)
    programs = [
        [stash(2.0)],
        [stash(float("nan")), drop],
        [stash(-0.0), drop, stash(0.5), add],
        [stash(2.0 ** -32), stash(0.0), add, add],
        [("add_unit", 0, 0.5), stash(3.0), ("add_unit", 1, 0.25), drop, stash(1.0), add, stash(2.0 ** -40)],
        [stash(2.0), add],                                     # and added: now it is reported
    ]
    lanes, _, fields, _, _ = run_rows(hip, programs)
    want4 = [(0, 0, False), (0, 0, False), (ea.F96 // 2, 1, False), (0, 2, False), (ea.F96, 1, False)]
    for s, w in enumerate(want4):
        assert lane_state(lanes[s][4]) == w and fields[s, 8] == 0, s
    assert lane_state(lanes[5][4])[1:] == (1, True) and fields[5, 8] == 1
    for s, (flag, valid) in enumerate([(1, 2), (1, 0), (0, 2), (0, 2), (1, 2), (1, 2)]):
        assert all(x[3] & 1 == flag for x in lanes[s][5:]), s
        assert all(x[3] & 2 == valid for x in lanes[s]), s
        assert len({x[:2] for x in lanes[s][5:]}) == 1, s      # one triple in every stash lane
    assert lane_state(lanes[4][0]) == (ea.F96 // 2, 1, False) and lane_state(lanes[4][1]) == (ea.F96 // 4, 1, False)


def test_fixed_div_round(hip):
    """fixed_div_round_dev on the 22,978 (A, n) of the catalogue, one pair per lane."""
    cases = ea.div_cases()
    a = [A & ((1 << 128) - 1) for _, A, _ in cases]
    lo = np.array([x & M64 for x in a], dtype=np.uint64)
    hi = np.array([x >> 64 for x in a], dtype=np.uint64)
    n = np.array([c[2] for c in cases], dtype=np.uint64)
    got = hip.test_fixed_div(lo, hi, n)
    ref = np.array(ea.div_references(), dtype=np.float64)
    bad = np.nonzero(bits(got) != bits(ref))[0]
    print(f"fixed_div_round_dev: {len(cases)} pairs, {len(bad)} disagreements")
    assert len(bad) == 0, [(cases[i], float(got[i]), float(ref[i])) for i in bad[:8]]


def finaliser_inputs(cases):
    inject = np.zeros((len(cases), 5, 4), dtype=np.uint64)
    meta = np.zeros((len(cases), 5), dtype=np.int64)
    for s, c in enumerate(cases):
        for k, (total, count, flag) in enumerate(c["states"]):
            inject[s, k] = (total & M64, total >> 64, count, int(flag))
        h = c["hash"] - (1 << 64) if c["hash"] >> 63 else c["hash"]          # the same 64 bits, as int64
        meta[s] = (c["n_events"], c["exc"], 77, c["n_unplaced"], h)
    return inject, meta


def test_finalisers(hip):
    """write_row_result on injected accumulator states, four rows per wave, and
    k_eval_reduce on the DevResults the same launch wrote: both tables equal the
    reference rows and each other."""
    names = list(ea.finaliser_cases())
    cases = [ea.finaliser_cases()[k] for k in names]
    inject, meta = finaliser_inputs(cases)
    lanes, acc, fields, t_row, t_reduce = run_rows(hip, [[] for _ in cases], inject, meta)
    ref = np.array([ea.finaliser_row(c) for c in cases], dtype=np.float64)
    for s, name in enumerate(names):
        assert bits(t_row[s]).tolist() == bits(ref[s]).tolist(), (name, t_row[s].tolist(), ref[s].tolist())
        assert bits(t_reduce[s]).tolist() == bits(ref[s]).tolist(), (name, t_reduce[s].tolist(), ref[s].tolist())
        c = cases[s]
        assert [lane_state(x) for x in lanes[s][:5]] == [(t, n, f) for t, n, f in c["states"]], name
        assert [(int(acc[s, 0, k]), int(acc[s, 1, k])) for k in range(5)] == [x[:2] for x in lanes[s][:5]], name
        assert fields[s].tolist() == [c["n_events"], c["states"][0][1], c["states"][4][1], c["n_unplaced"], 77, 0,
                                      int(meta[s, 4]), c["exc"], int(any(x[2] for x in c["states"]))], name
    assert np.array_equal(bits(t_row), bits(t_reduce))
    print(f"finalisers: {len(cases)} rows, no disagreement")


def test_finalisers_on_accumulated_states(hip):
    """The same through the accumulators: utilisation means above 1 by add (the
    score clamps to 1), thirds by add_unit and the stash, each beside other rows."""
    c = ea.finaliser_cases()["means above 1"]
    seqs = [[1.5, 1.25, 1.75], [1.0, 1.5, 1.0], [1.25] * 3, [1.0, 1.0, 1.75]]
    program = [("add", k, v) for k in range(4) for v in seqs[k]] + [("add_unit", 4, 0.0625)] * 4
    thirds = [("add_unit", k, 1 / 3) for k in range(4) for _ in range(3)] + \
             [("stash_unit", 4, 1 / 3)] + [("add_stash", 4, 0.0)] * 7
    cases = [c, ea.finaliser_cases()["thirds"], c, c]
    _, meta = finaliser_inputs(cases)
    _, _, _, t_row, t_reduce = run_rows(hip, [program, thirds, program, program], None, meta)
    ref = np.array([ea.finaliser_row(x) for x in cases], dtype=np.float64)
    assert np.array_equal(bits(t_row), bits(ref)) and np.array_equal(bits(t_reduce), bits(ref))
    assert t_row[0, 0] == 1.0 and t_row[0, 1:5].min() > 1.0


def test_div_by_recip(hip, default_workload):
    """div_by_recip(n, d, RN(1 / d)) on the device == on the host for every
    numerator the host verifies, == n / d wherever the host's verification
    passed, and it passes for every divisor of the default workload."""
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    cases = ea.divisor_cases(he.prepare_device_workload(default_workload))
    chunk, total, unverified = 1 << 22, 0, []
    for d, hi, from_workload in cases:
        zs = set()
        for start in range(0, hi + 1, chunk):
            count = min(chunk, hi + 1 - start)
            z, host, dev = hip.test_div_by_recip(d, hi, start, count)
            zs.add(z)
            assert host.shape == dev.shape == (count,)
            assert np.array_equal(bits(dev), bits(host)), (d, hi, start)
            if z != 0.0:
                quot = np.arange(start, start + count, dtype=np.float64) / float(d)
                assert np.array_equal(bits(host), bits(quot)), (d, hi, start)
            total += count
        assert len(zs) == 1 and zs <= {0.0, 1.0 / d}, (d, hi, zs)
        if 0.0 in zs:
            unverified.append((d, hi))
        assert not (from_workload and 0.0 in zs), (d, hi)
    print(f"div_by_recip: {len(cases)} divisors, {total} numerators, device == host on all; "
          f"not verified by the host (the kernels divide): {unverified}")
