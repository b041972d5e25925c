"""CPU side of the exact-arithmetic catalogue (tests/exact_arith_cases.py).

* Preconditions: enough sequences are in contract for "flag or exact" to mean
  something, every kind of division case and every normalising branch is
  there, the finaliser scenarios are what their names say.
* The host twin (csrc/include/fks/exact_mean.hpp, through `exact_acc` and
  `fixed_div_round` of `_fks_cpu`) equals the references.
* A Python transliteration of the device routines (LaneAcc, RowAcc with its
  fragmentation stash, fixed_div_round_dev) equals the references on the whole
  catalogue, and each seeded mutant of it -- the slips such code invites --
  disagrees on at least one case: the catalogue tells them apart without a GPU.
"""
import math
import struct

import pytest

import exact_arith_cases as ea
from funsearch_kubernetes_simulator_amd.ops import cpu_engine as ce

M64 = (1 << 64) - 1


def signed128(lo: int, hi: int) -> int:
    v = (hi << 64) | lo
    return v - (1 << 128) if v >> 127 else v


def dbits(v: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", v))[0]


# ---- the device routines, transliterated -------------------------------------------------
# `mut`: the seeded slips
MUTANTS = ("ties_up", "no_sticky", "no_carry", "band_45", "no_headroom", "sign_ignored", "small_truncates")


def model_fixed_div(A: int, n: int, mut=()) -> float:
    """fixed_div_round_dev (device_common.h); divmod stands for the restoring division."""
    if A == 0 or n == 0:
        return 0.0
    neg, a = A < 0, abs(A)
    q, r = divmod(a, n)
    exp2, small = -96, False
    if q >> 64:
        extra = 0
        while q >> (64 + extra):
            extra += 1
        sticky = (q & ((1 << extra) - 1)) != 0 or r != 0
        q >>= extra
        exp2 += extra
    else:
        small = not (q >> 63)
        while not (q >> 63):
            r <<= 1
            bit = 1 if r >= n else 0
            if bit:
                r -= n
            q = (q << 1) | bit
            exp2 -= 1
        sticky = r != 0
    if "no_sticky" in mut:
        sticky = False
    low, m53 = q & 0x7FF, q >> 11
    exp2 += 11
    up = low > 0x400 or (low == 0x400 and (sticky or (m53 & 1) or "ties_up" in mut))
    if small and "small_truncates" in mut:
        up = False
    if up:
        m53 += 1
        if m53 >> 53:
            m53 >>= 1
            exp2 += 1
    v = math.ldexp(float(m53), exp2)
    return -v if neg else v


def model_lane_acc(seq, mut=()):
    """LaneAcc::add on one accumulator: (sum, count, inexact)."""
    total, count, inexact = 0, 0, False
    for v in seq:
        bits = dbits(v)
        E, frac = (bits >> 52) & 0x7FF, bits & ((1 << 52) - 1)
        count += 1
        if E == 0 and frac == 0:
            continue
        bad = E == 0x7FF or E == 0
        M, shift = frac | (1 << 52), E - 979
        if not bad and shift < 0:
            if shift <= -53 or (M & ((1 << -shift) - 1)):
                bad = True
            else:
                M >>= -shift
                shift = 0
        if not bad and shift > 126 - 53:
            bad = True
        if bad:
            inexact = True
            continue
        t = M << shift
        total += -t if bits >> 63 else t
        if abs(total) >> 126 and "no_headroom" not in mut:
            inexact = True
    return total, count, inexact


class RowAccModel:
    """RowAcc (replay_rows.hip.h) on the 16 lanes of one row: lane = [lo, hi, count, inexact]."""
    STASH_VALID = 2

    def __init__(self, mut=()):
        self.lane = [[0, 0, 0, 0] for _ in range(16)]
        self.mut = mut

    def _accumulate(self, a, tl, th):
        a[0] = (a[0] + tl) & M64
        carry = 0 if "no_carry" in self.mut else int(a[0] < tl)
        a[1] = (a[1] + th + carry) & M64

    def add(self, k, v):
        a, bits = self.lane[k], dbits(v)
        a[2] += 1
        if bits == 0:
            return
        E = bits >> 52
        if "sign_ignored" in self.mut:
            E &= 0x7FF
        M, shift = (bits & ((1 << 52) - 1)) | (1 << 52), E - 979
        bad = E == 0 or E >= 0x7FF or shift > 126 - 53
        if shift >= 0:
            tl = (M << shift) & M64 if shift < 64 else 0
            th = 0 if shift == 0 else (M >> (64 - shift) if shift < 64 else (M << (shift - 64)) & M64)
        else:
            bad = bad or shift <= -53 or (M & ((1 << -shift) - 1)) != 0
            tl, th = M >> (-shift & 63), 0
        if bad:
            a[3] |= 1
            return
        self._accumulate(a, tl, th)
        if a[1] >> 62 and "no_headroom" not in self.mut:
            a[3] |= 1

    def _unit(self, v):
        bits = dbits(v)
        s = (bits >> 52) - 979
        M = (bits & ((1 << 52) - 1)) | (1 << 52)
        top = 45 if "band_45" in self.mut else 44
        return bits, (M << (s & 63)) & M64, M >> ((64 - s) & 63), s < 13 or s > top

    def add_unit(self, k, v):
        a = self.lane[k]
        bits, tl, th, out = self._unit(v)
        a[2] += 1
        if bits == 0:
            return
        if out:
            a[3] |= 1
        self._accumulate(a, tl, th)

    def stash_unit(self, v):
        bits, tl, th, out = self._unit(v)
        for j in range(16):
            a = self.lane[j]
            if j >= 5:
                a[0], a[1], a[3] = (0, 0, 0) if bits == 0 else (tl, th, int(out))
            a[3] |= self.STASH_VALID

    def stash_drop(self):
        for a in self.lane:
            a[3] &= ~self.STASH_VALID

    def add_stash(self):
        src, a = self.lane[12], self.lane[4]   # row_ror 8: lane 4 reads lane 12
        tl, th, bad = src[0], src[1], src[3] & 1
        a[2] += 1
        a[3] |= bad
        self._accumulate(a, tl, th)

    def run(self, ops):
        for op, k, v in ops:
            if op == "add":
                self.add(k, v)
            elif op == "add_unit":
                self.add_unit(k, v)
            elif op == "stash_unit":
                self.stash_unit(v)
            elif op == "add_stash":
                self.add_stash()
            else:
                self.stash_drop()
        return self

    def state(self, k):
        a = self.lane[k]
        return (a[1] << 64) | a[0], a[2], bool(a[3] & 1)


def agrees(got, ref) -> bool:
    """The accumulator rule: count always, flag always, sum whenever the flag is clear."""
    return got[1] == ref[1] and got[2] == ref[2] and (ref[2] or got[0] == ref[0])


def model_disagreements(mut=()) -> int:
    """Cases of the catalogue on which the (mutated) model differs from the references."""
    bad = 0
    for seq in ea.acc_cases().values():
        bad += not agrees(model_lane_acc(seq, mut), ea.acc_reference(seq, "lane"))
        for op, contract in (("add", "row_add"), ("add_unit", "unit")):
            row = RowAccModel(mut).run([(op, 2, v) for v in seq])
            bad += not agrees(row.state(2), ea.acc_reference(seq, contract))
        ops, held = ea.stash_program(seq, len(seq))
        row = RowAccModel(mut).run(ops)
        bad += not all(agrees(row.state(k), ea.acc_reference(held[k], "unit")) for k in range(5))
    for (_, A, n), ref in zip(ea.div_cases(), ea.div_references()):
        bad += dbits(model_fixed_div(A, n, mut)) != dbits(ref)
    return bad


def test_model_equals_references():
    assert model_disagreements() == 0


@pytest.mark.parametrize("mut", MUTANTS)
def test_catalogue_catches_mutant(mut):
    assert model_disagreements((mut,)) > 0


def test_stash_flag_does_not_leak_in_the_model():
    """A flagged sample that is stashed and never added leaves accumulator 4 clean."""
    row = RowAccModel().run([("stash_unit", 4, 2.0), ("stash_drop", 4, 0.0), ("stash_unit", 4, 0.5), ("add_stash", 4, 0.0)])
    assert row.state(4) == (ea.F96 // 2, 1, False)
    row = RowAccModel().run([("stash_unit", 4, 2.0)])
    assert row.lane[12][3] & 1 and row.state(4) == (0, 0, False)


# ---- preconditions ---------------------------------------------------------------------

@pytest.mark.parametrize("contract", ea.CONTRACTS)
def test_half_of_the_sequences_are_in_contract(contract):
    share = ea.in_contract_share(contract)
    assert 0.5 <= share < 1.0, share   # and some are flagged


def test_sequences_cover_what_they_claim():
    cases = ea.acc_cases()
    assert {len(s) for s in cases.values()} >= {0, 1, 2, 3, 255, 256}
    assert all(len(s) <= 256 for s in cases.values())
    # carries from the low to the high word happen in the in-contract ratio sequences
    carries = 0
    for name, seq in cases.items():
        if name.startswith("ratios"):
            lo = 0
            for v in seq:
                t = int(ea.Fraction(v) * ea.F96) & M64
                carries += (lo + t) > M64
                lo = (lo + t) & M64
    assert carries > 1000, carries
    ref = {k: {c: ea.acc_reference(s, c)[2] for c in ea.CONTRACTS} for k, s in cases.items()}
    clear = {"lane": False, "row_add": False, "unit": False}
    assert ref["edge[2^-31]"] == clear and ref["edge[1]"] == clear and ref["edge[below 2]"] == clear
    assert ref["edge[below 2^-31]"] == {"lane": False, "row_add": False, "unit": True} == ref["edge[2]"]
    assert ref["edge[2^-96]"] == ref["edge[3*2^-96]"] == ref["edge[(2^53-1)*2^-96]"] == ref["edge[below 2^30]"] \
        == {"lane": False, "row_add": False, "unit": True}
    for k in ("2^-97", "(2^53-1)*2^-97", "2^30", "5e-324", "2^-1022", "inf", "nan"):
        assert all(ref[f"edge[{k}]"].values()), k
    assert ref["edge[-1]"] == ref["edge[-2^-96]"] == {"lane": False, "row_add": True, "unit": True}
    assert ref["edge[-0.0]"] == {"lane": False, "row_add": True, "unit": True} and ref["edge[+0.0]"] == clear
    assert ref["2^29 twice"]["lane"] and ref["2^29 twice"]["row_add"] and not ref["2^29 + below 2^29"]["lane"]
    assert ref["2^29 twice and back"]["lane"]
    assert ea.acc_reference(cases["cancel to negative"], "lane") == (-(ea.F96 // 4), 2, False)
    assert ea.acc_reference(cases["cancel to zero"], "lane") == (0, 4, False)
    assert ea.acc_reference(cases["cancel to -2^-96"], "lane") == (-1, 3, False)


def test_division_cases_cover_every_kind_and_branch():
    cases = ea.div_cases()
    assert 15000 <= len(cases) <= 30000, len(cases)
    labels = [c[0] for c in cases]
    for want in ("tie_even", "tie_odd", "tie_even_neg", "tie_odd_neg", "tie_off", "tie_off_neg", "carry", "carry_neg",
                 "q63", "q64", "q65", "below_one", "n_list", "random"):
        assert labels.count(want) > 0, want
    assert labels.count("random") >= 3000
    assert all(0 < abs(A) < 2 ** 126 and 1 <= n < 2 ** 63 for _, A, n in cases)
    branches = [ea.div_branch(A, n) for _, A, n in cases]
    for want in ("shift_right", "exact_64", "shift_left", "zero"):
        assert branches.count(want) > 50, want
    assert {n for _, _, n in cases} >= set(ea.DIV_N)
    # ties sit on both sides of the 64-bit quotient split, even and odd
    for label in ("tie_even", "tie_odd"):
        sides = {ea.div_branch(A, n) for lab, A, n in cases if lab == label}
        assert sides >= {"shift_right", "exact_64", "shift_left"}, (label, sides)
    # a tie is a tie: 54 significant quotient bits, the last one set, no remainder
    for lab, A, n in cases:
        if lab in ("tie_even", "tie_odd", "carry"):
            q, r = divmod(A, n)
            assert r == 0 and (q >> ((q & -q).bit_length() - 1)).bit_length() == 54, (A, n)
    assert (1, 2 ** 40) in {(A, n) for _, A, n in cases}


def test_finaliser_cases_are_what_their_names_say():
    cases = ea.finaliser_cases()
    rows = {k: ea.finaliser_row(c) for k, c in cases.items()}
    for c in cases.values():
        assert len({s[1] for s in c["states"][:4]}) == 1          # one snapshot count
        assert all(0 <= s[0] < 2 ** 126 and 0 <= s[1] < 2 ** 31 for s in c["states"])
    assert rows["plain"][0] > 0 and rows["plain"][11] == 0
    assert rows["no snapshots"][0] == 0 and rows["no snapshots"][6] == 0 and rows["no snapshots"][5] > 0
    assert rows["unplaced pods"][0] == 0 and min(rows["unplaced pods"][1:6]) > 0   # means kept
    assert rows["unplaced pods"][9] == 3
    assert rows["exception"] == [0.0] * 10 + [6.0, 0.0, 0.0]
    assert rows["frag below 0.1"][5] < 0.1 == rows["frag at 0.1"][5] < rows["frag above 0.1"][5]
    for k in ("frag at 0.1", "frag above 0.1", "frag 0.25"):       # the penalty is capped
        r = rows[k]
        assert r[0] == (r[1] + r[2] + r[3] + r[4]) / 4.0 - 0.1 > 0
    r = rows["frag below 0.1"]
    assert r[0] == (r[1] + r[2] + r[3] + r[4]) / 4.0 - r[5] > 0
    r = rows["clamped to 0"]
    assert r[0] == 0.0 and (r[1] + r[2] + r[3] + r[4]) / 4.0 - 0.1 < 0
    r = rows["means above 1"]
    assert r[0] == 1.0 and min(r[1:5]) > 1.0
    assert rows["flagged utilisation"][11] == 1 and rows["flagged fragmentation"][11] == 1
    assert rows["hash with the top bits set"][12] == float(0xFEDCBA9876543210 >> 11) >= 2.0 ** 52
    assert 0 < min(rows["mean below 2^-32"][1:6]) and max(rows["mean below 2^-32"][1], rows["mean below 2^-32"][5]) < 2.0 ** -32


def test_finaliser_reference_uses_the_evaluators_formula():
    from funsearch_kubernetes_simulator_amd.simulator.metrics import EvaluationResults, combine_policy_score
    for name, c in ea.finaliser_cases().items():
        if c["exc"] or c["states"][0][1] == 0:
            continue
        r = ea.finaliser_row(c)
        res = EvaluationResults(r[1], r[2], r[3], r[4], r[5], int(r[6]), int(r[7]))
        assert r[0] == combine_policy_score(res, c["n_unplaced"] == 0), name


def test_divisor_cases_hold_the_default_workloads_reciprocals(default_workload):
    from funsearch_kubernetes_simulator_amd.ops import hip_engine as he
    lay = he.prepare_device_workload(default_workload)
    cases = ea.divisor_cases(lay)
    assert len(cases) == len(set(cases))
    assert all(d >= 1 and 0 <= hi < 2 ** 31 for d, hi, _ in cases)
    ds = {d for d, _, wl in cases if wl}
    c = default_workload.cluster
    assert ds >= {max(int(t), 1) for t in c.node_cpu_total} | {max(int(t), 1) for t in c.node_mem_total}
    assert ds >= {max(int(g), 1) for g in c.node_ngpus} | {1000, int(lay["tot_gmilli"])}
    assert {(2 ** 24 - 3, 2 ** 24 - 3, False), (3, 8, False), (7, 8, False), (1000, 2 ** 21 - 1, True)} <= set(cases)
    assert sum(hi + 1 for _, hi, _ in cases) < 2 ** 26   # numerators in all: seconds on the host


# ---- the host twin ---------------------------------------------------------------------

def test_host_accumulator_equals_reference():
    m = ce.native()
    for name, seq in ea.acc_cases().items():
        lo, hi, count, inexact = m.exact_acc(list(seq))
        assert agrees((signed128(lo, hi), count, bool(inexact)), ea.acc_reference(seq, "lane")), name


def test_host_division_equals_reference():
    m = ce.native()
    for (label, A, n), ref in zip(ea.div_cases(), ea.div_references()):
        a = A & ((1 << 128) - 1)
        got = m.fixed_div_round(a & M64, a >> 64, n)
        assert dbits(got) == dbits(ref), (label, A, n, got, ref)
