"""Coverage accumulator (include/monica_amd.h, "coverage"): what needs no GPU -- the reference model tests/covref.py on
hand-made cases with known answers, the selection rule of MNC_COV_ASSIGNED, the binding's constants against the header,
and the argument / device errors of the C-ABI."""
import ctypes as C
import os
import re

import numpy as np

import covref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "monica_amd.h")


def rec(rid, rs, cigar, selected=True):
    re_ = rs + sum(l for l, op in cigar if op != "I")
    return (rid, rs, re_, cigar, selected)


def reg(id_, parent, mapq, nm, mlen):
    return dict(id=id_, parent=parent, mapq=mapq, blen=mlen + nm, mlen=mlen, n_ambi=0)


# ---------------------------------------------------------------- covref on known answers
def test_deletion_is_not_covered():
    r = rec(0, 3, [(10, "M"), (2, "D"), (5, "M")])
    assert r[2] == 20
    assert covref.covered_runs(3, r[3]) == [(3, 13), (15, 20)]
    d = covref.depth([r], [25])[0]
    assert d.tolist() == [0] * 3 + [1] * 10 + [0] * 2 + [1] * 5 + [0] * 5
    s = covref.summary([r], [d])
    assert (int(s[0]["covered"]), int(s[0]["depth_sum"]), int(s[0]["max_depth"]), int(s[0]["n_aln"])) == (15, 15, 1, 1)
    # SPAN covers the deleted bases as well
    assert covref.depth([r], [25], span=True)[0].tolist() == [0] * 3 + [1] * 17 + [0] * 5


def test_insertion_does_not_break_a_run():
    cig = [(5, "M"), (3, "I"), (5, "M")]
    assert covref.covered_runs(7, cig) == [(7, 17)]                 # one run
    assert covref.covered_runs(0, [(4, "M"), (2, "M"), (1, "I"), (3, "M"), (1, "D"), (2, "M")]) == [(0, 9), (10, 12)]
    r = rec(0, 7, cig)
    assert r[2] == 17
    assert covref.depth([r], [20])[0].tolist() == [0] * 7 + [1] * 10 + [0] * 3


def test_a_record_ending_on_the_last_base_leaves_the_next_contig_alone():
    recs = [rec(0, 4, [(6, "M")]), rec(1, 0, [(3, "M")]), rec(1, 0, [(2, "M")])]
    assert recs[0][2] == 10
    d = covref.depth(recs, [10, 5])
    assert d[0].tolist() == [0] * 4 + [1] * 6
    assert d[1].tolist() == [2, 2, 1, 0, 0]                         # base 0 of contig 1: two, not one
    s = covref.summary(recs, d)
    assert s["n_aln"].tolist() == [1, 2] and s["covered"].tolist() == [6, 3] and s["max_depth"].tolist() == [1, 2]


def test_overlapping_records_and_unselected_ones():
    recs = [rec(0, 0, [(8, "M")]), rec(0, 4, [(8, "M")]), rec(0, 6, [(2, "M")]), rec(0, 0, [(12, "M")], selected=False)]
    d = covref.depth(recs, [12])[0]
    assert d.tolist() == [1, 1, 1, 1, 2, 2, 3, 3, 1, 1, 1, 1]
    s = covref.summary(recs, [d])[0]
    assert (int(s["covered"]), int(s["depth_sum"]), int(s["max_depth"]), int(s["n_aln"])) == (12, 18, 3, 3)


def test_bins_with_a_short_last_bin():
    d = np.array([0, 1, 2, 0, 0, 0, 3, 1, 1, 0, 5], dtype=np.int64)
    cov, dsum = covref.bins(d, 4)
    assert cov.tolist() == [2, 2, 2] and dsum.tolist() == [3, 4, 6] and cov.dtype == np.int32 and dsum.dtype == np.int64
    cov, dsum = covref.bins(d, 1)
    assert cov.tolist() == (d > 0).astype(int).tolist() and dsum.tolist() == d.tolist()
    cov, dsum = covref.bins(d, 11)
    assert cov.tolist() == [6] and dsum.tolist() == [13]
    assert [len(x) for x in covref.bins(d, 100)] == [1, 1]


# ---------------------------------------------------------------- the selectors
def test_assigned_takes_the_record_best_hit_chose():
    # a tie EARLIER in the list, then a strictly smaller ratio: the decision is a contig, the choice the last record
    regs = [reg(0, 0, 60, 10, 100), reg(1, 1, 60, 20, 200), reg(2, 2, 60, 5, 100)]
    assert covref.best_hit([(10, 100), (20, 200), (5, 100)]) == 2
    assert covref.select(regs, covref.ASSIGNED, 60) == [False, False, True]
    # the minimum first, worse ones behind it
    assert covref.select([reg(0, 0, 60, 1, 100), reg(1, 1, 60, 2, 100), reg(2, 2, 60, 2, 100)], covref.ASSIGNED, 60) == [True, False, False]
    # the last update a tie: ambiguous, nothing is added
    assert covref.best_hit([(5, 100), (10, 200)]) is None
    assert covref.select([reg(0, 0, 60, 5, 100), reg(1, 1, 60, 10, 200)], covref.ASSIGNED, 60) == [False, False]
    # secondaries and ungated primaries are no candidates; one gated record is the choice whatever its ratio
    regs = [reg(0, 0, 12, 1, 100), reg(1, 0, 0, 0, 100), reg(2, 2, 60, 30, 100)]
    assert covref.select(regs, covref.ASSIGNED, 60) == [False, False, True]
    assert covref.select(regs, covref.ASSIGNED | covref.SPAN, 60) == [False, False, True]
    assert covref.select(regs, covref.GATED, 60) == [False, False, True]
    assert covref.select(regs, covref.PRIMARY, 60) == [True, False, True]
    assert covref.select(regs, covref.ALL, 60) == [True, True, True]
    assert covref.select(regs, covref.GATED, 0) == [True, False, True]
    assert covref.select([], covref.ASSIGNED, 60) == []
    assert covref.select(regs, covref.ASSIGNED, 60, skipped=True) == [False] * 3


def test_assigned_agrees_with_the_library_best_hit(capi):
    rng = np.random.default_rng(5)
    for _ in range(300):
        hits = [(int(rng.integers(0, 6)), int(rng.integers(1, 4)) * 50) for _ in range(int(rng.integers(1, 6)))]
        want = capi.best_hit(hits)
        got = covref.best_hit(hits)
        assert (got if got is not None else -1) == want, hits


# ---------------------------------------------------------------- binding against the header
def test_constants_and_dtypes_match_the_header(capi):
    text = open(HEADER).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+MNC_COV_(\w+)\s+(\d+)", text)}
    assert defs == dict(GATED=capi.COV_GATED, PRIMARY=capi.COV_PRIMARY, ALL=capi.COV_ALL, ASSIGNED=capi.COV_ASSIGNED, SPAN=capi.COV_SPAN)
    assert defs == dict(GATED=covref.GATED, PRIMARY=covref.PRIMARY, ALL=covref.ALL, ASSIGNED=covref.ASSIGNED, SPAN=covref.SPAN)
    assert sorted(defs.values()) == [1, 2, 4, 8, 16]
    # mnc_coverage_summary(cov, int64 covered, int64 depth_sum, int32 max_depth, int64 n_aln): the rows of Coverage.summary()
    m = re.search(r"int\s+mnc_coverage_summary\(([^)]*)\)", text)
    args = [a.strip() for a in m.group(1).split(",")][1:]
    assert [a.split("*")[1] for a in args] == list(capi.COV_SUMMARY_DTYPE.names)
    assert [a.split()[0] for a in args] == ["int64_t", "int64_t", "int32_t", "int64_t"]
    assert [capi.COV_SUMMARY_DTYPE[n].str for n in capi.COV_SUMMARY_DTYPE.names] == ["<i8", "<i8", "<i4", "<i8"]
    assert capi.COV_SUMMARY_DTYPE == covref.SUMMARY_DTYPE
    for name in ("create", "free", "reset", "device_bytes", "summary", "fetch_bins", "fetch_depth", "device"):
        assert "mnc_coverage_" + name in capi.EXPORTS
    assert "mnc_engine_add_coverage" in capi.EXPORTS
    # the three rows of the limits table
    limits = text[text.index("limits, and what happens at each"):text.index("---- classify")]
    assert "mnc_engine_add_coverage: MNC_ERR_UNSUPPORTED" in limits and "MNC_COV_SPAN" in limits and "2^31" in limits


# ---------------------------------------------------------------- errors that need no device
def test_create_without_a_device_and_argument_errors(capi):
    L = capi.lib()
    idx = capi.Index.from_seqs(["a:1"], [np.frombuffer(b"ACGTTGCAAGGCTTAACCGGTATGCATGCAAT" * 40, dtype=np.uint8)])
    h = C.c_void_p()
    # a device that does not exist -- on a machine without a GPU that is device 0
    n_dev = capi.device_count()
    assert L.mnc_coverage_create(idx._h, n_dev, 1024, C.byref(h)) == capi.ERR_NODEVICE and not h.value
    try:
        capi.Coverage(idx, n_dev, 1024)
        raise AssertionError("no error")
    except capi.MncError as err:
        assert err.code == capi.ERR_NODEVICE
    # the arguments are checked first
    assert L.mnc_coverage_create(None, n_dev, 1024, C.byref(h)) == capi.ERR_ARG
    assert L.mnc_coverage_create(idx._h, n_dev, 1024, None) == capi.ERR_ARG
    for bad in (0, -1, -(1 << 31)):
        assert L.mnc_coverage_create(idx._h, n_dev, bad, C.byref(h)) == capi.ERR_ARG and not h.value
    n = C.c_int64(7)
    assert L.mnc_coverage_reset(None) == capi.ERR_ARG
    assert L.mnc_coverage_device_bytes(None, C.byref(n)) == capi.ERR_ARG
    assert L.mnc_coverage_summary(None, None, None, None, None) == capi.ERR_ARG
    assert L.mnc_coverage_fetch_bins(None, 0, None, None, 0, C.byref(n)) == capi.ERR_ARG
    assert L.mnc_coverage_fetch_depth(None, 0, 0, 0, None) == capi.ERR_ARG
    assert L.mnc_coverage_device(None, None, C.byref(n)) == capi.ERR_ARG
    assert L.mnc_engine_add_coverage(None, None, capi.COV_GATED) == capi.ERR_ARG
    assert n.value == 7
    L.mnc_coverage_free(None)                                      # a no-op
