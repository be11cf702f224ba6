"""What the abundance feature promises without a GPU: the library exports the new symbols, the binding matches the header,
the plain-numpy contract (tests/abundref.py) gives its known answers, and the argument checks that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import abundref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "monica_amd.h")
SYMBOLS = ("create", "free", "reset", "device_bytes", "add_lists", "info", "fetch_unique", "fetch_lists", "solve", "device")


def test_library_exports_every_new_symbol(capi):
    for name in SYMBOLS:
        assert "mnc_abundance_" + name in capi.EXPORTS and hasattr(capi.lib(), "mnc_abundance_" + name)
    assert "mnc_engine_add_abundance" in capi.EXPORTS and hasattr(capi.lib(), "mnc_engine_add_abundance")
    text = open(HEADER).read()
    section = text[text.index("------ abundance"):text.index("------ FASTQ batches")]
    for name in SYMBOLS:
        assert re.search(r"\bmnc_abundance_" + name + r"\(", section), name
    # the four doubles of the weight table, as the header spells them, are the ones the reference uses
    for h in ("0x1.0000000000000p+0", "0x1.ae89f995ad3adp-1", "0x1.6a09e667f3bcdp-1", "0x1.306fe0a31b715p-1"):
        assert h in section
    assert "best_n = 5" in section and "not\n * been fitted" in section
    limits = text[text.index("limits, and what happens at each"):text.index("---- classify")]
    assert "mnc_engine_add_abundance: MNC_ERR_UNSUPPORTED" in limits and "mnc_engine_add_abundance: MNC_ERR_ARG" in limits
    for name in ("add_lists", "info", "unique", "lists", "solve", "reset", "close"):
        assert callable(getattr(capi.Abundance, name))
    assert callable(capi.Engine.add_abundance)
    assert (capi.ABUNDANCE_MAX_DELTA, capi.ABUNDANCE_SCALE_Q) == (abundref.MAX_DELTA, abundref.SCALE_Q) == (80, 3)


def test_python_signatures(capi):
    from monica_amd import aligner, mappy_compat
    for f in (aligner.aligner_coverage, aligner.multi_threaded_aligner):
        p = inspect.signature(f).parameters
        assert "abundance" in p and p["abundance"].default is None
        assert p["abundance"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert "abundance" not in inspect.signature(aligner.aligner).parameters
    p = inspect.signature(mappy_compat.Aligner.map_batch).parameters
    assert p["abundance"].default is None
    p = inspect.signature(mappy_compat.Aligner.abundance).parameters
    assert (p["max_delta"].default, p["scale_q"].default) == (80, 3) and "cap_cands" in p
    assert inspect.signature(capi.Abundance.solve).parameters["max_iter"].default == 200 == inspect.signature(abundref.solve).parameters["max_iter"].default


# ---------------------------------------------------------------- the weight table
def test_weights_against_two_to_the_minus_x_over_four():
    for scale_q in (1, 3, 7):
        delta = np.arange(0, abundref.MAX_PRODUCT // scale_q + 1)
        w = abundref.weights(delta, scale_q)
        want = 2.0 ** (-(delta * scale_q) / 4.0)
        assert w.dtype == np.float64 and (w > 0).all()
        assert (np.abs(w - want) <= np.spacing(want)).all()                # 1 ulp
        assert (w >= np.finfo(np.float64).tiny).all()                      # normal doubles down to the largest product
    assert abundref.weights([0], 3)[0] == 1.0 and abundref.weights([4], 1)[0] == 0.5 and abundref.weights([4], 3)[0] == 0.125
    assert abundref.weights([2], 3)[0] == abundref.T[2] * 0.5              # x = 6: T[2] * 2^-1, exactly


# ---------------------------------------------------------------- candidates
REC = np.dtype([("rid", "<i4"), ("dp_max", "<i4"), ("n_cigar", "<i4")])


def recs(*rows):
    return np.array(list(rows), dtype=REC)


def test_candidates():
    cg = [0, 1, 2, 1]                                                       # contigs 1 and 3 share genome 1
    assert abundref.candidates(recs(), cg) == []
    assert abundref.candidates(recs((0, 500, 0)), cg) == []                 # no CIGAR: not a record here
    assert abundref.candidates(recs((2, 500, 9)), cg) == [(2, 0)]
    # the per-genome maximum, ascending genome id, the delta cut at exactly max_delta
    r = recs((2, 900, 5), (0, 1000, 7), (1, 700, 3), (3, 920, 4), (0, 400, 2))
    assert abundref.candidates(r, cg, 80) == [(0, 0), (1, 80)]
    assert abundref.candidates(r, cg, 79) == [(0, 0)]
    assert abundref.candidates(r, cg, 100) == [(0, 0), (1, 80), (2, 100)]
    unique, rows, n = abundref.collect([r, recs((2, 500, 9)), recs(), recs((1, 10, 1), (3, 10, 1))], cg, 3, 100)
    assert unique.tolist() == [0, 1, 1] and rows == [[(0, 0), (1, 80), (2, 100)]] and n == 3
    assert abundref.sort_rows([[(1, 0), (2, 0)], [(0, 5), (2, 0)], [(0, 0), (2, 0), (3, 1)], [(0, 0), (2, 0)]]) == \
        [[(0, 0), (2, 0)], [(0, 0), (2, 0), (3, 1)], [(0, 5), (2, 0)], [(1, 0), (2, 0)]]
    off, gen, dlt = abundref.rows_to_csr(rows)
    assert off.tolist() == [0, 3] and abundref.csr_to_rows(off, gen, dlt) == rows


# ---------------------------------------------------------------- the EM's known answers
def test_two_genomes_converge_monotonically_towards_the_one_with_more_unique_reads():
    rows = [[(0, 0), (1, 0)]] * 10
    trace = []
    theta, expected, iters = abundref.solve([3, 1], rows, 2, max_iter=400, tol_q32=0, trace=trace)
    t0 = [t[0] for t, _ in trace]
    assert len(trace) == iters and 2 <= iters <= 400
    assert trace[0][1] == [(3 << 32) + 10 * (1 << 31), (1 << 32) + 10 * (1 << 31)]      # theta = 1/2 each: half a read each
    # [1, 0]-ward, monotonically: theta_0' = (3 + 10 theta_0) / 14 climbs from 1/2 towards its fixed point 3/4 -- the ambiguous
    # reads follow the unique ones' proportions -- and the floors keep it just below
    assert all(b >= a for a, b in zip(t0, t0[1:])) and t0[0] == 8.0 / 14.0 and t0[1] > t0[0]
    assert 0.7499 < t0[-1] <= 0.75 and theta[0] == t0[-1] and abs(theta.sum() - 1.0) < 1e-15
    n_reads, n_cands = 14, 20
    assert n_reads - n_cands * 2.0 ** -32 <= expected.sum() <= n_reads


def test_a_row_with_delta_at_max_delta():
    # one row (0:0, 1:80) at scale_q = 3: x = 240, w = 2^-60 -- z = 1/2 + 2^-61 rounds to 1/2, p_0 = 1 and genome 1 gets
    # floor(2^-60 * 2^32) = 0 of the read
    theta, expected, iters = abundref.solve([0, 0], [[(0, 0), (1, 80)]], 2, scale_q=3, max_iter=1)
    assert iters == 1 and abundref.weights([80], 3)[0] == 2.0 ** -60
    assert theta.tolist() == [1.0, 0.0] and expected.tolist() == [1.0, 0.0]
    # at scale_q = 1 (w = 2^-20) it keeps a share: p_1 = 2^-20 / (1 + 2^-20)
    theta, expected, _ = abundref.solve([0, 0], [[(0, 0), (1, 80)]], 2, scale_q=1, max_iter=1)
    p1 = np.float64(2.0 ** -21) / (np.float64(0.5) + np.float64(2.0 ** -21))
    assert expected[1] == np.floor(p1 * 2.0 ** 32) / 2.0 ** 32 and 0 < theta[1] < 1e-6


def test_without_stored_rows_the_first_iteration_is_the_fixed_point():
    one = abundref.solve([5, 0, 3], [], 3, max_iter=1)
    many = abundref.solve([5, 0, 3], [], 3, max_iter=50, tol_q32=0)
    assert one[2] == 1 and many[2] == 2                                     # the test is met at the second iteration: nothing moved
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1])
    assert one[0].tolist() == [5 / 8, 0.0, 3 / 8] and one[1].tolist() == [5.0, 0.0, 3.0]
    nothing = abundref.solve([0, 0], [], 2)
    assert nothing[0].tolist() == [0, 0] and nothing[1].tolist() == [0, 0] and nothing[2] == 0


def test_the_answer_does_not_depend_on_row_order():
    rng = np.random.default_rng(5)
    rows = []
    for _ in range(200):
        gs = sorted(rng.choice(7, size=int(rng.integers(2, 5)), replace=False).tolist())
        rows.append([(g, int(rng.integers(0, 81))) for g in gs])
    a = abundref.solve([4, 0, 9, 1, 0, 0, 2], rows, 7, max_iter=9, tol_q32=0)
    b = abundref.solve([4, 0, 9, 1, 0, 0, 2], [rows[i] for i in rng.permutation(len(rows))], 7, max_iter=9, tol_q32=0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 9


# ---------------------------------------------------------------- argument checks that need no device
def test_python_argument_checks(capi):
    idx = capi.Index.from_seqs(["a:1"], [np.frombuffer(b"ACGTTGCAAGGCTTAACCGGTATGCATGCAAT" * 40, dtype=np.uint8)])
    for kw in (dict(cap_cands=-1), dict(max_delta=-1), dict(scale_q=0), dict(max_delta=81, scale_q=50), dict(max_delta=4001, scale_q=1)):
        with pytest.raises(ValueError):
            capi.Abundance(idx, 0, **kw)
    L = capi.lib()
    h = C.c_void_p()
    n_dev = capi.device_count()                                    # a device that does not exist -- without a GPU that is device 0
    for args in ((-1, 80, 3), (100, -1, 3), (100, 80, 0), (100, 1001, 4), (100, 4001, 1)):
        assert L.mnc_abundance_create(idx._h, n_dev, *args, C.byref(h)) == capi.ERR_ARG and not h.value
    assert L.mnc_abundance_create(idx._h, n_dev, 100, 1000, 4, C.byref(h)) == capi.ERR_NODEVICE and not h.value   # the largest product is fine
    with pytest.raises(capi.MncError) as err:
        capi.Abundance(idx, n_dev)
    assert err.value.code == capi.ERR_NODEVICE
    assert L.mnc_abundance_create(None, n_dev, 100, 80, 3, C.byref(h)) == capi.ERR_ARG
    assert L.mnc_abundance_create(idx._h, n_dev, 100, 80, 3, None) == capi.ERR_ARG
    n = C.c_int64(7)
    it = C.c_int32(0)
    assert L.mnc_abundance_reset(None) == capi.ERR_ARG
    assert L.mnc_abundance_device_bytes(None, C.byref(n)) == capi.ERR_ARG
    assert L.mnc_abundance_info(None, None, None, None, None) == capi.ERR_ARG
    assert L.mnc_abundance_fetch_unique(None, None) == capi.ERR_ARG
    assert L.mnc_abundance_fetch_lists(None, None, None, None, 0, 0) == capi.ERR_ARG
    assert L.mnc_abundance_add_lists(None, 0, None, None, None) == capi.ERR_ARG
    assert L.mnc_abundance_solve(None, 1, 0, None, None, C.byref(it)) == capi.ERR_ARG
    assert L.mnc_abundance_device(None, None, None, None, None) == capi.ERR_ARG
    assert L.mnc_engine_add_abundance(None, None) == capi.ERR_ARG
    L.mnc_abundance_free(None)


def test_a_database_of_several_parts_is_refused_before_anything_runs(tmp_path):
    from monica_amd import aligner
    cwd = os.getcwd()
    query = tmp_path / "query"
    query.mkdir()
    (query / "s.fastq").write_bytes(b"@r1\nACGT\n+\nIIII\n")
    try:
        with pytest.raises(ValueError, match="ONE index part"):
            aligner.multi_threaded_aligner(str(query), ["index0.mmi", "index1.mmi"], mode="basic", abundance=True)
        assert os.getcwd() == cwd and sorted(os.listdir(query)) == ["s.fastq"]    # no folder made, no index loaded
        hits = tmp_path / "hits"
        hits.mkdir()
        with pytest.raises(ValueError, match="ONE index part"):                   # a part that is not the last
            aligner.aligner_coverage(str(query / "s.fastq"), "s", None, "basic", str(hits), 60, last_index=False, abundance=True)
        (hits / "s_hits.pkl").write_bytes(b"")
        with pytest.raises(ValueError, match="ONE index part"):                   # hits carried over from an earlier part
            aligner.aligner_coverage(str(query / "s.fastq"), "s", None, "basic", str(hits), 60, last_index=True, abundance=True)
    finally:
        os.chdir(cwd)
