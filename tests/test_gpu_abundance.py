"""Abundance by EM over every candidate genome, on the device (mnc_abundance_*, mnc_engine_add_abundance; csrc/k_abundance.hip).

Reference: tests/abundref.py -- the contract in plain numpy -- applied to the CPU ORACLE's regions (oracle.Index.map_cigar,
opt.cigar = 1).  Nothing is compared against the engine's own dumps or export.  The EM is compared bit for bit: float64
arrays with np.array_equal."""
import ctypes as C
import os
import pickle
import threading

import numpy as np
import pytest

import abundref
import util
from monica_amd import synth
from test_gpu_alignments import mutate

pytestmark = pytest.mark.gpu

ACGT = util.ACGT
MIN_MAPQ = 60
LDS_G = 2048                                     # csrc/k_abundance.hip: AB_LDS_G, the cut-off it states
TOL = 1 << 22


class World:
    """Five contigs, four genomes: A (60 kb) and a second, unrelated contig of the SAME name (45 kb, so the two share a
    genome); B (40 kb); C, a 1 % diverged copy of A's first 50 kb; D, a 0.3 % diverged copy of the whole of A.  A read from
    A's first 50 kb fits A and D about equally well and C nearly so: rows of two and of three candidates; reads from B and
    from A's second contig have one."""

    def __init__(self, capi, oracle):
        names, seqs = util.small_genomes(4, 70_000, 70_000)
        a = seqs[0][:60_001].copy()
        self.names = [names[0], names[1], names[2], names[3], names[0]]
        self.seqs = [a, seqs[1][:40_003].copy(), synth.diverge(a, 0x77, 10_000)[:50_000].copy(), synth.diverge(a, 0x99, 3_000).copy(),
                     seqs[2][:45_000].copy()]
        self.capi = capi
        self.idx = capi.Index.from_seqs(self.names, self.seqs)
        self.oidx = oracle.Index.from_seqs(self.names, [s.tobytes() for s in self.seqs])
        self.oidx.opt.cigar = 1
        self.eng = capi.Engine(self.idx, 0)
        self.cg = [int(g) for g in self.idx.contig_genome]
        self.G = len(self.idx.genome_names)
        assert self.G == 4 and self.cg[0] == self.cg[4] and len(set(self.cg)) == 4

    def oracle_regs(self, reads):
        return [self.oidx.map_cigar(np.asarray(rd, dtype=np.uint8).tobytes())[0] for rd in reads]


@pytest.fixture(scope="module")
def world(capi, oracle):
    return World(capi, oracle)


@pytest.fixture(scope="module")
def corpus(world):
    """~150 reads of 1.5-2 kb at 10 % errors from both strands, random reads and a chimera among them; the oracle's answer
    is computed once on the CPU, and checked to hold what the tests rely on."""
    rng = np.random.default_rng(0xAB0D)
    reads = []
    for i in range(140):
        g = world.seqs[i % 5]
        n = int(rng.integers(1500, 2001))
        s = int(rng.integers(0, len(g) - n))
        rd = mutate(rng, g[s:s + n])
        reads.append(util.revcomp(rd) if rng.integers(0, 2) else rd)
    for i in range(8):
        reads.insert(int(rng.integers(0, len(reads) + 1)), ACGT[rng.integers(0, 4, 1800)])
    reads.append(np.concatenate([mutate(rng, world.seqs[1][2_000:2_900]), mutate(rng, world.seqs[0][52_000:53_200])]))   # a chimera of B and A's tail
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    bases, offsets = util.pack_reads(reads)
    regs = world.oracle_regs(reads)
    unique, rows, n_reads = abundref.collect(regs, world.cg, world.G)
    # ---- what keeps the tests honest, on the oracle's output
    assert len(rows) >= 30, "stored rows"
    assert sum(len(r) == 3 for r in rows) >= 5, "rows with three candidates"
    assert int(unique.sum()) >= 20, "unique reads"
    assert sum(len(abundref.candidates(r, world.cg)) == 0 for r in regs) >= 1, "a read with no record"
    assert n_reads == int(unique.sum()) + len(rows) < len(reads)
    assert any(d > 0 for row in rows for _, d in row)
    return dict(reads=reads, bases=bases, offsets=offsets, regs=regs, unique=unique, rows=rows, n_reads=n_reads,
                n_cands=sum(len(r) for r in rows))


def held(ab):
    """What the accumulator holds, in the reference's terms."""
    off, gen, dlt = ab.lists()
    return ab.unique(), abundref.csr_to_rows(off, gen, dlt), ab.info()


def check_collection(ab, unique, rows, n_reads, scale=1):
    got_unique, got_rows, info = held(ab)
    assert got_unique.dtype == np.int64 and np.array_equal(got_unique, unique * scale)
    assert got_rows == abundref.sort_rows(rows * scale)
    assert info == dict(n_reads=n_reads * scale, n_stored_reads=len(rows) * scale, n_cands=sum(len(r) for r in rows) * scale, n_dropped=0)


def check_solve(ab, unique, rows, G, scale_q=abundref.SCALE_Q, n_reads=None, **kw):
    theta, expected, iters = ab.solve(**kw)
    w_theta, w_expected, w_iters = abundref.solve(unique, rows, G, scale_q, n_reads=n_reads, **kw)
    assert theta.dtype == expected.dtype == np.float64
    assert iters == w_iters, f"{iters} iterations, the reference ran {w_iters}"
    assert np.array_equal(theta, w_theta), f"theta {theta} != {w_theta}"
    assert np.array_equal(expected, w_expected), f"expected {expected} != {w_expected}"
    return theta, expected, iters


# ---------------------------------------------------------------- 1. collection
def test_collection_equals_the_reference(capi, world, corpus):
    world.eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    ab = capi.Abundance(world.idx, 0, cap_cands=4096)
    assert 12 * 4096 <= ab.device_bytes() < 12 * 4096 + (1 << 12)
    world.eng.add_abundance(ab)
    check_collection(ab, corpus["unique"], corpus["rows"], corpus["n_reads"])
    check_collection(ab, corpus["unique"], corpus["rows"], corpus["n_reads"])          # reading does not change it
    # a tighter cut: fewer candidates, more unique reads
    tight = capi.Abundance(world.idx, 0, cap_cands=4096, max_delta=20)
    world.eng.add_abundance(tight)
    u20, r20, n20 = abundref.collect(corpus["regs"], world.cg, world.G, 20)
    assert n20 == corpus["n_reads"] and len(r20) < len(corpus["rows"])
    check_collection(tight, u20, r20, n20)
    ptrs = ab.device_arrays()
    assert all(ptrs)
    ab.close(), tight.close()


# ---------------------------------------------------------------- 2. additivity
def test_one_batch_equals_three_and_two_engines_on_two_threads(capi, world, corpus):
    n = len(corpus["reads"])
    off = corpus["offsets"]
    cuts = [0, n // 3, 2 * n // 3, n]
    ab = capi.Abundance(world.idx, 0, cap_cands=8192)
    for a, b in zip(cuts, cuts[1:]):
        world.eng.classify(corpus["bases"][off[a]:off[b]], off[a:b + 1] - off[a], MIN_MAPQ)
        world.eng.add_abundance(ab)
    check_collection(ab, corpus["unique"], corpus["rows"], corpus["n_reads"])
    three = ab.solve()
    ab.reset()
    assert held(ab)[2] == dict(n_reads=0, n_stored_reads=0, n_cands=0, n_dropped=0) and not ab.unique().any()
    # two engines, each on its own thread, add the whole corpus to the one accumulator at the same time (mnc_pileup's rule)
    other = capi.Engine(world.idx, 0)
    errors = []

    def run(eng):
        try:
            eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
            eng.add_abundance(ab)
            eng.sync()
        except BaseException as e:                                # noqa: B036 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=run, args=(e,)) for e in (world.eng, other)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    check_collection(ab, corpus["unique"], corpus["rows"], corpus["n_reads"], scale=2)
    check_solve(ab, corpus["unique"] * 2, corpus["rows"] * 2, world.G, max_iter=5, tol_q32=0)
    ab.reset()
    world.eng.add_abundance(ab)                                   # on after a reset: the batch is still in the engine
    one = ab.solve()
    assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1]) and one[2] == three[2]
    other.close(), ab.close()


# ---------------------------------------------------------------- 3. solve
def test_solve_bit_for_bit(capi, world, corpus):
    n = len(corpus["reads"])
    half = n // 2
    off = corpus["offsets"]
    ab = capi.Abundance(world.idx, 0, cap_cands=4096)
    world.eng.classify(corpus["bases"][:off[half]], off[:half + 1], MIN_MAPQ)
    world.eng.add_abundance(ab)
    u1, r1, n1 = abundref.collect(corpus["regs"][:half], world.cg, world.G)
    check_solve(ab, u1, r1, world.G, max_iter=200, tol_q32=TOL)                        # between the batches of a run
    world.eng.classify(corpus["bases"][off[half]:], off[half:] - off[half], MIN_MAPQ)
    world.eng.add_abundance(ab)
    args = (corpus["unique"], corpus["rows"], world.G)
    first = check_solve(ab, *args, max_iter=200, tol_q32=TOL)                          # solve, add more, solve = add everything, solve
    assert 2 <= first[2] < 200, "stopped by tol_q32"
    again = ab.solve(max_iter=200, tol_q32=TOL)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]
    # a stop by max_iter; with tol_q32 = 0 this corpus reaches its integer fixed point after a few iterations, and the run
    # stops there -- test_a_stop_by_max_iter has a system that is still moving at iteration 7
    settled = abundref.solve(*args, max_iter=200, tol_q32=0)[2]
    for max_iter in (1, 2, 7):
        assert check_solve(ab, *args, max_iter=max_iter, tol_q32=0)[2] == min(max_iter, settled)
    assert abs(first[0].sum() - 1.0) < 1e-12
    assert corpus["n_reads"] - corpus["n_cands"] * 2.0 ** -32 <= first[1].sum() <= corpus["n_reads"]
    check_collection(ab, corpus["unique"], corpus["rows"], corpus["n_reads"])          # solve leaves the accumulator as it is
    it = C.c_int32(9)
    assert capi.lib().mnc_abundance_solve(ab._h, 0, 0, first[0].ctypes.data, first[1].ctypes.data, C.byref(it)) == capi.ERR_ARG
    ab.close()


# ---------------------------------------------------------------- 4. the smallest shapes, through add_lists
_INDEXES = {}


def index_of(capi, G):
    """An index of G genomes of one short contig each (the accumulator takes G and nothing else from it)."""
    if G not in _INDEXES:
        rng = np.random.default_rng(G)
        _INDEXES[G] = capi.Index.from_seqs([f"t{g}:acc{g}" for g in range(G)], [ACGT[rng.integers(0, 4, 80)] for _ in range(G)])
        assert len(_INDEXES[G].genome_names) == G
    return _INDEXES[G]


def random_rows(rng, G, n, lo, hi, max_delta, first_and_last=True):
    rows = []
    for i in range(n):
        k = int(rng.integers(lo, hi + 1))
        gs = set(rng.choice(G, size=k, replace=False).tolist())
        if first_and_last and i % 7 == 0:
            gs |= {0, G - 1}
        rows.append([(g, int(rng.integers(0, max_delta + 1))) for g in sorted(gs)])
    return rows


def via_add_lists(capi, G, unique_reads, rows, scale_q=3, max_delta=80, shuffle=None, **kw):
    """The rows and the unique reads (genome ids) through add_lists, in one call's order; solved and compared."""
    lists = [[(g, 0)] for g in unique_reads] + rows
    if shuffle is not None:
        lists = [lists[i] for i in shuffle.permutation(len(lists))]
    ab = capi.Abundance(index_of(capi, G), 0, cap_cands=max(sum(len(r) for r in rows), 1), max_delta=max_delta, scale_q=scale_q)
    ab.add_lists(*abundref.rows_to_csr(lists))
    unique = np.bincount(np.asarray(unique_reads, dtype=np.int64), minlength=G).astype(np.int64)
    check_collection(ab, unique, rows, len(lists))
    out = check_solve(ab, unique, rows, G, scale_q, n_reads=len(lists), **kw)
    ab.close()
    return out


def test_one_genome(capi):
    theta, expected, iters = via_add_lists(capi, 1, [0, 0, 0], [], max_iter=20, tol_q32=0)
    assert theta.tolist() == [1.0] and expected.tolist() == [3.0] and iters == 2


def test_no_rows_at_all(capi):
    ab = capi.Abundance(index_of(capi, 3), 0, cap_cands=0)
    ab.add_lists(np.zeros(1, dtype=np.int64), [], [])
    theta, expected, iters = ab.solve()
    assert theta.tolist() == [0, 0, 0] and expected.tolist() == [0, 0, 0] and iters == 0
    check_collection(ab, np.zeros(3, dtype=np.int64), [], 0)
    ab.close()


def test_only_unique_reads(capi):
    theta, expected, iters = via_add_lists(capi, 3, [0] * 5 + [2] * 3, [], max_iter=50, tol_q32=0)
    assert theta.tolist() == [5 / 8, 0.0, 3 / 8] and expected.tolist() == [5.0, 0.0, 3.0] and iters == 2


def test_one_row_of_two_candidates(capi):
    via_add_lists(capi, 3, [], [[(0, 0), (2, 1)]], max_iter=30, tol_q32=0)
    via_add_lists(capi, 3, [2], [[(0, 0), (2, 1)]], max_iter=30, tol_q32=TOL)


def test_one_row_with_every_one_of_70_genomes(capi):
    rng = np.random.default_rng(70)
    row = [(g, int(rng.integers(0, 81))) for g in range(70)]
    via_add_lists(capi, 70, [3, 3, 69], [row], max_iter=12, tol_q32=0)


def test_70000_rows_of_two_to_five_candidates(capi):
    rng = np.random.default_rng(70_000)
    rows = random_rows(rng, 20, 70_000, 2, 5, 80, first_and_last=False)
    via_add_lists(capi, 20, rng.integers(0, 20, 500).tolist(), rows, max_iter=2, tol_q32=0)


@pytest.mark.parametrize("G", [LDS_G - 1, LDS_G, LDS_G + 1])
def test_around_the_lds_cut_off(capi, G):
    rng = np.random.default_rng(G)
    rows = random_rows(rng, G, 3000, 2, 5, 80)
    assert any(r[0][0] == 0 and r[-1][0] == G - 1 for r in rows)
    via_add_lists(capi, G, [0, G - 1, G // 2, G - 1], rows, max_iter=3, tol_q32=0)


@pytest.mark.parametrize("scale_q,max_delta", [(1, 80), (3, 80), (4, 1000), (4000, 1)])
def test_deltas_of_zero_and_of_max_delta(capi, scale_q, max_delta):
    rng = np.random.default_rng(scale_q)
    rows = [[(0, 0), (1, max_delta)], [(0, max_delta), (1, 0), (3, 0)], [(1, max_delta), (2, max_delta)], [(0, 0), (4, 0)]]
    rows += random_rows(rng, 5, 60, 2, 4, max_delta, first_and_last=False)
    via_add_lists(capi, 5, [1, 4], rows, scale_q=scale_q, max_delta=max_delta, max_iter=6, tol_q32=0)


def test_a_stop_by_max_iter(capi):
    rng = np.random.default_rng(11)
    rows = random_rows(rng, 9, 2000, 2, 6, 80)
    uniq = rng.integers(0, 9, 40).tolist()
    for max_iter in (1, 2, 7):
        assert via_add_lists(capi, 9, uniq, rows, max_iter=max_iter, tol_q32=0)[2] == max_iter


def test_rows_in_shuffled_order_give_the_identical_answer(capi):
    rng = np.random.default_rng(11)
    rows = random_rows(rng, 9, 2000, 2, 6, 80)
    uniq = rng.integers(0, 9, 40).tolist()
    a = via_add_lists(capi, 9, uniq, rows, max_iter=8, tol_q32=0)
    b = via_add_lists(capi, 9, uniq, rows, max_iter=8, tol_q32=0, shuffle=np.random.default_rng(12))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 8
    # ... and so do the same rows given in three calls
    ab = capi.Abundance(index_of(capi, 9), 0, cap_cands=sum(len(r) for r in rows))
    lists = [[(g, 0)] for g in uniq] + rows
    for part in (lists[:700], lists[700:701], lists[701:]):
        ab.add_lists(*abundref.rows_to_csr(part))
    c = ab.solve(max_iter=8, tol_q32=0)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and c[2] == 8
    ab.close()


# ---------------------------------------------------------------- 5. capacity
def test_capacity(capi, world, corpus):
    L = capi.lib()
    world.eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    short = capi.Abundance(world.idx, 0, cap_cands=corpus["n_cands"] - 1)
    world.eng.add_abundance(short)
    unique, rows, info = held(short)
    assert info["n_dropped"] >= 1 and info["n_cands"] <= corpus["n_cands"] - 1
    # nothing lies beyond the buffer: what was stored is a sub-multiset of the reference's rows, and the counts agree with it
    want = abundref.sort_rows(corpus["rows"])
    left = list(want)
    for r in rows:
        left.remove(r)
    assert info["n_stored_reads"] == len(rows) == len(want) - info["n_dropped"] and info["n_cands"] == sum(len(r) for r in rows)
    assert info["n_reads"] == corpus["n_reads"] - info["n_dropped"] and np.array_equal(unique, corpus["unique"])   # a dropped row is no unique read
    theta, expected = np.full(world.G, -7.0), np.full(world.G, -7.0)
    it = C.c_int32(0)
    assert L.mnc_abundance_solve(short._h, 10, 0, theta.ctypes.data, expected.ctypes.data, C.byref(it)) == capi.ERR_RANGE
    with pytest.raises(capi.MncError) as err:
        short.solve()
    assert err.value.code == capi.ERR_RANGE
    short.reset()
    assert short.info() == dict(n_reads=0, n_stored_reads=0, n_cands=0, n_dropped=0)
    short.close()
    enough = capi.Abundance(world.idx, 0, cap_cands=corpus["n_cands"])                   # exactly what the corpus needs
    world.eng.add_abundance(enough)
    check_collection(enough, corpus["unique"], corpus["rows"], corpus["n_reads"])
    check_solve(enough, corpus["unique"], corpus["rows"], world.G, max_iter=4, tol_q32=0)
    # add_lists beyond capacity: MNC_ERR_RANGE, nothing added, n_dropped stays 0
    before = held(enough)
    off, gen, dlt = abundref.rows_to_csr([[(1, 0)], [(0, 0), (1, 3)]])
    assert L.mnc_abundance_add_lists(enough._h, 2, off.ctypes.data, gen.ctypes.data, dlt.ctypes.data) == capi.ERR_RANGE
    after = held(enough)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1] and before[2] == after[2] and after[2]["n_dropped"] == 0
    enough.close()


# ---------------------------------------------------------------- 6. errors
def test_errors_leave_the_accumulator_untouched(capi, world, corpus):
    L = capi.lib()
    h = C.c_void_p()
    for args in ((-1, 80, 3), (100, -1, 3), (100, 80, 0), (100, 1001, 4)):
        assert L.mnc_abundance_create(world.idx._h, 0, *args, C.byref(h)) == capi.ERR_ARG and not h.value
    n20 = 20
    off = corpus["offsets"][:n20 + 1]
    ab = capi.Abundance(world.idx, 0, cap_cands=4096)
    ab.add_lists(*abundref.rows_to_csr([[(1, 0)], [(0, 0), (3, 7)]]))
    before = held(ab)
    assert before[2] == dict(n_reads=2, n_stored_reads=1, n_cands=2, n_dropped=0)

    def unchanged():
        now = held(ab)
        return np.array_equal(before[0], now[0]) and before[1] == now[1] and before[2] == now[2]

    fresh = capi.Engine(world.idx, 0)
    assert L.mnc_engine_add_abundance(fresh._h, ab._h) == capi.ERR_ARG                  # no batch has been classified
    fresh.set_contract(capi.CONTRACT_CHAIN)
    fresh.classify(corpus["bases"][:off[-1]], off, MIN_MAPQ)
    assert L.mnc_engine_add_abundance(fresh._h, ab._h) == capi.ERR_ARG                  # MNC_CONTRACT_CHAIN: no dp_max
    fresh.close()
    assert unchanged()
    world.eng.classify(corpus["bases"][:off[-1]], off, MIN_MAPQ)
    other_idx = capi.Index.from_seqs(world.names[:1], [world.seqs[1][:20_000]])
    other = capi.Abundance(other_idx, 0, cap_cands=64)
    assert L.mnc_engine_add_abundance(world.eng._h, other._h) == capi.ERR_ARG           # an accumulator of another index
    assert other.info() == dict(n_reads=0, n_stored_reads=0, n_cands=0, n_dropped=0)
    other.close()
    n_dev = capi.device_count()
    if n_dev > 1:                                                                       # ... of another device
        far = capi.Abundance(world.idx, 1, cap_cands=64)
        assert L.mnc_engine_add_abundance(world.eng._h, far._h) == capi.ERR_ARG
        far.close()
    # add_lists: every malformed row
    for rows in ([[(0, 0), (0, 1)]], [[(2, 0), (1, 0)]], [[(0, 0), (4, 0)]], [[(-1, 0), (1, 0)]], [[(0, 0), (1, -1)]], [[(0, 0), (1, 81)]],
                 [[(0, 0), (1, 0)], [(4, 0)]]):
        o, g, d = abundref.rows_to_csr(rows)
        assert L.mnc_abundance_add_lists(ab._h, len(rows), o.ctypes.data, g.ctypes.data, d.ctypes.data) == capi.ERR_ARG, rows
    o = np.array([0, 2, 2], dtype=np.int64)                                              # an empty row
    g, d = np.array([0, 1], dtype=np.int32), np.zeros(2, dtype=np.int32)
    assert L.mnc_abundance_add_lists(ab._h, 2, o.ctypes.data, g.ctypes.data, d.ctypes.data) == capi.ERR_ARG
    assert unchanged()
    ab.close()


def test_a_mixed_call_of_long_and_short_reads_is_refused(capi):
    n = (1 << 20) + 5000
    g = synth.genome(0x5151, 1_100_000)
    idx = capi.Index.from_seqs([synth.contig_name(0)], [g])
    eng = capi.Engine(idx, 0)
    eng.set_long_reads(True)
    ab = capi.Abundance(idx, 0, cap_cands=64)
    long_read = g[20_000:20_000 + n].copy()
    assign, _, _ = eng.classify(*util.pack_reads([long_read, g[500_000:502_000]]), MIN_MAPQ)
    assert assign.tolist() == [0, 0]
    assert capi.lib().mnc_engine_add_abundance(eng._h, ab._h) == capi.ERR_UNSUPPORTED   # the engine holds the wide pass alone
    assert ab.info() == dict(n_reads=0, n_stored_reads=0, n_cands=0, n_dropped=0)
    ab.close(), eng.close()


# ---------------------------------------------------------------- 7. meaning
def test_a_mixture_of_three_close_genomes_is_ordered(capi, world):
    """70 / 20 / 10 % of the reads from A, D (0.3 % from A) and C (1 % from A), all from the 50 kb the three share.  Only the
    order of the three theta and the bounds on sum(expected) are asserted; the accuracy is reported in RESULTS.md."""
    rng = np.random.default_rng(0x3173)
    reads = []
    for contig, count in ((0, 140), (3, 40), (2, 20)):
        g = world.seqs[contig][:50_000]
        for _ in range(count):
            n = int(rng.integers(1500, 2001))
            s = int(rng.integers(0, len(g) - n))
            rd = mutate(rng, g[s:s + n])
            reads.append(util.revcomp(rd) if rng.integers(0, 2) else rd)
    reads = [reads[i] for i in rng.permutation(len(reads))]
    ab = capi.Abundance(world.idx, 0, cap_cands=4096)
    world.eng.classify(*util.pack_reads(reads), MIN_MAPQ)
    world.eng.add_abundance(ab)
    theta, expected, iters = ab.solve()
    info = ab.info()
    a, d, c = world.cg[0], world.cg[3], world.cg[2]
    print(f"mixture 0.70 / 0.20 / 0.10: theta A {theta[a]:.4f} D {theta[d]:.4f} C {theta[c]:.4f} B {theta[world.cg[1]]:.4f}, {iters} iterations, {info}")
    assert theta[a] > theta[d] > theta[c] > 0
    assert info["n_dropped"] == 0 and info["n_reads"] >= 190
    assert info["n_reads"] - info["n_cands"] * 2.0 ** -32 <= expected.sum() <= info["n_reads"]
    ab.close()


# ---------------------------------------------------------------- 8. files
def test_the_aligner_loop_leaves_abundance_csv_and_changes_nothing_else(capi, world, corpus, tmp_path, monkeypatch):
    from monica_amd import aligner, mappy_compat
    dbs = tmp_path / "databases"
    dbs.mkdir()
    synth.write_fasta(str(dbs / "database0.fna.gz"), world.names, world.seqs)
    paths = aligner.indexer(str(dbs), str(tmp_path / "indexes"))
    al = mappy_compat.Aligner(fn_idx_in=paths[0])
    assert al and al.index.contig_lens == [len(s) for s in world.seqs] and list(al.index.contig_genome) == world.cg
    ab = al.abundance(cap_cands=4096)
    out = al.map_batch(corpus["bases"], corpus["offsets"], MIN_MAPQ, abundance=ab)
    assert len(out) == 5
    check_collection(ab, corpus["unique"], corpus["rows"], corpus["n_reads"])
    theta, expected, _ = ab.solve()
    unique = ab.unique()
    ab.close()
    n = len(corpus["reads"])
    monkeypatch.setattr(aligner, "BATCH_READS", 60)
    monkeypatch.setattr(aligner, "BATCH_RAMP", (1.0,))
    monkeypatch.setattr(aligner, "PIPE_TRACE", [])
    listing, pkl = {}, {}
    for label, kw in (("plain", {}), ("abundance", dict(abundance=True))):
        query, outdir = tmp_path / f"query {label}", tmp_path / f"output {label}"
        query.mkdir(), outdir.mkdir()
        synth.write_fastq(str(query / "s.fastq"), corpus["bases"], corpus["offsets"], ids=[f"r{i}" for i in range(n)])
        cwd = os.getcwd()
        try:
            aligner.multi_threaded_aligner(str(query), paths, mode="basic", mapping_quality=MIN_MAPQ, n_threads=1, output_folder=str(outdir), **kw)
        finally:
            os.chdir(cwd)
        listing[label] = {os.path.relpath(os.path.join(d, f), query): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(query) for f in fs}
        pkl[label] = (outdir / "alignment.pkl").read_bytes()
    assert sum(1 for t in aligner.PIPE_TRACE if t[0] == "classify") >= 4, "one batch only"
    csv = os.path.join("mapped", "s.abundance.csv")
    assert csv not in listing["plain"] and sorted(listing["abundance"]) == sorted(list(listing["plain"]) + [csv])
    for name, data in listing["plain"].items():                   # abundance= changes no routed file
        assert listing["abundance"][name] == data, name
    assert any(name.endswith("fastq") and data for name, data in listing["plain"].items())
    assert pkl["plain"] == pkl["abundance"] and pickle.loads(pkl["plain"])
    lines = listing["abundance"][csv].decode().splitlines()
    assert lines[0] == "genome,theta,expected_reads,unique_reads" and len(lines) == 1 + world.G
    for g, line in enumerate(lines[1:]):
        name, t, e, u = line.split(",")
        assert name == al.index.genome_names[g] and float(t) == theta[g] and float(e) == expected[g] and int(u) == unique[g]
