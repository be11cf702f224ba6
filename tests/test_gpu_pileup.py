"""Per-base pileup accumulated on the device (mnc_pileup_*, mnc_engine_add_pileup; csrc/k_pileup.hip).

Reference: tests/pileref.py -- the contract in plain numpy -- applied to the CPU ORACLE's regions and CIGARs
(oracle.Index.map_cigar) with the oracle's own gate and covref's selectors.  Nothing is compared against the engine's
export or dumps.  One test has an answer that does not come from the oracle either: planted variants."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import covref
import pileref
import util
from monica_amd import synth
from test_gpu_alignments import mutate

pytestmark = pytest.mark.gpu

ACGT = util.ACGT
LENS = (60_001, 40_003, 50_000)          # test_gpu_coverage.py's world: no multiple of 64 or of the scan's tile (1 024)
REF_N = (20_100, 20_300, 20_501, 20_700, 21_100)      # contig 1: isolated N's in the reference, inside a covered stretch
MIN_MAPQ = 60
SELECTORS = (covref.GATED, covref.PRIMARY, covref.ALL, covref.ASSIGNED)
THRESHOLDS = ((2, 1, 500), (1, 1, 0))    # one of two, two of four: 500 permille exactly (the corpus fixture checks there are such)


class World:
    def __init__(self, capi, oracle):
        names, seqs = util.small_genomes(4, 70_000, 70_000)
        copy = synth.diverge(seqs[0], 0x77, 10_000)    # contig 2: a 1 % diverged copy of contig 0 (secondaries, low MAPQ)
        self.clean = [seqs[0][:LENS[0]].copy(), seqs[1][:LENS[1]].copy(), copy[:LENS[2]].copy()]   # what the reads are made of
        self.names, self.seqs = names[:3], [s.copy() for s in self.clean]
        self.seqs[1][list(REF_N)] = ord("N")
        self.capi = capi
        self.idx = capi.Index.from_seqs(self.names, self.seqs)
        self.oidx = oracle.Index.from_seqs(self.names, [s.tobytes() for s in self.seqs])
        self.oidx.opt.cigar = 1
        self.eng = capi.Engine(self.idx, 0)
        self._want = {}

    def oracle_dp(self, reads):
        return [self.oidx.map_cigar(np.asarray(rd, dtype=np.uint8).tobytes()) for rd in reads]

    def want(self, key, per_read, reads, what, min_mapq=MIN_MAPQ):
        """pileref's planes for one selector over the oracle's records, computed once and never written to."""
        k = (key, what, min_mapq)
        if k not in self._want:
            planes = pileref.tally(pileref.records_of(per_read, [np.asarray(r, dtype=np.uint8).tobytes() for r in reads], what, min_mapq), self.seqs)
            for p in planes:
                p.setflags(write=False)
            self._want[k] = planes
        return self._want[k]


def counts_of(pu):
    return [pu.counts(rid) for rid in range(len(LENS))]


def check(pu, want, scale=1):
    for rid, w in enumerate(want):
        got = pu.counts(rid)
        assert got.dtype == np.int32 and got.shape == w.shape
        for k, name in enumerate(pileref.PLANES):
            bad = np.flatnonzero(got[k] != w[k] * scale)
            assert not len(bad), f"contig {rid}, plane {name}: differs at {bad[:8]}: {got[k][bad[:8]]} != {(w[k] * scale)[bad[:8]]}"


def columns(rs, cigar):
    """(op, reference position, query column) of every M / D column and every I operation of a CIGAR."""
    t, q = int(rs), 0
    for length, op in cigar:
        if op == "I":
            yield op, t, q
            q += length
            continue
        for j in range(length):
            yield op, t + j, (q + j if op == "M" else -1)
        t += length
        q += length if op == "M" else 0


@pytest.fixture(scope="module")
def world(capi, oracle):
    return World(capi, oracle)


@pytest.fixture(scope="module")
def corpus(world):
    """test_gpu_coverage.py's corpus (~150 reads of 1.5-2 kb at 10 % errors from both strands, random reads, a read that
    ends on contig 0's last base, one that starts on contig 1's first, a 60-base deletion, a 60-base insertion, chimeras of
    two gated records) and, for the columns: error-free reads (one operation each, two of them over the reference N's)
    and a read with three N's.  The oracle's answer is computed once -- and checked to hold what the tests rely on."""
    rng = np.random.default_rng(0xC0FE)
    g = world.clean
    reads = []
    for i in range(132):
        s = g[i % 3]
        n = int(rng.integers(1500, 2001))
        at = int(rng.integers(0, len(s) - n))
        rd = mutate(rng, s[at:at + n])
        reads.append(util.revcomp(rd) if rng.integers(0, 2) else rd)
    for i in range(12):
        reads.insert(int(rng.integers(0, len(reads) + 1)), ACGT[rng.integers(0, 4, 1800)])
    g0, g1 = g[0], g[1]
    reads.append(g0[-1500:].copy())                                            # ends on the last base of contig 0
    reads.append(g1[:1500].copy())                                             # starts on the first base of contig 1
    reads.append(np.concatenate([g1[20_000:20_900], g1[20_960:21_800]]))       # a 60-base deletion (over four of the reference N's)
    reads.append(np.concatenate([g1[30_000:30_900], ACGT[rng.integers(0, 4, 60)], g1[30_900:31_800]]))   # a 60-base insertion
    for i in range(4):                                                          # chimeras: two gated primaries
        reads.append(np.concatenate([mutate(rng, g1[2_000 + 3_000 * i:2_900 + 3_000 * i]), mutate(rng, g0[52_000 + 1_000 * i:53_200 + 1_000 * i])]))
    reads.append(g0[5_000:6_500].copy())                                       # error-free: a single operation
    reads.append(util.revcomp(g1[8_000:9_500]))
    reads.append(g1[20_050:21_500].copy())                                     # error-free but for the reference's own N's
    reads.append(util.revcomp(g1[19_900:21_300]))
    with_n = g0[10_000:11_800].copy()
    n_at = (500, 900, 1300)
    with_n[list(n_at)] = ord("N")
    reads.append(with_n)
    i_with_n = len(reads) - 1
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    i_with_n = int(np.flatnonzero(order == i_with_n)[0])
    bases, offsets = util.pack_reads(reads)
    ref = world.oracle_dp(reads)
    # ---- what keeps the tests honest, on the oracle's output
    regs = np.concatenate([r for r, _ in ref])
    cigars = [c for _, cigs in ref for c in cigs]
    ops = [(l, op) for c in cigars for l, op in c]
    assert max(len(c) for c in cigars) > 192, "CIGARs of several 64-operation chunks"
    assert sum(len(c) == 1 for c in cigars) >= 2, "error-free reads: a single operation"
    at_end = [x for x in regs if x["re"] == LENS[x["rid"]] and x["rid"] + 1 < len(LENS)]
    assert at_end, "no record that ends on its contig's last base"
    assert any(x["rid"] == at_end[0]["rid"] + 1 and x["rs"] == 0 for x in regs), "the next contig's base 0 is not covered"
    assert sum(len(r) > 1 for r, _ in ref) >= 3, "reads with secondaries"
    assert (regs["rev"] == 1).sum() >= 20 and (regs["rev"] == 0).sum() >= 20
    assert any(op == "D" and l >= 50 for l, op in ops) and any(op == "I" and l >= 50 for l, op in ops)
    assert sum(len(r) == 0 for r, _ in ref) >= 10, "reads without any record"
    primary = regs["id"] == regs["parent"]
    assert (primary & (regs["mapq"] >= MIN_MAPQ)).any() and (primary & (regs["mapq"] < MIN_MAPQ)).any() and (~primary).any()
    n_gated = [int(((r["id"] == r["parent"]) & (r["mapq"] >= MIN_MAPQ)).sum()) for r, _ in ref]
    assert sum(n > 1 for n in n_gated) >= 2, "reads with more than one gated record (ASSIGNED must differ from GATED)"
    over_n = sum(1 for r, cigs in ref for x, c in zip(r, cigs) if x["rid"] == 1 for op, t, _ in columns(x["rs"], c) if op == "M" and t in REF_N)
    assert over_n >= 8, "M columns over a reference N"
    r, cigs = ref[i_with_n]
    assert len(r) >= 1 and r[0]["rev"] == 0
    q_in_m = {r[0]["qs"] + q for op, _, q in columns(r[0]["rs"], cigs[0]) if op == "M"}
    assert all(p in q_in_m for p in n_at), "a query N inside an M operation"
    # the planes themselves: every kind of column is there, and a threshold of THRESHOLDS[0] is met with equality
    planes = world.want("corpus", ref, reads, covref.ALL)
    for k in range(len(pileref.PLANES)):
        assert sum(int(p[k].sum()) for p in planes) > 0, pileref.PLANES[k]
    span = np.concatenate([p[pileref.DEPTH] + p[pileref.DEL] for p in planes])
    alts = np.concatenate([p[[pileref.A, pileref.C, pileref.G, pileref.T, pileref.DEL, pileref.INS]] for p in planes], axis=1)
    d, c, pm = THRESHOLDS[0]
    assert ((span >= d) & (alts >= c) & (alts * 1000 == pm * span)).any(), "no count at exactly min_permille"
    return dict(reads=reads, bases=bases, offsets=offsets, ref=ref)


def raw_add(capi, eng, pu, what):
    return capi.lib().mnc_engine_add_pileup(eng._h, pu._h, what)


# ---------------------------------------------------------------- 1. counts
def test_counts_of_every_selector_equal_the_reference(capi, world, corpus):
    world.eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    pu = capi.Pileup(world.idx, 0)
    cov = capi.Coverage(world.idx, 0, 1024)
    assert 32 * sum(LENS) <= pu.device_bytes() < 32 * sum(LENS) + (1 << 16)
    d_depth, d_alt, words = pu.device()
    assert d_depth and d_alt and words == sum(LENS)
    sums = set()
    for sel in SELECTORS:
        pu.reset(), cov.reset()
        world.eng.add_pileup(pu, sel)
        world.eng.add_coverage(cov, sel)
        want = world.want("corpus", corpus["ref"], corpus["reads"], sel)
        check(pu, want)
        for rid in range(len(LENS)):
            assert np.array_equal(pu.counts(rid)[0], cov.depth(rid)), "the depth plane is coverage's depth of the same add"
        sums.add(tuple(int(sum(p[k].sum() for p in want)) for k in range(8)))
    assert len(sums) == 4                                         # four selectors, four different answers
    # a sub-interval whose ends are no multiple of 64 or of the scan's tile, and an empty one
    want = world.want("corpus", corpus["ref"], corpus["reads"], SELECTORS[-1])
    assert np.array_equal(pu.counts(1, 19_999, 21_847), want[1][:, 19_999:21_847])
    assert np.array_equal(pu.counts(0, LENS[0] - 1, LENS[0]), want[0][:, -1:])
    assert pu.counts(2, 77, 77).shape == (8, 0)
    pu.close(), cov.close()


# ---------------------------------------------------------------- 2. accumulation and reset
def test_accumulation_split_batches_and_reset(capi, world, corpus):
    off = corpus["offsets"]
    n = len(corpus["reads"])
    cut = n // 2 | 1                                              # an odd read
    what = capi.COV_ALL
    want = world.want("corpus", corpus["ref"], corpus["reads"], what)
    pu = capi.Pileup(world.idx, 0)
    world.eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    for _ in range(3):
        world.eng.add_pileup(pu, what)
    check(pu, want, scale=3)
    check(pu, want, scale=3)                                      # reading does not change it
    pu.reset()
    assert not any(c.any() for c in counts_of(pu))
    assert len(pu.variants(-1, 0, 1, 0)) == 0 and set(pu.consensus(1, 0, 3000, 1)) == set(b"N")
    world.eng.classify(corpus["bases"][:off[cut]], off[:cut + 1], MIN_MAPQ)
    world.eng.add_pileup(pu, what)
    world.eng.classify(corpus["bases"][off[cut]:], off[cut:] - off[cut], MIN_MAPQ)
    world.eng.add_pileup(pu, what)
    check(pu, want)
    pu.close()


# ---------------------------------------------------------------- 3. two engines on threads
def test_two_engines_on_threads_add_into_one_pileup(capi, world, corpus):
    off = corpus["offsets"]
    cut = len(corpus["reads"]) // 2
    pu = capi.Pileup(world.idx, 0)
    halves = [(corpus["bases"][:off[cut]], off[:cut + 1]), (corpus["bases"][off[cut]:], off[cut:] - off[cut])]
    errors = []

    def work(bases, offsets):
        try:
            eng = capi.Engine(world.idx, 0)
            eng.classify(bases, offsets, MIN_MAPQ)
            eng.add_pileup(pu, capi.COV_GATED)
            eng.sync()
            eng.close()
        except Exception as err:                                  # noqa: BLE001 -- reported below, on the main thread
            errors.append(err)

    threads = [threading.Thread(target=work, args=h) for h in halves]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    check(pu, world.want("corpus", corpus["ref"], corpus["reads"], capi.COV_GATED))
    pu.close()


# ---------------------------------------------------------------- 3b. the walk shared with the coverage accumulator
def test_a_cigar_longer_than_two_chunks(capi, world):
    """test_gpu_coverage.py's reads of the same name: the run carried across a chunk border, together with the query and
    reference offsets carried beside it."""
    rng = np.random.default_rng(66)
    g = world.clean[1]
    reads = [mutate(rng, g[5_000:11_000], sub=0.04, ins=0.04, dele=0.04), util.revcomp(mutate(rng, g[30_000:36_000], sub=0.04, ins=0.04, dele=0.04))]
    ref = world.oracle_dp(reads)
    assert all(len(r) >= 1 for r, _ in ref) and all(len(c[0]) > 128 for _, c in ref), "CIGARs of more than 128 operations"
    world.eng.classify(*util.pack_reads(reads), 0)
    pu = capi.Pileup(world.idx, 0)
    world.eng.add_pileup(pu, capi.COV_ALL)
    check(pu, world.want("long cigar", ref, reads, capi.COV_ALL, 0))
    pu.close()


def test_coverage_and_pileup_of_the_same_adds_agree_on_depth(capi, world, corpus):
    n = 40
    off = corpus["offsets"][:n + 1]
    world.eng.classify(corpus["bases"][:off[-1]], off, MIN_MAPQ)
    pu, cov = capi.Pileup(world.idx, 0), capi.Coverage(world.idx, 0, 1024)
    for sel in SELECTORS:
        pu.reset(), cov.reset()
        world.eng.add_pileup(pu, sel)
        world.eng.add_coverage(cov, sel)
        total = 0
        for rid in range(len(LENS)):
            depth = cov.depth(rid)
            assert np.array_equal(depth, pu.counts(rid)[0]), f"selector {sel}, contig {rid}"
            total += int(depth.sum())
        assert total > 0, f"selector {sel}: nothing was added"
    pu.close(), cov.close()


# ---------------------------------------------------------------- 4. variants and consensus
def test_variants_and_consensus_equal_the_reference(capi, world, corpus):
    L = capi.lib()
    world.eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    pu = capi.Pileup(world.idx, 0)
    world.eng.add_pileup(pu, capi.COV_ALL)
    want = world.want("corpus", corpus["ref"], corpus["reads"], capi.COV_ALL)
    sizes = []
    for thr in THRESHOLDS:
        for rid in (-1, 0, 1, 2):
            w = pileref.variants(want, world.seqs, rid, *thr)
            got = pu.variants(rid, *thr)
            assert got.dtype == capi.VARIANT_DTYPE and got.tobytes() == w.tobytes(), f"variants of contig {rid} at {thr}: {len(got)} against {len(w)}"
            sizes.append(len(w))
        for rid, start, end in ((0, 0, LENS[0]), (1, 0, LENS[1]), (2, 0, LENS[2]), (1, 19_999, 21_847), (0, 1_023, 1_025), (0, LENS[0] - 1_500, LENS[0]),
                                (2, 31, 31)):
            assert pu.consensus(rid, start, end, thr[0]) == pileref.consensus(want, world.seqs, rid, start, end, thr[0]), (rid, start, end, thr)
    assert 0 < sizes[0] < sizes[4] and sizes[0] == sum(sizes[1:4]) and all(sizes)
    cons = pileref.consensus(want, world.seqs, 1, 0, LENS[1], 1)
    assert set(cons) == set(b"ACGT-N") and all(cons[p] in b"ACGT" for p in REF_N)    # a reference N does not make the consensus N
    # a short cap: the size, and nothing written
    thr = THRESHOLDS[0]
    n = C.c_int64(0)
    buf = np.zeros(sizes[0], dtype=capi.VARIANT_DTYPE)
    buf["rid"] = -7
    assert L.mnc_pileup_call_variants(pu._h, -1, *thr, buf.ctypes.data, sizes[0] - 1, C.byref(n)) == capi.ERR_RANGE
    assert n.value == sizes[0] and (buf["rid"] == -7).all()
    assert L.mnc_pileup_call_variants(pu._h, -1, *thr, None, 0, C.byref(n)) == capi.ERR_RANGE and n.value == sizes[0]
    assert L.mnc_pileup_call_variants(pu._h, -1, *thr, buf.ctypes.data, sizes[0], C.byref(n)) == capi.OK and n.value == sizes[0]
    assert buf.tobytes() == pileref.variants(want, world.seqs, -1, *thr).tobytes()
    for rid in (-2, 3):
        assert L.mnc_pileup_call_variants(pu._h, rid, *thr, buf.ctypes.data, len(buf), C.byref(n)) == capi.ERR_ARG
    for rid in (-1, 3):
        assert L.mnc_pileup_fetch_counts(pu._h, rid, 0, 1, buf.ctypes.data) == capi.ERR_ARG
        assert L.mnc_pileup_consensus(pu._h, rid, 0, 1, 1, buf.ctypes.data) == capi.ERR_ARG
    for start, end in ((-1, 5), (5, 4), (0, LENS[1] + 1)):
        assert L.mnc_pileup_fetch_counts(pu._h, 1, start, end, buf.ctypes.data) == capi.ERR_ARG
        assert L.mnc_pileup_consensus(pu._h, 1, start, end, 1, buf.ctypes.data) == capi.ERR_ARG
    pu.close()


# ---------------------------------------------------------------- 5. a known answer, independent of the oracle
def test_planted_variants_come_back(capi, world):
    g = world.clean[1]
    lo, hi = 33_000, 39_000                                       # the strain: this stretch of contig 1, edited
    rng = np.random.default_rng(0x51A)

    def unique_place(at, what):
        """The first position from `at` on where an indel cannot shift: a deletion of g[p:p+3], or the insertion of `what`
        in front of g[p], has one placement only."""
        for p in range(at, at + 200):
            if what is None and g[p - 1] != g[p + 2] and g[p] != g[p + 3] and len(set(g[p - 3:p + 6].tolist())) == 4:
                return p
            if what is not None and what[-1] != g[p - 1] and what[0] != g[p] and what[0] != g[p - 1] and what[-1] != g[p]:
                return p
        raise AssertionError("no such place")

    # reads start every 150 bases of the strain and are 1 500 long; the indels sit midway between two read borders
    del_at = unique_place(lo + 2_175, None)
    ins = np.frombuffer(b"GT" if g[lo + 3_375] not in b"GT" else b"CA", dtype=np.uint8)
    ins_at = unique_place(lo + 3_375, ins)                        # inserted in front of g[ins_at]
    subs = [lo + 1_610 + 131 * i for i in range(20)]
    assert all(abs(s - x) > 20 for s in subs for x in (del_at, ins_at)) and subs[-1] < lo + 4_200
    strain_ref = g.copy()                                         # the strain in reference coordinates: substitutions only
    for s in subs:
        strain_ref[s] = ACGT[(np.searchsorted(ACGT, g[s]) + 1 + int(rng.integers(0, 3))) % 4]
    strain = np.concatenate([strain_ref[lo:del_at], strain_ref[del_at + 3:ins_at], ins, strain_ref[ins_at:hi]])
    reads = []
    for i in range(30):
        rd = strain[150 * i:150 * i + 1_500].copy()
        reads.append(util.revcomp(rd) if i % 2 else rd)
    # the oracle puts the indels where they were planted
    ref = world.oracle_dp(reads)
    n_del = n_ins = 0
    for regs, cigs in ref:
        assert len(regs) == 1 and regs[0]["rid"] == 1
        t = int(regs[0]["rs"])
        for length, op in cigs[0]:
            if op == "D":
                assert (t, length) == (del_at, 3)
                n_del += 1
            if op == "I":
                assert (t, length) == (ins_at, 2)
                n_ins += 1
            t += length if op != "I" else 0
    assert n_del >= 5 and n_ins >= 5
    world.eng.classify(*util.pack_reads(reads), MIN_MAPQ)
    pu = capi.Pileup(world.idx, 0)
    world.eng.add_pileup(pu, capi.COV_GATED)
    v = pu.variants(1, 5, 5, 800)
    events = [(s, chr(g[s]), chr(strain_ref[s])) for s in subs] + [(del_at + j, chr(g[del_at + j]), "-") for j in range(3)] + [(ins_at - 1, chr(g[ins_at - 1]), "+")]
    assert [(int(x["pos"]), x["ref"].decode(), x["alt"].decode()) for x in v] == sorted(events)
    assert len(subs) + 1 + 1 == 22 and (v["count"] == v["span"]).all() and (v["rid"] == 1).all() and (v["span"] >= 5).all()
    assert np.array_equal(pu.variants(-1, 5, 5, 800), v)
    # the consensus of the covered stretch, deleted bases taken out, is the strain -- without the two inserted bases
    a, b = lo + 1_500, lo + 4_300
    cons = pu.consensus(1, a, b, 5)
    assert cons.count(b"-") == 3 and b"N" not in cons
    assert cons.replace(b"-", b"") == np.concatenate([strain_ref[a:del_at], strain_ref[del_at + 3:b]]).tobytes()
    pu.close()


# ---------------------------------------------------------------- 6. errors
def test_errors_leave_the_accumulator_untouched(capi, world, corpus, oracle):
    n = 40
    off = corpus["offsets"][:n + 1]
    pu = capi.Pileup(world.idx, 0)
    world.eng.classify(corpus["bases"][:off[-1]], off, MIN_MAPQ)
    world.eng.add_pileup(pu, capi.COV_ALL)
    before = counts_of(pu)
    assert sum(int(c.sum()) for c in before) > 0
    # the chain contract: no CIGAR
    chain = capi.Engine(world.idx, 0)
    chain.set_contract(capi.CONTRACT_CHAIN)
    chain.classify(corpus["bases"][:off[-1]], off, MIN_MAPQ)
    for sel in SELECTORS:
        assert raw_add(capi, chain, pu, sel) == capi.ERR_ARG
    chain.close()
    # a pileup of another index
    other_idx = capi.Index.from_seqs(world.names[:1], [world.seqs[1][:20_000]])
    other = capi.Pileup(other_idx, 0)
    assert raw_add(capi, world.eng, other, capi.COV_ALL) == capi.ERR_ARG
    assert not other.counts(0).any()
    # an add before any classify; no selector, two, SPAN, unknown bits
    fresh = capi.Engine(world.idx, 0)
    assert raw_add(capi, fresh, pu, capi.COV_ALL) == capi.ERR_ARG
    fresh.close()
    for what in (0, capi.COV_GATED | capi.COV_ALL, 15, capi.COV_ALL | capi.COV_SPAN, capi.COV_SPAN, 32, capi.COV_ALL | 64):
        assert raw_add(capi, world.eng, pu, what) == capi.ERR_ARG, what
    after = counts_of(pu)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    other.close(), pu.close()


def test_a_mixed_usual_and_wide_call_adds_nothing(capi):
    n = (1 << 20) + 5000
    g = synth.genome(0x5151, 1_100_000)
    idx = capi.Index.from_seqs([synth.contig_name(0)], [g])
    eng = capi.Engine(idx, 0)
    eng.set_long_reads(True)
    pu = capi.Pileup(idx, 0)
    short = g[500_000:502_000].copy()
    short[1000] = ACGT[(np.searchsorted(ACGT, short[1000]) + 1) % 4]
    assign, _, _ = eng.classify(*util.pack_reads([short]), MIN_MAPQ)
    assert assign.tolist() == [0]
    eng.add_pileup(pu, capi.COV_GATED)
    before = pu.counts(0, 499_000, 503_000)
    assert before[0].sum() == 2000 and before[1:5].sum() == 2000 and before[1:5, 1000 + 1000].sum() == 1
    assert [(int(x["pos"]), x["alt"]) for x in pu.variants(-1, 1, 1, 1000)] == [(501_000, bytes([short[1000]]))]
    assign, _, _ = eng.classify(*util.pack_reads([g[20_000:20_000 + n], short]), MIN_MAPQ)
    assert assign.tolist() == [0, 0]
    for what in (capi.COV_GATED, capi.COV_ALL):
        assert raw_add(capi, eng, pu, what) == capi.ERR_UNSUPPORTED
    assert np.array_equal(pu.counts(0, 499_000, 503_000), before) and not pu.counts(0, 20_000, 30_000).any()
    pu.close()
    eng.close()


# ---------------------------------------------------------------- 7. Python: map_batch(pileup=) and the aligner loop
def test_python_map_batch_and_the_aligner_loop(capi, world, corpus, tmp_path, monkeypatch):
    from monica_amd import aligner, mappy_compat
    dbs = tmp_path / "databases"
    dbs.mkdir()
    synth.write_fasta(str(dbs / "database0.fna.gz"), world.names, world.seqs)
    paths = aligner.indexer(str(dbs), str(tmp_path / "indexes"))
    want = world.want("corpus", corpus["ref"], corpus["reads"], capi.COV_GATED)
    al = mappy_compat.Aligner(fn_idx_in=paths[0])
    assert al and al.index.contig_lens == list(LENS)
    pu = al.pileup()
    out = al.map_batch(corpus["bases"], corpus["offsets"], MIN_MAPQ, pileup=pu)
    assert len(out) == 5 and (out[0] >= 0).sum() > 50
    check(pu, want)
    pu.reset()
    al.map_batch(corpus["bases"], corpus["offsets"], MIN_MAPQ, pileup=pu, pileup_what=capi.COV_ALL)
    check(pu, world.want("corpus", corpus["ref"], corpus["reads"], capi.COV_ALL))
    pu.close()
    # ---- the loop: several batches of one sample, variants.tsv beside the coverage CSV; without pileup= no such file
    n = len(corpus["reads"])
    monkeypatch.setattr(aligner, "BATCH_READS", 100)
    monkeypatch.setattr(aligner, "BATCH_RAMP", (1.0,))
    monkeypatch.setattr(aligner, "PIPE_TRACE", [])
    thr = THRESHOLDS[0]
    listing = {}
    for label, kw in (("plain", dict(coverage=1000)), ("pileup", dict(coverage=1000, pileup=thr)), ("pileup alone", dict(pileup=True))):
        query, outdir = tmp_path / f"query {label}", tmp_path / f"output {label}"
        query.mkdir(), outdir.mkdir()
        synth.write_fastq(str(query / "s.fastq"), corpus["bases"], corpus["offsets"], ids=[f"r{i}" for i in range(n)])
        cwd = os.getcwd()
        try:
            aligner.multi_threaded_aligner(str(query), paths, mode="basic", mapping_quality=MIN_MAPQ, n_threads=1, output_folder=str(outdir), **kw)
        finally:
            os.chdir(cwd)
        listing[label] = {os.path.relpath(os.path.join(d, f), query): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(query) for f in fs}
    assert sum(1 for t in aligner.PIPE_TRACE if t[0] == "classify") >= 6, "one batch only"
    tsv = os.path.join("mapped", "s.variants.tsv")
    assert tsv not in listing["plain"] and sorted(listing["pileup"]) == sorted(list(listing["plain"]) + [tsv])
    for name, data in listing["plain"].items():                   # pileup= changes no routed file and not the coverage CSV
        assert not name.endswith(("fastq", ".csv")) or listing["pileup"][name] == data, name
    assert any(name.endswith("fastq") for name in listing["plain"])
    assert sorted(listing["pileup alone"]) == sorted(set(listing["pileup"]) - {os.path.join("mapped", "s.coverage.csv")})
    assert listing["pileup"][tsv].decode() == pileref.variants_tsv(pileref.variants(want, world.seqs, -1, *thr), world.names, world.names)
    assert listing["pileup alone"][tsv].decode() == pileref.variants_tsv(pileref.variants(want, world.seqs, -1, *aligner.PILEUP_THRESHOLDS), world.names, world.names)
