"""Insertion alleles of the pileup on the device (include/monica_amd.h, "insertion alleles"; csrc/pile_ins.h).  Reference:
tests/insref.py on exact rows (test 1) and on the CPU ORACLE's regions and CIGARs with pileref's planes (tests 2 to 5); the
planted insertions of test 4 have an answer that does not come from the oracle."""
import ctypes as C
import threading

import numpy as np
import pytest

import covref
import insref
import pileref
import util
from test_gpu_alignments import mutate
from test_gpu_pileup import LENS, MIN_MAPQ, SELECTORS, World, check

pytestmark = pytest.mark.gpu

ACGT = util.ACGT
SHAPES = (1, 31, 32, 33, 63, 64, 65, 129, 200)       # the short / long border (32) and the borders of the wave's 64-base steps
PLANTED = ((33, 24_000), (64, 27_000), (130, 30_000), (10, 33_000))     # (bases, about where on contig 1); the last has an N inside
ROOM = (1 << 15, 1 << 16)                         # alleles, pool bases: more than any corpus below holds


@pytest.fixture(scope="module")
def world(capi, oracle):
    return World(capi, oracle)


def fetch(pu, rid=-1, thr=(0, 1, 0)):
    rec, bases = pu.insertions(rid, *thr)
    return rec.tobytes(), bases


def same(got, want):
    rec, bases = want
    assert got[1] == bases and got[0] == rec.tobytes(), f"{len(got[1])} alleles against {len(bases)}"


# ---------------------------------------------------------------- 1. exact shapes through add_insertion_list
@pytest.mark.parametrize("n_at", (None, 0, -1), ids=("acgt", "n-first", "n-last"))
def test_exact_shapes_through_the_list(capi, world, n_at):
    rng = np.random.default_rng(7)
    places = ((0, 0), (0, LENS[0] - 1), (2, LENS[2] - 1), (1, 777))           # first and last bases of contigs among them
    rows = []                                                                # (rid, pos, count, bases)
    for n in SHAPES:
        for k, (rid, pos) in enumerate(places):
            a = ACGT[rng.integers(0, 4, n)].copy()
            if n_at is not None:
                a[n_at] = ord("N")
            rows.append((rid, pos, 1 + k, a.tobytes()))
    twice = [(rid, pos, 2, a) for rid, pos, _, a in rows]                    # every allele in a second row of the same call
    sibling = [(rid, pos, 5, a[:-1] + (b"A" if a[-1:] != b"A" else b"C")) for rid, pos, _, a in rows[::4]]   # differs in the last base only
    again = [(rid, pos, 3, a) for rid, pos, _, a in rows[:9]]                # ... and in a second call
    calls = (rows + twice, sibling + again)
    assert len(calls[0]) > 64 and len({len(a) for *_, a in sibling}) == len(SHAPES)
    want = insref.Counter()
    pu = capi.Pileup(world.idx, 0, insertions=ROOM)
    for call in calls:
        pu.add_insertions(*(list(x) for x in zip(*call)))
        for rid, pos, count, a in call:
            want[(rid, pos, insref.codes(a))] += count
    empty = [np.zeros((8, n), dtype=np.int64) for n in LENS]                 # nothing was aligned: every span is 0
    same(fetch(pu), insref.call(want, empty, world.seqs, -1, 0, 1, 0))
    same(fetch(pu, 2), insref.call(want, empty, world.seqs, 2, 0, 1, 0))
    same(fetch(pu, -1, (0, 4, 0)), insref.call(want, empty, world.seqs, -1, 0, 4, 0))
    pooled = [a for (_, _, a) in want if len(a) > 32 or 4 in a]
    assert pu.insertion_info() == dict(n_alleles=len(want), n_events=sum(want.values()), n_dropped=0, n_pool_bases=sum(len(a) + len(a) % 2 for a in pooled),
                                       n_pool_dropped=0, n_collisions=0)
    assert not any(pu.counts(rid).any() for rid in range(3)), "the list touches no plane"
    before = fetch(pu)                                                      # bad rows leave it untouched
    for bad in ((3, 0, 1, b"A"), (0, LENS[0], 1, b"A"), (0, -1, 1, b"A"), (0, 5, 0, b"A"), (0, 5, 1, b"")):
        with pytest.raises(capi.MncError, match="row 0"):
            pu.add_insertions(*([x] for x in bad))
    assert fetch(pu) == before
    assert capi.lib().mnc_pileup_store_insertions(pu._h, 10, 10) == capi.ERR_ARG      # a second call, and after an add
    pu.close()


# ---------------------------------------------------------------- the corpus of tests 2 to 5
@pytest.fixture(scope="module")
def corpus(world):
    """~150 reads of 1.5-2 kb at 10 % errors from both strands, and for each of PLANTED six error-free reads over one
    place of contig 1, forward and reverse-complemented in turn, four of which carry the insertion."""
    rng = np.random.default_rng(0x1A5)
    g = world.clean
    reads = []
    for i in range(150):
        s = g[i % 3]
        n = int(rng.integers(1500, 2001))
        at = int(rng.integers(0, len(s) - n))
        rd = mutate(rng, s[at:at + n])
        reads.append(util.revcomp(rd) if rng.integers(0, 2) else rd)
    g1, planted, plant_reads = g[1], [], []
    for n, about in PLANTED:
        ins = ACGT[rng.integers(0, 4, n)].copy()
        p = next(p for p in range(about, about + 200) if len({ins[0], ins[-1]} & {g1[p - 1], g1[p]}) == 0)   # one placement only
        if n == 10:
            ins[4] = ord("N")
        planted.append((p - 1, ins.tobytes()))
        for k in range(6):
            lo = p - 400 - 120 * k
            rd = np.concatenate([g1[lo:p], ins, g1[p:lo + 1500]]) if k not in (1, 4) else g1[lo:lo + 1500].copy()
            plant_reads.append(util.revcomp(rd) if k % 2 else rd)
    reads += plant_reads
    ref = world.oracle_dp(reads)
    ref_planted = ref[len(reads) - len(plant_reads):]
    # ---- what keeps the tests honest, on the oracle's output
    recs = [(x, c) for r, cigs in ref for x, c in zip(r, cigs)]
    assert any(op == "I" and k >= 64 for _, c in recs for k, (_, op) in enumerate(c)), "no I at a CIGAR operation index of 64 or more"
    assert any(op == "I" for x, c in recs if x["rev"] for _, op in c), "no I in a reverse-strand record"
    alleles = insref.tally(pileref.records_of(ref, [r.tobytes() for r in reads], covref.ALL, MIN_MAPQ), world.seqs)
    assert len({(rid, pos) for rid, pos, _ in alleles}) < len(alleles), "no place with two different alleles"
    for pos, ins in planted:
        assert alleles[(1, pos, insref.codes(ins))] >= 4, f"the oracle places the {len(ins)}-base insertion elsewhere"
    bases, offsets = util.pack_reads(reads)
    return dict(reads=reads, bases=bases, offsets=offsets, ref=ref, planted=planted, plant_reads=plant_reads, ref_planted=ref_planted)


def want_of(world, corpus, what, key="corpus"):
    """(insref's alleles, pileref's planes) of the corpus -- or of its planted reads alone -- for one selector."""
    reads, ref = (corpus["reads"], corpus["ref"]) if key == "corpus" else (corpus["plant_reads"], corpus["ref_planted"])
    k = ("ins " + key, what)
    if k not in world._want:
        world._want[k] = insref.tally(pileref.records_of(ref, [r.tobytes() for r in reads], what, MIN_MAPQ), world.seqs)
    return world._want[k], world.want("ins " + key, ref, reads, what)


# ---------------------------------------------------------------- 2. through the engine
@pytest.mark.parametrize("sel", SELECTORS)
def test_alleles_of_every_selector_equal_the_reference(capi, world, corpus, sel):
    world.eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    pu, plain = capi.Pileup(world.idx, 0, insertions=ROOM), capi.Pileup(world.idx, 0)
    world.eng.add_pileup(pu, sel)
    world.eng.add_pileup(plain, sel)
    alleles, planes = want_of(world, corpus, sel)
    assert 300 < len(alleles) <= ROOM[0]
    for thr in ((0, 1, 0), (2, 2, 500)):
        same(fetch(pu, -1, thr), insref.call(alleles, planes, world.seqs, -1, *thr))
    same(fetch(pu, 1), insref.call(alleles, planes, world.seqs, 1, 0, 1, 0))
    check(pu, planes)
    rec, _ = pu.insertions()
    for rid in range(3):
        got, ins = pu.counts(rid), np.zeros(LENS[rid], dtype=np.int64)
        assert np.array_equal(got, plain.counts(rid)), "the store changes no plane"
        np.add.at(ins, rec["pos"][rec["rid"] == rid], rec["count"][rec["rid"] == rid])
        assert np.array_equal(ins, got[pileref.INS]), "the alleles of a place sum to its INS count"
    info = pu.insertion_info()
    assert (info["n_alleles"], info["n_events"], info["n_dropped"], info["n_pool_dropped"], info["n_collisions"]) == (len(alleles), sum(alleles.values()), 0, 0, 0)
    pu.close(), plain.close()


# ---------------------------------------------------------------- 3. order and cut independence
def test_order_and_cuts_do_not_show(capi, world, corpus):
    off, n = corpus["offsets"], len(corpus["reads"])

    def add(pu, eng, a, b):
        eng.classify(corpus["bases"][off[a]:off[b]], off[a:b + 1] - off[a], MIN_MAPQ)
        eng.add_pileup(pu, capi.COV_ALL)
        eng.sync()

    def on_threads(pu):
        errors = []

        def work(a, b):
            try:
                eng = capi.Engine(world.idx, 0)
                add(pu, eng, a, b)
                eng.close()
            except Exception as err:                              # noqa: BLE001 -- reported below, on the main thread
                errors.append(err)

        ts = [threading.Thread(target=work, args=c) for c in ((0, n // 2), (n // 2, n))]
        [t.start() for t in ts], [t.join() for t in ts]
        assert not errors, errors

    got = []
    for plan in (lambda pu: add(pu, world.eng, 0, n), lambda pu: [add(pu, world.eng, a, b) for a, b in ((101, n), (0, 37), (37, 101))], on_threads):
        pu = capi.Pileup(world.idx, 0, insertions=ROOM)
        plan(pu)
        got.append((fetch(pu), fetch(pu, -1, (2, 2, 500)), [pu.consensus(rid, 0, None, 2, insertions=True) for rid in range(3)]))
        assert pu.insertion_info()["n_collisions"] == 0
        pu.close()
    assert got[0] == got[1] == got[2] and len(got[0][0][1]) > 300


# ---------------------------------------------------------------- 4. consensus
def test_consensus_with_insertions(capi, world, corpus):
    g1 = world.clean[1]
    for key, reads in (("corpus", corpus["reads"]), ("planted", corpus["plant_reads"])):
        world.eng.classify(*util.pack_reads(reads), MIN_MAPQ)
        pu = capi.Pileup(world.idx, 0, insertions=ROOM)
        world.eng.add_pileup(pu, capi.COV_ALL)
        alleles, planes = want_of(world, corpus, capi.COV_ALL, key)
        for rid, start, end, depth in ((0, 0, LENS[0], 1), (1, 0, LENS[1], 2), (2, 1_023, 3_100, 1), (1, 23_000, 34_000, 3), (2, 31, 31, 1)):
            got = pu.consensus(rid, start, end, depth, insertions=True)
            assert got == insref.consensus(alleles, planes, world.seqs, rid, start, end, depth), (key, rid, start, end, depth)
            assert bytes(c for c in got if not 97 <= c <= 122) == pu.consensus(rid, start, end, depth)
        if key == "planted":                                       # four of six reads say so: known without the oracle
            cons = pu.consensus(1, 23_000, 34_000, 3, insertions=True)
            for pos, ins in corpus["planted"]:
                assert bytes([g1[pos]]) + ins.lower() + bytes([g1[pos + 1]]) in cons, f"the {len(ins)}-base insertion behind base {pos}"
            assert sum(97 <= c <= 122 for c in cons) == sum(len(ins) for _, ins in corpus["planted"])
        assert pu.insertion_info()["n_collisions"] == 0
        pu.close()


# ---------------------------------------------------------------- 5. limits
def test_limits_and_reset(capi, world, corpus):
    L = capi.lib()
    world.eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    alleles, planes = want_of(world, corpus, capi.COV_ALL)
    long_need = sum(len(a) + len(a) % 2 for (_, _, a) in alleles if len(a) > 32 or 4 in a)
    assert len(alleles) > 300 and long_need > 64 + 130
    # fewer slots than alleles: events are dropped, the read-outs refuse, the planes are right
    pu = capi.Pileup(world.idx, 0, insertions=(200, 1 << 16))
    world.eng.add_pileup(pu, capi.COV_ALL)
    info = pu.insertion_info()
    assert info["n_dropped"] > 0 and info["n_alleles"] < len(alleles) and info["n_events"] + info["n_dropped"] == sum(alleles.values()) and info["n_collisions"] == 0
    n, m = C.c_int64(0), C.c_int64(0)
    assert L.mnc_pileup_call_insertions(pu._h, -1, 0, 1, 0, None, 0, C.byref(n), None, 0, C.byref(m)) == capi.ERR_RANGE
    with pytest.raises(capi.MncError) as err:
        pu.consensus(1, 0, 1000, 1, insertions=True)
    assert err.value.code == capi.ERR_RANGE
    check(pu, planes)
    pu.close()
    # a pool too small for the long alleles; reset clears it, and a fresh add of reads it has room for reads out clean
    pu = capi.Pileup(world.idx, 0, insertions=(ROOM[0], 64))
    world.eng.add_pileup(pu, capi.COV_ALL)
    info = pu.insertion_info()
    assert info["n_pool_dropped"] > 0 and info["n_dropped"] == 0 and info["n_alleles"] == len(alleles) and info["n_events"] == sum(alleles.values())
    with pytest.raises(capi.MncError) as err:
        pu.insertions()
    assert err.value.code == capi.ERR_RANGE
    pu.reset()
    assert set(pu.insertion_info().values()) == {0} and len(pu.insertions()[0]) == 0
    sub = corpus["plant_reads"][:6]                                # the 33-base insertion alone: 34 pool places
    world.eng.classify(*util.pack_reads(sub), MIN_MAPQ)
    world.eng.add_pileup(pu, capi.COV_ALL)
    want = insref.tally(pileref.records_of(corpus["ref_planted"][:6], [r.tobytes() for r in sub], capi.COV_ALL, MIN_MAPQ), world.seqs)
    assert sum(len(a) + len(a) % 2 for (_, _, a) in want if len(a) > 32 or 4 in a) == 34
    same(fetch(pu), insref.call(want, pileref.tally(pileref.records_of(corpus["ref_planted"][:6], [r.tobytes() for r in sub], capi.COV_ALL, MIN_MAPQ), world.seqs),
                                world.seqs, -1, 0, 1, 0))
    assert pu.insertion_info()["n_pool_dropped"] == 0
    pu.close()
