"""The strand store of the pileup (mnc_pileup_store_strands, mnc_engine_add_pileup_quals, the read-outs by strand;
csrc/k_pile_strand.hip) against tests/strandref.py -- the contract in plain numpy -- over the CPU ORACLE's regions and CIGARs.
Every comparison is of integers, for equality.  One test has an answer that does not come from the oracle: planted SNVs."""
import numpy as np
import pytest

import covref
import strandref
import util
from test_gpu_alignments import mutate

pytestmark = pytest.mark.gpu

LENS = (30_001, 20_003, 25_000)          # no multiple of 64 or of the scan's tile (1 024)
REF_N = (10_100, 10_300, 10_501)         # contig 1: N's in the reference, inside a covered stretch
MIN_MAPQ = 60
# ((min_depth, min_count, min_permille), (per strand: count, permille)).  The corpus is about five deep, two or three a
# strand: one observation of two or three is 500 or 333 permille, so 400 cuts between them; (1, 0) is "seen on both strands"
THRESHOLDS = (((2, 2, 250), (1, 400)), ((1, 1, 0), (1, 0)))


class World:
    def __init__(self, capi, oracle):
        names, seqs = util.small_genomes(3, 31_000, 31_000)
        self.clean = [s[:n].copy() for s, n in zip(seqs, LENS)]
        self.names, self.seqs = names, [s.copy() for s in self.clean]
        self.seqs[1][list(REF_N)] = ord("N")
        self.idx = capi.Index.from_seqs(self.names, self.seqs)
        self.oidx = oracle.Index.from_seqs(self.names, [s.tobytes() for s in self.seqs])
        self.oidx.opt.cigar = 1
        self.eng = capi.Engine(self.idx, 0)
        self._want = {}

    def want(self, corpus, what, min_qual):
        if (what, min_qual) not in self._want:
            planes = strandref.tally(corpus["ref"], corpus["reads"], corpus["quals"], what, MIN_MAPQ, self.seqs, min_qual)
            self._want[what, min_qual] = [p.setflags(write=False) or p for p in planes]
        return self._want[what, min_qual]

    def classify(self, corpus, lo=0, hi=None):
        off = corpus["offsets"]                                 # reads [lo, hi) as the engine's batch; returns their qualities
        hi = len(off) - 1 if hi is None else hi
        self.eng.classify(corpus["bases"][off[lo]:off[hi]], off[lo:hi + 1] - off[lo], MIN_MAPQ)
        return corpus["qual_bytes"][off[lo]:off[hi]]


@pytest.fixture(scope="module")
def world(capi, oracle):
    return World(capi, oracle)


@pytest.fixture(scope="module")
def corpus(world):
    """60 reads of 1.5-2 kb at 10 % errors from both strands, over 8 kb of each contig (errors of different reads meet at a
    base: variants on both strands); a read that ends on contig 0's last base, one over the reference N's, one of all Q0, one
    of all Q40.  Qualities: seeded random Phred 0 .. 40 per base -- asymmetric, so a reversed index on a reverse record shows."""
    rng = np.random.default_rng(0x57A4D)
    g, reads = world.clean, []
    for i in range(60):
        at = (0, 6_000, 0)[i % 3] + int(rng.integers(0, 6_000))        # contig 1: around the reference N's
        rd = mutate(rng, g[i % 3][at:at + int(rng.integers(1500, 2001))])
        reads.append(util.revcomp(rd) if i % 4 >= 2 else rd)
    reads += [g[0][-1500:].copy(), util.revcomp(mutate(rng, g[1][10_000:11_600]))]
    quals = [(33 + rng.integers(0, 41, len(r))).astype(np.uint8) for r in reads]
    quals[4][:], quals[7][:] = 33, 33 + 40                        # a forward read of all Q0, a reverse read of all Q40
    bases, offsets = util.pack_reads(reads)
    ref = [world.oidx.map_cigar(np.asarray(r, dtype=np.uint8).tobytes()) for r in reads]
    regs, cigars = np.concatenate([r for r, _ in ref]), [c for _, cigs in ref for c in cigs]
    assert max(len(c) for c in cigars) > 128 and max(l for c in cigars for l, op in c if op == "M") > 64
    assert (regs["rev"] == 1).sum() >= 15 and (regs["rev"] == 0).sum() >= 15 and len(ref[4][0]) and len(ref[7][0])
    assert any(x["re"] == LENS[0] and x["rid"] == 0 for x in regs), "no record that ends on contig 0's last base"
    assert any(x["rid"] == 1 and x["rs"] < REF_N[0] and x["re"] > REF_N[-1] for x in regs), "no record over the reference N's"
    return dict(reads=reads, quals=quals, bases=bases, offsets=offsets, qual_bytes=np.concatenate(quals), ref=ref)


def check(got, want, what):
    for rid, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and g.shape == w.shape, what
        bad = np.argwhere(g != w)[:8]
        assert not len(bad), f"{what}: contig {rid} differs at (plane, base) {bad.tolist()}: {g[tuple(bad.T)]} != {w[tuple(bad.T)]}"


def strand_counts(pu):
    return [pu.strand_counts(rid) for rid in range(len(LENS))]


@pytest.mark.parametrize("ins", (False, True), ids=("planes", "with insertion store"))
@pytest.mark.parametrize("min_qual", (0, 12, 41))
@pytest.mark.parametrize("sel", (covref.GATED, covref.ALL))
def test_planes_by_strand_equal_the_reference(capi, world, corpus, sel, min_qual, ins):
    q = world.classify(corpus)
    pu = capi.Pileup(world.idx, 0, insertions=(1 << 14, 1 << 16) if ins else None, strands=min_qual)
    assert 72 * sum(LENS) <= pu.device_bytes() and all(pu.strands_device())
    world.eng.add_pileup(pu, sel, quals=None if min_qual == 0 and not ins else q)    # without a mask either add serves
    want = world.want(corpus, sel, min_qual)
    check(strand_counts(pu), want, "strand_counts")
    check([pu.counts(rid) for rid in range(len(LENS))], [w[:8] for w in want], "counts")
    masked, depth = (sum(int(w[k].sum()) for w in want) for k in (strandref.LOWQ, 0))
    assert (masked == 0) if min_qual == 0 else (masked > 0 and (depth == 0) == (min_qual == 41))    # nothing, some, every M column
    assert np.array_equal(pu.strand_counts(1, 9_999, 11_847), want[1][:, 9_999:11_847]) and pu.strand_counts(2, 77, 77).shape == (18, 0)
    if min_qual == 0:                                             # bit for bit a plain pileup's
        plain = capi.Pileup(world.idx, 0)
        world.eng.add_pileup(plain, sel)
        assert all(np.array_equal(pu.counts(rid), plain.counts(rid)) for rid in range(len(LENS)))
        assert pu.variants(-1, 2, 1, 500).tobytes() == plain.variants(-1, 2, 1, 500).tobytes()
        plain.close()
    if ins:                                                       # the allele table is strand-less and unmasked
        assert pu.insertion_info()["n_events"] == sum(int(w[7].sum()) for w in world.want(corpus, sel, 0))
    pu.close()


def test_two_batches_equal_one(capi, world, corpus):
    pu = capi.Pileup(world.idx, 0, strands=12)
    for lo, hi in ((0, 23), (23, None)):
        world.eng.add_pileup(pu, capi.COV_ALL, quals=world.classify(corpus, lo, hi))
    check(strand_counts(pu), world.want(corpus, covref.ALL, 12), "two batches")
    pu.reset()
    assert not any(c.any() for c in strand_counts(pu))
    pu.close()


@pytest.mark.parametrize("thr,sthr", THRESHOLDS)
def test_variants_by_strand_equal_the_reference(capi, world, corpus, thr, sthr):
    pu = capi.Pileup(world.idx, 0, strands=12)
    world.eng.add_pileup(pu, capi.COV_ALL, quals=world.classify(corpus))
    want = world.want(corpus, covref.ALL, 12)
    sizes = []
    for rid in (-1, 1):
        w = strandref.variants(want, world.seqs, rid, thr, sthr)
        got = pu.variants_strands(rid, *thr, *sthr)
        assert got.dtype == capi.VARIANT_STRAND_DTYPE and got.tobytes() == w.tobytes(), f"contig {rid}: {len(got)} against {len(w)}"
        sizes.append(len(w))
    loose, plain = pu.variants_strands(-1, *thr, 0, 0), pu.variants(-1, *thr)    # the strand rule takes some away, and not all
    assert 0 < sizes[1] <= sizes[0] < len(loose) == len(plain) and all(np.array_equal(loose[k], plain[k]) for k in capi.VARIANT_DTYPE.names)
    pu.close()


def test_an_allele_of_one_strand_only_is_filtered(capi, world):
    g, lo = world.clean[2], 8_000
    one, both = lo + 1_000, lo + 1_300                            # under every read: they start every 100 bases, 1 500 long
    reads = []
    for i in range(10):
        rd = g[lo + 100 * i:lo + 100 * i + 1_500].copy()
        for at in (both,) if i % 2 else (one, both):
            rd[at - lo - 100 * i] = util.ACGT[(np.searchsorted(util.ACGT, g[at]) + 1) % 4]
        reads.append(util.revcomp(rd) if i % 2 else rd)
    world.eng.classify(*util.pack_reads(reads), MIN_MAPQ)
    pu = capi.Pileup(world.idx, 0, strands=0)
    world.eng.add_pileup(pu, capi.COV_GATED)
    assert [(int(v["pos"]), int(v["count"])) for v in pu.variants(2, 1, 1, 0)] == [(one, 5), (both, 10)]
    v = pu.variants_strands(2, 1, 1, 0, 1, 0)
    assert [(int(x["pos"]), int(x["count"]), int(x["count_fwd"]), int(x["span"]), int(x["span_fwd"])) for x in v] == [(both, 10, 5, 10, 5)]
    pu.close()


@pytest.mark.parametrize("case", ("store after an add", "no qualities for a mask", "qualities for a plain pileup", "min_qual out of range"))
def test_refusals(capi, world, corpus, case):
    L = capi.lib()
    q = world.classify(corpus, 0, 8)
    pu = capi.Pileup(world.idx, 0, strands=12 if case == "no qualities for a mask" else None)
    if case == "store after an add":
        world.eng.add_pileup(pu, capi.COV_ALL)
        assert L.mnc_pileup_store_strands(pu._h, 0) == capi.ERR_ARG
        assert L.mnc_pileup_fetch_strand_counts(pu._h, 0, 0, 1, q.ctypes.data) == capi.ERR_ARG
    elif case == "no qualities for a mask":
        assert L.mnc_engine_add_pileup(world.eng._h, pu._h, capi.COV_ALL) == capi.ERR_ARG and b"add with qualities" in L.mnc_last_error()
        assert not any(c.any() for c in strand_counts(pu))
    elif case == "qualities for a plain pileup":
        assert L.mnc_engine_add_pileup_quals(world.eng._h, pu._h, capi.COV_ALL, q.ctypes.data, 0) == capi.ERR_ARG and not pu.counts(0).any()
    else:
        assert [L.mnc_pileup_store_strands(pu._h, x) for x in (-1, 94, 93)] == [capi.ERR_ARG, capi.ERR_ARG, capi.OK]
    pu.close()
