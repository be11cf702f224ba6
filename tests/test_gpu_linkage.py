"""Linkage (mnc_linkage_*, mnc_engine_add_linkage; csrc/k_linkage.hip) against tests/linkref.py -- the contract in plain
Python -- over the CPU ORACLE's regions and CIGARs.  Every comparison is of integers, for equality.  One test has an answer
that does not come from the oracle: two planted haplotypes."""
import numpy as np
import pytest

import covref
import linkref
import util
from test_gpu_alignments import mutate

pytestmark = pytest.mark.gpu

LENS = (30_001, 20_003, 25_000)          # no multiple of 64
REF_N = (3_100, 3_300, 3_501)            # contig 2: N's in the reference, inside a covered stretch
MIN_MAPQ = 60
WINDOWS = (1, 16, 64)
PHASE = ((1, 0), (4, 600), (2, 1000))    # (min_pairs, min_permille): any majority; four to one; unanimous pairs only


def alt_of(base, k):
    """an allele that is not the reference base (a reference N: any)"""
    return util.ACGT[(np.searchsorted(util.ACGT, base) + 1 + k % 3) % 4] if base in util.ACGT else util.ACGT[k % 4]


class World:
    """Three contigs, contig 1 without a site.  Sixty reads of 1.5-2 kb at 10 % errors from both strands over 8 kb of contigs
    0 and 2, every other one from a haplotype that carries the alt allele at every fifth grid site; a clean read on contig
    0's first bases and one that ends on its last base.  Sites: every 13th base of the covered stretches with a base allele
    that is not the reference's, every tenth of them with a second allele, contig 0's first and last base, a reference N,
    and '-' sites where the oracle's CIGARs delete and where they do not."""

    def __init__(self, capi, oracle):
        self.names, seqs = util.small_genomes(3, 31_000, 31_000)
        self.clean = clean = [s[:n].copy() for s, n in zip(seqs, LENS)]
        self.seqs = seqs = [s.copy() for s in clean]
        seqs[2][list(REF_N)] = ord("N")
        self.oidx = oracle.Index.from_seqs(self.names, [s.tobytes() for s in seqs])
        self.oidx.opt.cigar = 1
        grid = {0: list(range(0, 8_000, 13)) + list(range(LENS[0] - 1_500, LENS[0] - 1, 13)) + [LENS[0] - 1], 2: list(range(0, 8_000, 13)) + [REF_N[0]]}
        rows = [(rid, p, alt_of(seqs[rid][p], k + x).tobytes()) for rid, at in grid.items() for k, p in enumerate(at) for x in (0, 1) if x == 0 or k % 10 == 0]
        hap = [s.copy() for s in clean]
        for rid, at in grid.items():
            hap[rid][at[::5]] = [alt_of(seqs[rid][p], 5 * k) for k, p in enumerate(at[::5])]
        rng = np.random.default_rng(0x11C4A6E)
        self.reads = []
        for i in range(60):
            rid, at = (0, 2)[i % 2], int(rng.integers(0, 6_000))
            rd = mutate(rng, (hap if i % 4 >= 2 else clean)[rid][at:at + int(rng.integers(1500, 2001))])
            self.reads.append(util.revcomp(rd) if i % 3 == 0 else rd)
        self.reads += [clean[0][:1500].copy(), clean[0][-1500:].copy()]
        self.bases, self.offsets = util.pack_reads(self.reads)
        self.ref = self.map(self.reads)
        self.regs, self.cigars = np.concatenate([r for r, _ in self.ref]), [c for _, cigs in self.ref for c in cigs]
        self.deleted = set()
        for r, cig in zip(self.regs, self.cigars):
            t = int(r["rs"])
            for length, op in cig:
                self.deleted.update((int(r["rid"]), t + k) for k in range(length if op == "D" else 0))
                t += length if op != "I" else 0
        dels = sorted(d for d in self.deleted if d[0] != 1)
        rows += [(rid, p, b"-") for rid, p in dels[::max(len(dels) // 40, 1)]]
        rows += [(rid, p, b"-") for rid in (0, 2) for p in range(7, 6_000, 601) if (rid, p) not in self.deleted]
        rows = sorted(set(rows), key=lambda r: (r[0], r[1], b"ACGT-".index(r[2])))
        self.sites = np.array([(rid, pos, 0, 0, b"N", alt, 0) for rid, pos, alt in rows], dtype=capi.VARIANT_DTYPE)
        self.idx = capi.Index.from_seqs(self.names, seqs)
        self.eng = capi.Engine(self.idx, 0)
        # linkref's tables at the widest window; a narrower window's are their first columns
        self.want = {sel: linkref.tally(self.ref, self.reads, sel, MIN_MAPQ, seqs, self.sites, max(WINDOWS)) for sel in (covref.GATED, covref.ALL)}

    def map(self, reads):
        return [self.oidx.map_cigar(np.asarray(r, dtype=np.uint8).tobytes()) for r in reads]

    def classify(self, lo=0, hi=None):
        hi = len(self.offsets) - 1 if hi is None else hi
        self.eng.classify(self.bases[self.offsets[lo]:self.offsets[hi]], self.offsets[lo:hi + 1] - self.offsets[lo], MIN_MAPQ)

    def check(self):
        """What the corpus must hold for the comparisons to mean anything, from the oracle alone."""
        sites, regs, (site, pair) = self.sites, self.regs, self.want[covref.ALL]
        assert max(len(c) for c in self.cigars) > 128 and (regs["rev"] == 1).sum() >= 10 and (regs["rev"] == 0).sum() >= 10
        assert any(x["re"] == LENS[0] and x["rid"] == 0 for x in regs), "no record that ends on contig 0's last base"
        under = [np.flatnonzero((sites["rid"] == r["rid"]) & (sites["pos"] >= r["rs"]) & (sites["pos"] < r["re"])) for r in regs]
        assert max(len(u) for u in under) > 64 and not (sites["rid"] == 1).any()
        straddles = 0                                           # both sides of a record's 64th site say something
        reads_of = [read for (rr, _), read in zip(self.ref, self.reads) for _ in rr]
        for r, cig, read, u in zip(regs, self.cigars, reads_of, under):
            cols = linkref.columns(r, cig, read) if len(u) > 64 else {}
            straddles += len(u) > 64 and None not in [linkref.statement(cols.get(int(s["pos"])), bytes(s["alt"]), int(linkref.pileref.ref_codes(
                self.seqs[int(s["rid"])])[int(s["pos"])])) for s in sites[u[63:65]]]
        assert straddles, "no pair over a 64-site chunk border of a record"
        assert all((pair[:, 0, k] > 0).any() for k in range(4)), "a cell of the adjacent pairs is empty everywhere"
        dash, on_del = sites["alt"] == b"-", np.array([(int(s["rid"]), int(s["pos"])) in self.deleted for s in sites])
        assert (dash & on_del).any() and (dash & ~on_del).any() and site[dash & on_del, 1].min() > 0 and not site[dash & ~on_del, 1].any()
        at = {(int(s["rid"]), int(s["pos"])): i for i, s in enumerate(sites)}
        assert site[at[0, 0]].sum() and site[at[0, LENS[0] - 1]].sum() and (2, REF_N[0]) in at and len(at) < len(sites) - 10


@pytest.fixture(scope="module")
def world(capi, oracle):
    w = World(capi, oracle)
    w.check()
    return w


def same(got, want):
    return got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("sel", (covref.GATED, covref.ALL))
def test_tables_equal_the_reference(capi, world, sel, window):
    sites, (site, pair) = world.sites, world.want[sel]
    world.classify()
    lk, pu = capi.Linkage(world.idx, sites, window), capi.Pileup(world.idx, 0)
    assert lk.device_bytes() >= len(sites) * (20 * window + 8)
    world.eng.add_linkage(lk, sel)
    world.eng.add_pileup(pu, sel)
    got = lk.site_counts()
    assert same(got, site), np.argwhere(got != site)[:8]
    assert same(lk.pairs(), pair[:, :window]), np.argwhere(lk.pairs() != pair[:, :window])[:8]
    assert same(lk.pairs(70, 9), pair[70:79, :window])
    counts = [pu.counts(rid) for rid in range(len(LENS))]       # the statement rule against the pileup's own allele plane
    base = np.flatnonzero(sites["alt"] != b"-")
    assert np.array_equal(got[base, 1], [counts[int(s["rid"])][1 + b"ACGT".index(s["alt"]), int(s["pos"])] for s in sites[base]])
    lk.close(), pu.close()


def test_batch_cut_and_reset(capi, world):
    site, pair = world.want[covref.ALL]
    lk = capi.Linkage(world.idx, world.sites, 16)
    for cut in (23, 41):
        for lo, hi in ((0, cut), (cut, None)):
            world.classify(lo, hi)
            world.eng.add_linkage(lk, capi.COV_ALL)
        assert same(lk.site_counts(), site) and same(lk.pairs(), pair[:, :16]), cut
        lk.reset()
        assert not lk.site_counts().any() and not lk.pairs().any()
    lk.close()


@pytest.mark.parametrize("min_pairs,min_permille", PHASE)
def test_phase_equals_the_reference(capi, world, min_pairs, min_permille):
    block, phase = linkref.phase(world.want[covref.ALL][1], world.sites, min_pairs, min_permille)
    sizes = np.bincount(block)
    assert (sizes == 1).any() and (sizes > 1).any() and (phase == 0).any() and (phase == 1).any()
    world.classify()
    lk = capi.Linkage(world.idx, world.sites, 1)
    world.eng.add_linkage(lk, capi.COV_ALL)
    got_block, got_phase = lk.phase(min_pairs, min_permille)
    assert same(got_block, block) and got_phase.dtype == np.uint8 and np.array_equal(got_phase, phase)
    lk.close()


def test_planted_haplotypes(capi, world):
    """Contig 1, two haplotypes: SNVs every 150-250 bases, A with the alt at the even ones, B at the odd; two reads of 2 kb per
    haplotype every 250 bases (depth 16 each) at 8 % errors, so an adjacent pair is seen about 20 times."""
    rng, g = np.random.default_rng(0x9A91), world.clean[1]
    at = 2_000 + np.cumsum(rng.integers(150, 251, 55))
    haps = [g.copy(), g.copy()]
    for k, p in enumerate(at):
        haps[k % 2][p] = alt_of(g[p], k)
    reads = [mutate(rng, h[s:s + 2_000], 0.03, 0.025, 0.025) for s in range(1_000, 13_000, 250) for h in haps for _ in range(2)]
    reads = [util.revcomp(r) if i % 3 == 0 else r for i, r in enumerate(reads)]
    sites = np.array([(1, p, 0, 0, b"N", alt_of(g[p], k).tobytes(), 0) for k, p in enumerate(at)], dtype=capi.VARIANT_DTYPE)
    want = np.arange(len(sites)) % 2
    _, pair = linkref.tally(world.map(reads), reads, covref.GATED, MIN_MAPQ, world.seqs, sites, 1)
    block, phase = linkref.phase(pair, sites, 3, 500)
    assert not block.any() and np.array_equal(phase, want), "the reference does not see one alternating block: the inputs are wrong"
    world.eng.classify(*util.pack_reads(reads), MIN_MAPQ)
    lk = capi.Linkage(world.idx, sites, 1)
    world.eng.add_linkage(lk, capi.COV_GATED)
    got_block, got_phase = lk.phase(3, 500)
    assert not got_block.any() and (np.array_equal(got_phase, want) or np.array_equal(got_phase, 1 - want))
    lk.close()


@pytest.mark.parametrize("case", ("another index", "chain contract", "bad selector"))
def test_errors(capi, world, case):
    L = capi.lib()
    idx = world.idx if case != "another index" else capi.Index.from_seqs(world.names, world.seqs)
    lk, pu = capi.Linkage(idx, world.sites, 4), capi.Pileup(idx, 0)
    try:
        if case == "chain contract":
            world.eng.set_contract(capi.CONTRACT_CHAIN)
        world.classify(0, 8)
        for what in (0, capi.COV_GATED | capi.COV_ALL, capi.COV_GATED | capi.COV_SPAN, 1 << 9) if case == "bad selector" else (capi.COV_GATED,):
            rc = L.mnc_engine_add_linkage(world.eng._h, lk._h, what)
            assert rc == L.mnc_engine_add_pileup(world.eng._h, pu._h, what) == capi.ERR_ARG, (case, what)
        assert not lk.site_counts().any() and not lk.pairs().any()
    finally:
        world.eng.set_contract(capi.CONTRACT_DP)
        lk.close(), pu.close()
