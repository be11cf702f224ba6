"""Haplotag (mnc_haplotag_*, mnc_engine_add_haplotag; csrc/k_haplotag.hip) against tests/hapref.py -- the contract in plain
Python -- over test_gpu_linkage's world: the CPU ORACLE's regions and CIGARs.  Every comparison is of integers, for equality.
One test has an answer that does not come from the oracle: the reads of two planted haplotypes."""
import numpy as np
import pytest

import covref
import hapref
import linkref
import util
from test_gpu_alignments import mutate
from test_gpu_linkage import MIN_MAPQ, PHASE, World, alt_of

pytestmark = pytest.mark.gpu

# the block layouts: linkref.phase at test_gpu_linkage's three settings, every site a block of its own (one vote decides),
# and runs of exactly 64 sites per contig under a seeded random phase.  Each with its (min_votes, min_permille).
LAYOUTS = {"phase0": (2, 600), "phase1": (2, 600), "phase2": (3, 1000), "single": (1, 0), "runs64": (2, 600)}


def layout(world, name):
    sites, n = world.sites, len(world.sites)
    if name.startswith("phase"):
        return linkref.phase(world.want[covref.ALL][1], sites, *PHASE[int(name[5:])])
    if name == "single":
        return np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    k = np.concatenate([np.arange(c) for c in np.bincount(sites["rid"])])          # a site's rank on its contig
    start = k % 64 == 0
    phase = np.random.default_rng(0x4A9).integers(0, 2, n).astype(np.uint8)
    return (np.cumsum(start) - 1).astype(np.int32), np.where(start, 0, phase).astype(np.uint8)


class Ref:
    """hapref's answers for every layout and both selectors, computed once; check(): what the corpus must hold for the
    comparisons to mean anything, from the reference alone."""

    def __init__(self, world):
        self.stmts = {sel: hapref.statements(world.ref, world.reads, sel, MIN_MAPQ, world.seqs, world.sites) for sel in (covref.GATED, covref.ALL)}
        self.layouts = {name: layout(world, name) for name in LAYOUTS}
        self.want = {(name, sel): hapref.tally(st, *self.layouts[name], *LAYOUTS[name]) for name in LAYOUTS for sel, st in self.stmts.items()}

    def check(self):
        seen = dict.fromkeys(("border", "chunk start", "two blocks", "tie", "permille", "untagged", "words"), False)
        for (name, _), (blk, tag, _, pairs) in self.want.items():
            block, (min_votes, min_permille) = self.layouts[name][0], LAYOUTS[name]
            decided = {}
            for k, j, first, b, n0, n1, voted in pairs:
                chunks = {(i - first) // 64 for i in voted}
                seen["border"] |= any(c in chunks and c + 1 in chunks for c in chunks)
                head = int(np.searchsorted(block, b))                 # the block's first site
                seen["chunk start"] |= head > first and (head - first) % 64 == 0
                hap = hapref.decide(n0, n1, min_votes, min_permille)
                decided[k, j] = decided.get((k, j), 0) + (hap is not None)
                seen["tie"] |= n0 == n1
                seen["permille"] |= hap is None and n0 != n1 and n0 + n1 >= min_votes
            seen["two blocks"] |= max(decided.values()) >= 2
            seen["untagged"] |= bool((tag == -1).any() and (tag >= 0).any())
            seen["words"] |= bool(blk.any(axis=0).all())
        assert all(seen.values()), seen


@pytest.fixture(scope="module")
def world(capi, oracle):
    w = World(capi, oracle)
    w.hap = Ref(w)
    w.hap.check()                                               # (before anything runs on the GPU)
    return w


def tagger(capi, world, name, cap_reads=None):
    return capi.Haplotag(world.idx, world.sites, *world.hap.layouts[name], len(world.reads) if cap_reads is None else cap_reads, *LAYOUTS[name])


def same(got, want):
    return got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("name", LAYOUTS)
@pytest.mark.parametrize("sel", (covref.GATED, covref.ALL))
def test_blocks_and_tags_equal_the_reference(capi, world, sel, name):
    blk, tag, votes, _ = world.hap.want[name, sel]
    world.classify()
    ht = tagger(capi, world, name)
    assert ht.n_blocks == len(blk) and ht.device_bytes() >= 10 * len(world.sites) + 16 * len(blk) + 12 * len(world.reads)
    world.eng.add_haplotag(ht, sel)
    got, (got_tag, got_votes) = ht.blocks(), ht.tags()
    assert same(got, blk), np.argwhere(got != blk)[:8]
    assert same(got_tag, tag), np.flatnonzero(got_tag != tag)[:8]
    assert same(got_votes, votes) and same(ht.blocks(3, 5), blk[3:8])
    ht.close()


def test_batch_cut_and_reset(capi, world):
    blk = world.hap.want["phase0", covref.ALL][0]
    ht = tagger(capi, world, "phase0")
    for cut in (23, 41):
        for lo, hi in ((0, cut), (cut, None)):
            world.classify(lo, hi)
            world.eng.add_haplotag(ht, capi.COV_ALL)
        _, tag, votes, _ = hapref.tally(world.hap.stmts[covref.ALL][cut:], *world.hap.layouts["phase0"], *LAYOUTS["phase0"])
        got_tag, got_votes = ht.tags()                            # the last piece's
        assert same(ht.blocks(), blk) and same(got_tag, tag) and same(got_votes, votes), cut
        ht.reset()
        assert not ht.blocks().any() and (ht.tags()[0] == -1).all() and not ht.tags()[1].any()
    ht.close()


def test_planted_haplotypes(capi, world):
    """test_gpu_linkage's construction: contig 1, SNVs every 150-250 bases, haplotype A with the alt at the even ones, B at the
    odd; two reads per haplotype every 250 bases at 8 % errors -- of 3 kb, not 2: at 2 kb 22 of the 192 reads are undecided in
    the reference (16 of them without a gated record), at 3 kb 7.  Sites, block and phase from the reference."""
    rng, g = np.random.default_rng(0x9A91), world.clean[1]
    at = 2_000 + np.cumsum(rng.integers(150, 251, 55))
    haps = [g.copy(), g.copy()]
    for k, p in enumerate(at):
        haps[k % 2][p] = alt_of(g[p], k)
    reads = [mutate(rng, h[s:s + 3_000], 0.03, 0.025, 0.025) for s in range(1_000, 13_000, 250) for h in haps for _ in range(2)]
    reads = [util.revcomp(r) if i % 3 == 0 else r for i, r in enumerate(reads)]
    truth = np.arange(len(reads)) // 2 % 2
    sites = np.array([(1, p, 0, 0, b"N", alt_of(g[p], k).tobytes(), 0) for k, p in enumerate(at)], dtype=capi.VARIANT_DTYPE)
    mapped = world.map(reads)
    block, phase = linkref.phase(linkref.tally(mapped, reads, covref.GATED, MIN_MAPQ, world.seqs, sites, 1)[1], sites, 3, 500)
    blk, tag, votes, _ = hapref.tally(hapref.statements(mapped, reads, covref.GATED, MIN_MAPQ, world.seqs, sites), block, phase, 2, 600)
    # ---- conditions on the inputs, from the reference alone: one block; no decided read against its haplotype, up to the
    # swap of the two labels; at most one read in ten undecided
    said = tag >= 0
    assert not block.any() and (((tag[said] & 1) == truth[said]).all() or ((tag[said] & 1) != truth[said]).all())
    assert (~said).sum() * 10 <= len(reads) and blk[0, 0] > 20 and blk[0, 1] > 20
    world.eng.classify(*util.pack_reads(reads), MIN_MAPQ)
    ht = capi.Haplotag(world.idx, sites, block, phase, len(reads), 2, 600)
    world.eng.add_haplotag(ht, capi.COV_GATED)
    got_tag, got_votes = ht.tags()
    assert same(ht.blocks(), blk) and same(got_tag, tag) and same(got_votes, votes)
    ht.close()


@pytest.mark.parametrize("case", ("another index", "chain contract", "bad selector", "above cap_reads"))
def test_errors(capi, world, case):
    L = capi.lib()
    idx = world.idx if case != "another index" else capi.Index.from_seqs(world.names, world.seqs)
    ht = capi.Haplotag(idx, world.sites, *world.hap.layouts["phase0"], 7 if case == "above cap_reads" else 8)
    lk = capi.Linkage(idx, world.sites, 1)
    try:
        if case == "chain contract":
            world.eng.set_contract(capi.CONTRACT_CHAIN)
        world.classify(0, 8)
        for what in (0, capi.COV_GATED | capi.COV_ALL, capi.COV_GATED | capi.COV_SPAN, 1 << 9) if case == "bad selector" else (capi.COV_GATED,):
            rc = L.mnc_engine_add_haplotag(world.eng._h, ht._h, what)
            assert rc == (capi.ERR_RANGE if case == "above cap_reads" else L.mnc_engine_add_linkage(world.eng._h, lk._h, what)) != capi.OK, (case, what)
            assert case == "above cap_reads" or rc == capi.ERR_ARG
        assert not ht.blocks().any() and L.mnc_haplotag_fetch_tags(ht._h, 8, None, None) == capi.ERR_ARG
    finally:
        world.eng.set_contract(capi.CONTRACT_DP)
        ht.close(), lk.close()
