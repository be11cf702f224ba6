"""Phased pileup (mnc_engine_add_pileup_phased; csrc/k_pile_phase.hip) against tests/phaseref.py -- the contract in plain
Python -- over test_gpu_linkage's world and test_gpu_haplotag's block layouts, plus `dense`: more blocks under one record than
the kernel's window holds.  Every comparison is of integers, for equality."""
import numpy as np
import pytest

import covref
import linkref
import phaseref
import pileref
import util
from test_gpu_alignments import mutate
from test_gpu_haplotag import LAYOUTS, layout
from test_gpu_linkage import LENS, MIN_MAPQ, World, alt_of

pytestmark = pytest.mark.gpu

W = 256                                                         # csrc/k_pile_phase.hip: PHASE_W
THR = dict(LAYOUTS, dense=(1, 0))                               # (min_votes, min_permille) per layout
SELS = (covref.GATED, covref.ALL)
NO_HAP1 = ("phase2", "runs64")


def dense(world, capi, rid=0, lo=2_000, n=W + 200):
    """A site with a base allele at every base of a stretch, a '-' site as well at every 7th; every site its own block."""
    rows = [(rid, lo + k, 0, 0, b"N", a, 0) for k in range(n) for a in (alt_of(world.seqs[rid][lo + k], k).tobytes(), b"-")[:1 + (k % 7 == 0)]]
    return np.array(rows, dtype=capi.VARIANT_DTYPE), np.arange(len(rows), dtype=np.int32), np.zeros(len(rows), dtype=np.uint8)


@pytest.fixture(scope="module")
def world(capi, oracle):
    w = World(capi, oracle)
    w.lay = {name: (w.sites, *layout(w, name)) for name in LAYOUTS}
    w.lay["dense"] = dense(w, capi)
    w.phased = {(name, sel): phaseref.tally(w.ref, w.reads, sel, MIN_MAPQ, w.seqs, *w.lay[name], *THR[name]) for name in THR for sel in SELS}
    # ---- what the corpus must hold for the comparisons to mean anything, from the reference alone
    notes = [n for _, n in w.phased.values()]
    assert all(any(n[key] for n in notes) for key in ("M changes haplotype", "D over a border", "I on a last base"))
    assert any(d and (max(d) - first) // W > (min(d) - first) // W for first, d in w.phased["dense", covref.ALL][1]["decided"]), "no window border crossed"
    # (but haplotype 1 under unanimous pairs and under runs of a random phase: this world's reads decide no record for it)
    assert all(any(p.any() for p in dest) for (name, _), (planes, _) in w.phased.items() for k, dest in enumerate(planes)
               if (k, name in NO_HAP1) != (1, True)), "an empty destination"
    return w


def adds(capi, world, name, sel, rest=True, pieces=((0, None),), into=None):
    # the corpus in `pieces` into fresh pileups (or `into`) of hap0, hap1 and the rest
    ht = capi.Haplotag(world.idx, *world.lay[name], 1, *THR[name])          # (cap_reads plays no part)
    pus = into or [capi.Pileup(world.idx, 0) for _ in range(2 + rest)]
    for lo, hi in pieces:
        world.classify(lo, hi)
        world.eng.add_pileup_phased(ht, *pus, what=sel)
    return pus, ht


def equal(pus, want):
    got = [[pu.counts(rid) for rid in range(len(LENS))] for pu in pus]
    return all(g.dtype == np.int32 and np.array_equal(g, x) for gs, ws in zip(got, want) for g, x in zip(gs, ws))


@pytest.mark.parametrize("name", THR)
@pytest.mark.parametrize("sel", SELS)
def test_planes_equal_the_reference(capi, world, sel, name):
    want = world.phased[name, sel][0]
    pus, ht = adds(capi, world, name, sel)
    plain = capi.Pileup(world.idx, 0)
    world.eng.add_pileup(plain, sel)
    assert equal(pus, want) and not ht.blocks().any()
    assert equal([plain], [[sum(pu.counts(rid) for pu in pus) for rid in range(len(LENS))]])
    if (name, sel) == ("dense", covref.ALL):                    # without a rest: the haplotypes' planes are the same
        two, _ = adds(capi, world, name, sel, rest=False)
        assert equal(two, want[:2])


def test_batch_cut_and_reset(capi, world):
    want, pus = world.phased["phase0", covref.ALL][0], None
    for cut in (23, 41):
        pus, _ = adds(capi, world, "phase0", covref.ALL, pieces=((0, cut), (cut, None)), into=pus)
        assert equal(pus, want), cut
        for pu in pus:
            pu.reset()
        assert not any(pu.counts(rid).any() for pu in pus for rid in range(len(LENS)))


def test_planted_haplotypes(capi, world):
    """test_gpu_haplotag's construction (contig 1, one block of 55 SNVs, reads of 3 kb from two haplotypes)."""
    rng, g = np.random.default_rng(0x9A91), world.clean[1]
    at = 2_000 + np.cumsum(rng.integers(150, 251, 55))
    haps = [g.copy(), g.copy()]
    for k, p in enumerate(at):
        haps[k % 2][p] = alt_of(g[p], k)
    reads = [mutate(rng, h[s:s + 3_000], 0.03, 0.025, 0.025) for s in range(1_000, 13_000, 250) for h in haps for _ in range(2)]
    reads = [util.revcomp(r) if i % 3 == 0 else r for i, r in enumerate(reads)]
    sites = np.array([(1, p, 0, 0, b"N", alt_of(g[p], k).tobytes(), 0) for k, p in enumerate(at)], dtype=capi.VARIANT_DTYPE)
    mapped, lo, hi = world.map(reads), int(at[0]), int(at[-1]) + 1
    block, phase = linkref.phase(linkref.tally(mapped, reads, covref.GATED, MIN_MAPQ, world.seqs, sites, 1)[1], sites, 3, 500)
    planes, _ = phaseref.tally(mapped, reads, covref.GATED, MIN_MAPQ, world.seqs, sites, block, phase, 2, 600)
    want = [pileref.consensus(planes[d], world.seqs, 1, lo, hi, 8) for d in (0, 1)]
    # ---- the condition on the input, from the reference alone
    planted = [bytes(h[at]) for h in haps]
    assert not block.any() and sorted(bytes(c[p - lo] for p in at) for c in want) == sorted(planted) and b"N" not in want[0] + want[1]
    world.eng.classify(*util.pack_reads(reads), MIN_MAPQ)
    ht, pus = capi.Haplotag(world.idx, sites, block, phase, 1, 2, 600), [capi.Pileup(world.idx, 0) for _ in range(2)]
    world.eng.add_pileup_phased(ht, *pus, what=capi.COV_GATED)
    assert [pu.consensus(1, lo, hi, 8) for pu in pus] == want


@pytest.mark.parametrize("case", ("another index", "chain contract", "bad selector", "hap0 is hap1", "store_insertions", "store_strands"))
def test_errors(capi, world, case):
    L, ht = capi.lib(), capi.Haplotag(world.idx, *world.lay["phase0"], 8)
    other = capi.Index.from_seqs(world.names, world.seqs) if case == "another index" else world.idx
    pus = [capi.Pileup(world.idx, 0), capi.Pileup(other, 0, insertions=(16, 64) if case == "store_insertions" else None),
           capi.Pileup(world.idx, 0, strands=0 if case == "store_strands" else None)]
    try:
        if case == "chain contract":
            world.eng.set_contract(capi.CONTRACT_CHAIN)
        world.classify(0, 8)
        for what in (0, capi.COV_GATED | capi.COV_ALL, capi.COV_GATED | capi.COV_SPAN, 1 << 9) if case == "bad selector" else (capi.COV_GATED,):
            h = [pu._h for pu in pus]
            assert L.mnc_engine_add_pileup_phased(world.eng._h, ht._h, h[0], h[0] if case == "hap0 is hap1" else h[1], h[2], what) == capi.ERR_ARG, what
        assert not any(pu.counts(0).any() for pu in pus)
    finally:
        world.eng.set_contract(capi.CONTRACT_DP)
