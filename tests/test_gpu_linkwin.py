"""mnc_linkage_phase_window and mnc_linkage_add_tables (csrc/k_linkage.hip) against tests/linkwinref.py, array for array:
tables made inline and planted through add_tables; one case end to end over the oracle's records."""
import ctypes as C

import numpy as np
import pytest

import covref
import linkref
import linkwinref
import util
from test_gpu_alignments import mutate
from test_gpu_linkage import MIN_MAPQ, alt_of
from test_linkwin_host import random_tables

pytestmark = pytest.mark.gpu
BIG = 1 << 30
LONG, FLIPS = 3_300, np.random.default_rng(7).integers(0, 2, 3_300)
# LONG: more than three tiles of mnc_linkw_local (1024 sites), 25 of mnc_linkw_parent; FLIPS: the chains' orientations


def linkage(capi, sizes, window):
    """an accumulator over sizes[c] sites on the first bases of contig c"""
    seqs = [util.ACGT[np.random.default_rng(c).integers(0, 4, max(k, 1_500))] for c, k in enumerate(sizes)]
    sites = np.array([(c, p, 0, 0, b"N", b"A", 0) for c, k in enumerate(sizes) for p in range(k)], dtype=capi.VARIANT_DTYPE)
    return capi.Linkage(capi.Index.from_seqs(["c%d:1" % c for c in range(len(sizes))], seqs), sites, window)


def table(n, window, links):
    """cell (j, i) of every link (j, i, diff, orientation): diff records in cis or in trans"""
    pair = np.zeros((n, window, 4), dtype=np.int32)
    for j, i, diff, o in links:
        pair[j, i - j - 1, o] = diff
    return pair


def random_case(window, reach):
    sizes = (130, 1, 3, 70, 500)         # contig borders inside a window, inside a tile of 128 and next to one
    pair, _ = random_tables(window * 100 + reach, sizes, window, 0.05)
    return sizes, window, reach, (2, 300), pair, lambda keep, block, phase: (reach == 1 or not keep.all()) and np.bincount(block[keep]).max() > 1 and phase.any()


def bridged():
    """true sites at every contig's even places, linked in trans two apart; nothing between them"""
    sizes, links, base = (41, 1, 61), [], 0
    for k in sizes:
        links += [(base + i - 2, base + i, 9, 1) for i in range(2, k, 2)]
        base += k
    pair, rid = table(sum(sizes), 4, links), np.repeat(np.arange(3), sizes)
    assert np.array_equal(linkwinref.phase_window(pair, rid, 1, 1, 0)[1], np.arange(sum(sizes))), "the adjacent phase sees a link"
    return sizes, 4, 4, (1, 0), pair, lambda keep, block, phase: np.array_equal(block[keep], rid[keep]) and keep.sum() == 21 + 1 + 31 and phase.any() and not phase.all()


CASES = {
    "one site": lambda: ((1,), 1, 1, (1, 0), table(1, 1, []), lambda keep, block, phase: keep.all()),
    "two sites": lambda: ((2,), 1, 1, (1, 0), table(2, 1, [(0, 1, 5, 1)]), lambda keep, block, phase: phase[1] == 1 and not block.any()),
    "window 64 reach 1": lambda: random_case(64, 1), "window 64 reach 5": lambda: random_case(64, 5),
    "window 64 reach 64": lambda: random_case(64, 64), "window 7 reach 7": lambda: random_case(7, 7),
    "chain by one": lambda: ((LONG,), 64, 64, (1, 0), table(LONG, 64, [(i - 1, i, 5, o) for i, o in enumerate(FLIPS) if i]),
                             lambda keep, block, phase: keep.all() and not block.any() and 0 < phase.sum() < LONG),
    "chain by reach": lambda: ((LONG,), 64, 64, (1, 0), table(LONG, 64, [(max(i - 64, 0), i, 5, o) for i, o in enumerate(FLIPS) if i]),
                               lambda keep, block, phase: keep.all() and not block.any() and 0 < phase.sum() < LONG),
    "bridged": bridged,
    # site 3 is linked to 1 in trans and to 0 in cis with one diff: the nearer one wins, which its phase shows
    "tie": lambda: ((4,), 4, 4, (1, 0), table(4, 4, [(0, 1, 6, 0), (1, 3, 7, 1), (0, 3, 7, 0)]), lambda keep, block, phase: phase[3] == 1 and keep.tolist() == [True, True, False, True]),
    "floating tree": lambda: ((4,), 4, 4, (1, 0), table(4, 4, [(0, 2, 5, 0), (1, 3, 5, 1)]), lambda keep, block, phase: keep.tolist() == [True, False, True, False]),
    # site 2: diff 2^30 from site 1, 2^30 + 2^29 from site 0 (the parent; site 1 falls under the edge).  Site 3: 7 in 2^31 - 7 is
    # below 900 permille only in 64 bits (7 000 against 900 * tot = 1.9e12)
    "big counts": lambda: ((4,), 2, 2, (1, 900), np.array([[[0] * 4, [BIG, 0, 0, BIG // 2]], [[BIG, 0, 0, 0], [0] * 4], [[BIG, BIG - 7, 0, 0], [0] * 4], [[0] * 4] * 2],
                           dtype=np.int32), lambda keep, block, phase: keep.tolist() == [True, False, True, True] and block.tolist() == [0, -1, 0, 1]),
}


def same(got, want):
    return all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("case", CASES)
def test_window_phase_equals_the_reference(capi, case):
    sizes, window, reach, thresholds, pair, purpose = CASES[case]()
    want = linkwinref.phase_window(pair, np.repeat(np.arange(len(sizes)), sizes), reach, *thresholds)
    assert purpose(*want), "the reference does not show what the case is there for: the inputs are wrong"
    lk = linkage(capi, sizes, window)
    lk.add_tables(np.zeros((len(pair), 2)), pair)
    block, phase, n_kept = np.zeros(len(pair), dtype=np.int32), np.zeros(len(pair), dtype=np.uint8), C.c_int64(-1)
    assert capi.lib().mnc_linkage_phase_window(lk._h, reach, *thresholds, block.ctypes.data, phase.ctypes.data, C.byref(n_kept)) == capi.OK
    assert same(lk.phase_window(reach, *thresholds), want) and same((block, phase), want[1:]) and n_kept.value == want[0].sum()
    one = lk.phase_window(1, *thresholds)
    assert one[0].all() and same(one[1:], lk.phase(*thresholds))  # reach 1 is the adjacent phase, on the same accumulator
    lk.close()


def test_add_tables_sums_and_refuses(capi):
    sizes, L = (30, 2, 9), capi.lib()
    pair, _ = random_tables(5, sizes, 8, 0.5)
    site = np.random.default_rng(5).integers(0, 9, (len(pair), 2)).astype(np.int32)
    lk = linkage(capi, sizes, 8)
    for times in (1, 2):
        lk.add_tables(site, pair)
        assert np.array_equal(lk.pairs(), times * pair) and np.array_equal(lk.site_counts(), times * site)
    for at, v, word in (((3, 2, 0), -1, b"pair[3][2][0] = -1"), ((29, 0, 3), 4, b"pair[29][0][3] = 4"), ((31, 5, 1), 1, b"pair[31][5][1]"), ((40, 0, 2), 1, b"pair[40][0][2]")):
        bad = pair.copy()
        bad[at] = v
        assert L.mnc_linkage_add_tables(lk._h, site.ctypes.data, bad.ctypes.data) == capi.ERR_ARG and word in L.mnc_last_error(), L.mnc_last_error()
    assert L.mnc_linkage_add_tables(lk._h, (-site).ctypes.data, pair.ctypes.data) == capi.ERR_ARG
    for reach in (0, 9):
        assert L.mnc_linkage_phase_window(lk._h, reach, 1, 0, pair.ctypes.data, pair.ctypes.data, None) == capi.ERR_ARG
    assert L.mnc_linkage_phase_window(lk._h, 8, 1, 0, None, pair.ctypes.data, None) == capi.ERR_ARG
    assert np.array_equal(lk.pairs(), 2 * pair) and np.array_equal(lk.site_counts(), 2 * site)
    lk.close()


def test_planted_haplotypes_among_noise_sites(capi, oracle):
    """test_gpu_linkage.py's planted world (same genome, sites and reads, the haplotypes mixed 50 / 50) with a grid of sites
    where no strain differs: the adjacent phase is cut at every grid site, the window phase is not."""
    names, seqs = util.small_genomes(3, 31_000, 31_000)
    rng, g = np.random.default_rng(0x9A91), seqs[1][:20_003].copy()
    at = 2_000 + np.cumsum(rng.integers(150, 251, 55))
    haps = [g.copy(), g.copy()]
    for k, p in enumerate(at):
        haps[k % 2][p] = alt_of(g[p], k)
    reads = [mutate(rng, h[s:s + 2_000], 0.03, 0.025, 0.025) for s in range(1_000, 13_000, 250) for h in haps for _ in range(2)]
    reads = [util.revcomp(r) if i % 3 == 0 else r for i, r in enumerate(reads)]
    rows = sorted([(int(p), alt_of(g[p], k).tobytes(), k % 2) for k, p in enumerate(at)] + [(p, alt_of(g[p], 0).tobytes(), -1) for p in range(int(at[0]) + 40, 13_000, 97) if p not in at])
    sites = np.array([(0, p, 0, 0, b"N", alt, 0) for p, alt, _ in rows], dtype=capi.VARIANT_DTYPE)
    hap = np.array([h for _, _, h in rows])
    oidx = oracle.Index.from_seqs(names[1:2], [g.tobytes()])
    oidx.opt.cigar = 1
    ref = [oidx.map_cigar(np.asarray(r, dtype=np.uint8).tobytes()) for r in reads]
    _, pair = linkref.tally(ref, reads, covref.GATED, MIN_MAPQ, [g], sites, 8)
    want = keep, block, phase = linkwinref.phase_window(pair, sites["rid"], 8, 3, 500)
    assert keep[hap >= 0].all() and not block[hap >= 0].any(), "the planted sites are not one block: the inputs are wrong"
    assert (hap < 0).sum() > 50 and (~keep[hap < 0] | (np.bincount(block[keep])[block] == 1)[hap < 0]).all(), "a grid site is in a block"
    assert np.bincount(linkref.phase(pair, sites, 3, 500)[0][hap >= 0]).max() == 1, "the adjacent phase joins two planted sites: no grid site between them"
    idx = capi.Index.from_seqs(names[1:2], [g])
    eng, lk = capi.Engine(idx, 0), capi.Linkage(idx, sites, 8)
    eng.classify(*util.pack_reads(reads), MIN_MAPQ)
    eng.add_linkage(lk, capi.COV_GATED)
    assert same(lk.phase_window(8, 3, 500), want)
    true = keep & (hap >= 0)
    assert np.array_equal(phase[true], hap[true]) or np.array_equal(phase[true], 1 - hap[true])
    ht = capi.Haplotag(idx, sites[keep], block[keep], phase[keep], len(reads))
    assert ht.n_blocks == block.max() + 1
    ht.close(), lk.close()
