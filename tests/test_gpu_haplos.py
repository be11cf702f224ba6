"""Haplos (mnc_haplos_*, mnc_engine_add_haplos; csrc/k_haplos.hip) against tests/haploref.py -- the contract in plain Python
-- over the CPU ORACLE's regions and CIGARs, on the world of test_gpu_linkage.py.  Every comparison is of integers, for
equality.  Two tests have answers that do not come from the oracle: k = 2 is the pair table, and three planted strains."""
import ctypes as C

import numpy as np
import pytest

import covref
import haploref
import util
from test_gpu_linkage import MIN_MAPQ, World, alt_of

pytestmark = pytest.mark.gpu

KS = (2, 3, 6)
THRESHOLDS = ((1, 1, 0), (4, 2, 200))    # (min_total, min_count, min_permille): anything seen; twice, and a fifth of the window


@pytest.fixture(scope="module")
def world(capi, oracle):
    w = World(capi, oracle)
    extra = [w.clean[0][7_990:9_500].copy()]                    # ONE site under it: fewer than any k
    w.reads, w.ref = w.reads + extra, w.ref + w.map(extra)
    w.bases, w.offsets = util.pack_reads(w.reads)
    w.hap = {(sel, k): haploref.tally(w.ref, w.reads, sel, MIN_MAPQ, w.seqs, w.sites, k) for sel in (covref.GATED, covref.ALL) for k in KS}
    # ---- what the corpus must hold for the comparisons to mean anything, from the oracle and haploref alone: the records ALL adds
    sites, codes = w.sites, [haploref.pileref.ref_codes(s) for s in w.seqs]
    recs = [(r, cig, read) for (regs, cigs), read in zip(w.ref, w.reads)
            for r, cig, selected in zip(regs, cigs, covref.select(regs, covref.ALL, MIN_MAPQ)) if selected]
    under = [np.flatnonzero((sites["rid"] == r["rid"]) & (sites["pos"] >= r["rs"]) & (sites["pos"] < r["re"])) for r, _, _ in recs]
    assert 1 in [len(u) for u in under] and max(len(u) for u in under) > 64
    ends = list(np.flatnonzero(np.diff(sites["rid"])) + 1) + [len(sites)]
    for k in KS:
        hap, inside, straddles = w.hap[covref.ALL, k], np.zeros(len(sites), dtype=np.int64), 0
        for (r, cig, read), u in zip(recs, under):
            inside[u[:max(len(u) - k + 1, 0)]] += 1             # the windows inside the record's range of sites
            straddles += len(u) > 64 and None not in haploref.said(r, cig, read, sites[u[65 - k:65]], codes)
        assert straddles, "no spelled window over a 64-site chunk border of a record"
        assert hap[:, 1:].any() and (inside > hap.sum(axis=1)).any(), "no non-zero pattern, or no record that is missing at a site"
        assert all(hap[e - k + 1:e].sum() == 0 for e in ends), "the last k - 1 rows of a contig"
    assert ((w.hap[covref.ALL, 6] > 0).sum(axis=1) >= 3).any(), "no window with three patterns at k = 6"
    return w


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def raw_words(hp):
    import torch                                                # row[n_sites][2^k], then track[n_sites]; after a read-out: behind every add
    iface = {"shape": (((1 << hp.k) + 1) * len(hp.sites),), "typestr": "<i4", "data": (hp.device(), False), "version": 2}
    return torch.as_tensor(type("Words", (), {"__cuda_array_interface__": iface})(), device="cuda:0").cpu().numpy()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("sel", (covref.GATED, covref.ALL))
def test_tables_equal_the_reference(capi, world, sel, k):
    want = world.hap[sel, k]
    world.classify()
    hp = capi.Haplos(world.idx, world.sites, k)
    assert hp.device_bytes() >= len(world.sites) * (4 * (1 << k) + 4)
    world.eng.add_haplos(hp, sel)
    got = hp.table()
    assert same(got, want), np.argwhere(got != want)[:8]
    assert same(hp.table(70, 9), want[70:79])
    hp.close()


def test_k2_is_the_pair_table(capi, world):
    world.classify()
    hp, lk = capi.Haplos(world.idx, world.sites, 2), capi.Linkage(world.idx, world.sites, 1)
    world.eng.add_haplos(hp, capi.COV_ALL)
    world.eng.add_linkage(lk, capi.COV_ALL)
    assert hp.table().any() and same(hp.table(), lk.pairs()[:, 0, :])
    hp.close(), lk.close()


def test_batch_cut_and_reset(capi, world):
    want = world.hap[covref.ALL, 3]
    hp = capi.Haplos(world.idx, world.sites, 3)
    for cut in (23, 41):
        for lo, hi in ((0, cut), (cut, None)):
            world.classify(lo, hi)
            world.eng.add_haplos(hp, capi.COV_ALL)
        assert same(hp.table(), want) and raw_words(hp).any(), cut
        hp.reset()
        assert not hp.table().any() and not raw_words(hp).any()
    hp.close()


@pytest.mark.parametrize("k", (3, 6))
@pytest.mark.parametrize("thr", THRESHOLDS)
def test_call_equals_the_reference(capi, world, thr, k):
    want = haploref.call(world.hap[covref.ALL, k], world.sites, thr, len(world.seqs))
    assert len(want[3]) > 1 and len(np.unique(want[0])) >= 3 and want[2][1].sum() == 0 and (want[0][want[1] > 0] == 0).any() == (thr[1] > 1)
    world.classify()
    hp = capi.Haplos(world.idx, world.sites, k)
    world.eng.add_haplos(hp, capi.COV_ALL)
    got = hp.call(*thr)
    assert got[3].dtype == capi.HAPLO_DTYPE and all(same(g, x) for g, x in zip(got[:3], want[:3])) and got[3].tolist() == want[3].tolist()
    n, out = C.c_int64(0), np.full(len(want[3]), -1, dtype=capi.HAPLO_DTYPE)
    assert capi.lib().mnc_haplos_call(hp._h, *thr, None, None, None, out.ctypes.data, len(out) - 1, C.byref(n)) == capi.ERR_RANGE
    assert n.value == len(out) and (out["window"] == -1).all()
    hp.close()


def test_three_planted_strains(capi, world):
    """One contig of 6 kb, a site every 40 bases from 1 000 on.  Strain A is the contig; among the first fifty sites B carries
    the alt allele at every fourth and C at every fourth, two further on, so each k = 4 window there tells the three apart
    and the windows behind show one pattern.  Thirty error-free reads of 1.5-2 kb, ten per strain, both strands; their ends
    lie 20 bases from the nearest site, so every record covers its read and the answer follows from the reads' places."""
    g, k, j = world.clean[1][:6_000].copy(), 4, np.arange(100)
    at = 1_000 + 40 * j
    alt = np.array([alt_of(g[p], x) for x, p in enumerate(at)], dtype=np.uint8)
    carries = [j < 0, (j % 4 == 0) & (j < 50), (j % 4 == 2) & (j < 50)]
    strains = [g.copy() for _ in carries]
    for z, c in zip(strains, carries):
        z[at[c]] = alt[c]
    reads, want = [], np.zeros((100, 1 << k), dtype=np.int32)
    for i in range(30):
        s, e = 20 + 40 * (i * 7 % 100), 20 + 40 * (i * 7 % 100) + 1_520 + 40 * (i % 13)
        reads.append(util.revcomp(strains[i % 3][s:e]) if i % 2 else strains[i % 3][s:e].copy())
        for w in range(100 - k + 1):
            if s <= at[w] and at[w + k - 1] < e:                # the read covers the window: its strain's pattern, first site first
                want[w, int("".join("01"[int(b)] for b in carries[i % 3][w:w + k]), 2)] += 1
    idx = capi.Index.from_seqs(world.names[:1], [g])
    eng, sites = capi.Engine(idx, 0), np.array([(0, p, 0, 0, b"N", bytes([a]), 0) for p, a in zip(at, alt)], dtype=capi.VARIANT_DTYPE)
    hp = capi.Haplos(idx, sites, k)
    eng.classify(*util.pack_reads(reads), MIN_MAPQ)
    eng.add_haplos(hp, capi.COV_GATED)
    n_haps, total, hist, rec = hp.call()
    assert same(hp.table(), want) and np.array_equal(n_haps, (want > 0).sum(axis=1)) and np.array_equal(total, want.sum(axis=1))
    assert (n_haps == 3).any() and (n_haps == 1).any() and hist[0, 3] > 0 and hist[0].sum() == (total > 0).sum() and len(rec) == n_haps.sum()
    assert not raw_words(hp)[:100 << k].reshape(100, 1 << k)[:, 0].any(), "a missing word"
    hp.close()
