"""Reads assigned to barcodes on the device (mnc_demux_*, mnc_engine_add_demux; csrc/k_demux.hip).

Reference: tests/demuxref.py, the contract as the textbook table.  Every tag field and count is compared by exact integer
equality, at the smallest shapes at which the kernel takes another path."""
import numpy as np
import pytest

import demuxref
import util
from demuxref import BOTH, EITHER, FRONT

pytestmark = pytest.mark.gpu
ACGT = util.ACGT


def mutate(rng, seq, rate):
    """`seq` with a substitution, an inserted or a dropped base at about `rate` of its places."""
    out = []
    for c in seq:
        k = rng.integers(0, 3) if rng.random() < rate else -1
        if k == 0:
            out.append(ACGT[(np.searchsorted(ACGT, c) + 1 + rng.integers(0, 3)) % 4])
        elif k == 1:
            out += [c, ACGT[rng.integers(0, 4)]]
        elif k < 0:
            out.append(c)
    return np.array(out, dtype=np.uint8)


def world(seed, lens, n_barcodes, window, n_reads, twin=False):
    """(barcodes, reads): barcodes of the lengths `lens` in turn (`twin`: the last equals the first); reads with barcodes at both
    ends, at one, different ones, at 0 to 15 % errors, N runs, lower case, random reads, lengths 0, 1, |p| - 1, W - 1, W, W + 1."""
    rng = np.random.default_rng(seed)
    bcs = [ACGT[rng.integers(0, 4, lens[b % len(lens)])] for b in range(n_barcodes)]
    if twin:
        bcs[-1] = bcs[0].copy()
    rand = lambda n: ACGT[rng.integers(0, 4, max(int(n), 0))]
    exact = [0, 1, len(bcs[0]) - 1, window - 1, window, window + 1]
    reads = []
    for i in range(n_reads):
        a, b = bcs[rng.integers(0, n_barcodes)], bcs[rng.integers(0, n_barcodes)]
        rate, kind = rng.random() * 0.15, i % 6
        front = mutate(rng, a, rate) if kind != 3 else rand(len(a))
        rear = util.revcomp(mutate(rng, a if kind in (0, 4) else b, rate)) if kind in (0, 2, 4) else rand(len(a))
        body = rand(rng.integers(0, 2 * window) if i % 4 else rng.integers(0, 8))
        r = np.concatenate([rand(rng.integers(0, 9)), front, body, rear, rand(rng.integers(0, 9))])
        if kind == 4 and len(r):
            s = rng.integers(0, len(r))
            r[s:s + 3] = ord("N")
            r = np.frombuffer(r.tobytes().lower(), dtype=np.uint8).copy() if i % 12 == 4 else r
        if kind == 5:
            r = r[:exact[(i // 6) % 6]] if len(r) >= exact[(i // 6) % 6] else np.concatenate([r, rand(exact[(i // 6) % 6] - len(r))])
        reads.append(r)
    return [b.tobytes() for b in bcs], reads


def same(tags, want):
    for f in demuxref.TAG_DTYPE.names:
        assert np.array_equal(tags[f], want[f]), (f, np.flatnonzero(tags[f] != want[f])[:5], tags[tags[f] != want[f]][:5], want[tags[f] != want[f]][:5])


CASES = {
    **{f"len{m}": dict(lens=[m], n=5, window=100, n_reads=96) for m in (1, 31, 32, 33, 63, 64)},   # the word-width switch, the top bit
    "mixed": dict(lens=[1, 7, 24, 32, 33, 64, 40], n=7, window=100, n_reads=120),
    **{f"n{n}": dict(lens=[24], n=n, window=40, n_reads=96) for n in (1, 2, 32, 33, 65, 256)},   # one pass, two ends in one pass, several
    **{f"w{w}": dict(lens=[12], n=3, window=w, n_reads=72) for w in (1, 24, 150, 1024)},
    "front": dict(lens=[24], n=12, window=60, n_reads=96, ends=FRONT),
    "both": dict(lens=[24], n=12, window=60, n_reads=96, ends=BOTH),
    "tie": dict(lens=[16], n=6, window=60, n_reads=96, min_margin=0, twin=True),
    "dist0": dict(lens=[20, 40], n=6, window=80, n_reads=96, max_dist=0),
    "many": dict(lens=[8], n=2, window=12, n_reads=20_000, max_dist=1),       # every wave of the persistent grid takes several reads
    "dist_all": dict(lens=[9], n=4, window=30, n_reads=96, max_dist=9, min_margin=0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_tags_and_reads_equal_the_reference(capi, name):
    c = dict(dict(ends=EITHER, max_dist=4, min_margin=2, twin=False), **CASES[name])
    bcs, reads = world(len(name) * 131 + c["n"], c["lens"], c["n"], c["window"], c["n_reads"], c["twin"])
    want = demuxref.tags(bcs, reads, c["window"], c["max_dist"], c["min_margin"], c["ends"])
    kinds = set(want["barcode"].tolist())
    assert name in ("dist_all", "w1", "len1") or (-1 in kinds and max(kinds) >= 0), kinds
    dm = capi.Demux(None, bcs, c["window"], c["max_dist"], c["min_margin"], c["ends"], cap_reads=len(reads))
    assert dm.info()["word_bits"] == (32 if max(c["lens"]) <= 32 else 64)
    for bits in (0, 64):                                          # the wide kernel gives the same answer on short patterns
        dm.reset(), dm.set_word_bits(bits)
        dm.add(*util.pack_reads(reads))
        same(dm.tags(), want)
        reads_n, taxa = dm.counts()
        assert taxa is None and np.array_equal(reads_n, demuxref.read_counts(want, c["n"]))
    dm.close()


def test_counts_are_additive_and_tags_are_the_latest_adds(capi):
    bcs, reads = world(7, [24, 30], 5, 50, 90)
    want = demuxref.tags(bcs, reads, 50, 4, 2, EITHER)
    assert {-2, -1, 0} <= set(want["barcode"].tolist())
    dm = capi.Demux(None, bcs, 50, 4, 2, EITHER, cap_reads=60)
    assert capi.lib().mnc_demux_add(dm._h, None, np.zeros(62, dtype=np.int64).ctypes.data, 61, 0) == capi.ERR_RANGE
    dm.add(*util.pack_reads(reads[:60])), dm.add(*util.pack_reads(reads[60:]))
    same(dm.tags(), want[60:])
    same(dm.tags(0, 60), np.concatenate([want[60:], want[30:60]]))              # the first add's tags stay behind the second's
    assert np.array_equal(dm.counts()[0], demuxref.read_counts(want, 5))
    assert dm.info()["n_conflict"] == (want["barcode"] == -2).sum() and dm.info()["n_assigned"] == (want["barcode"] >= 0).sum()
    dm.reset()
    assert not dm.counts()[0].any() and dm.tags(0, 60).tolist() == [(-1, 255, 255, 0, 0)] * 60
    dm.close()


def test_planted_kit_barcodes_are_found_and_never_mistaken(capi):
    """96 random 24-mers, window 150, max_dist 6, min_margin 2; one barcode behind 5 to 59 random bases at 10 % errors."""
    rng = np.random.default_rng(96)
    bcs = [ACGT[rng.integers(0, 4, 24)] for _ in range(96)]
    truth = rng.integers(0, 96, 300)
    reads = [np.concatenate([ACGT[rng.integers(0, 4, rng.integers(5, 60))], mutate(rng, bcs[t], 0.10), ACGT[rng.integers(0, 4, 400)]]) for t in truth]
    want = demuxref.tags([b.tobytes() for b in bcs], reads, 150, 6, 2, FRONT)
    got_one = want["barcode"] >= 0                                # (the reference alone: 297 of 300, none wrong)
    assert got_one.sum() >= 0.85 * len(reads) and (want["barcode"][got_one] == truth[got_one]).all(), got_one.sum()
    dm = capi.Demux(None, [b.tobytes() for b in bcs], 150, 6, 2, FRONT, cap_reads=len(reads))
    dm.add(*util.pack_reads(reads))
    same(dm.tags(), want)
    dm.close()


# the taxa table in the counting kernel's LDS, and (257 rows of 8 genomes: 6 168 words) beyond it
@pytest.mark.parametrize("n_genomes,n_bc,genome_len", [(4, 5, 200_000), (8, 256, 40_000)])
def test_an_engines_batch_gets_the_same_tags_and_taxa_per_barcode(capi, n_genomes, n_bc, genome_len):
    rng = np.random.default_rng(5)
    names, seqs = util.small_genomes(n_genomes, genome_len, genome_len * 3 // 2)
    idx = capi.Index.from_seqs(names, seqs)
    bcs = [ACGT[rng.integers(0, 4, 24)] for _ in range(n_bc)]
    reads = []
    for i in range(60):
        g = seqs[i % len(seqs)]
        s = rng.integers(0, len(g) - 2000)
        piece = g[s:s + 1500] if i % 7 else ACGT[rng.integers(0, 4, 1500)]     # (a random read: no genome)
        bc = bcs[i % 5]
        reads.append(np.concatenate([mutate(rng, bc, 0.05), piece, util.revcomp(bc) if i % 3 else bc[:0]]) if i % 11 else piece)
    bases, offsets = util.pack_reads(reads)
    eng, eng2 = capi.Engine(idx, 0), capi.Engine(idx, 0)
    dm, plain = capi.Demux(idx, [b.tobytes() for b in bcs], cap_reads=len(reads)), capi.Demux(None, [b.tobytes() for b in bcs], cap_reads=len(reads))
    assign, best, _ = eng.classify(bases, offsets, 0)
    eng2.classify(*util.pack_reads(reads[::-1]), 0)                             # a second engine, the same reads backwards:
    eng2.add_demux(dm), eng.add_demux(dm)                                       # the counts double, the tags are the later add's
    plain.add(bases, offsets)
    tags = dm.tags()
    same(tags, plain.tags())
    assert (tags["barcode"] >= 0).sum() >= 40 and (tags["barcode"] == -1).sum() >= 3 and (assign >= 0).sum() >= 40
    want, hit = np.zeros((n_bc + 1, len(names), 3), dtype=np.int64), assign >= 0
    row = np.where(tags["barcode"] >= 0, tags["barcode"], n_bc)[hit]
    np.add.at(want, (row, idx.contig_genome[assign[hit]]), np.stack([np.ones(hit.sum(), dtype=np.int64), np.diff(offsets)[hit], best["mlen"][hit]], axis=1))
    reads_n, taxa = dm.counts()
    assert want[n_bc].any() and want[:5].any(axis=(1, 2)).all() and np.array_equal(taxa, 2 * want) and np.array_equal(reads_n, 2 * plain.counts()[0])
    for x in (dm, plain, eng, eng2):
        x.close()
