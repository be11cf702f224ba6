"""Alignment records of a whole batch (mnc_engine_export_alignments / _fetch_alignments, csrc/k_export.hip) on the GPU.

References: regions and CIGARs are the CPU oracle's (oracle.pyoracle, as in test_gpu_parity.py); cs and MD are
tests/alnref.py -- the contract restated in plain Python -- applied to the oracle's CIGAR and this file's own sequences.
Nothing is compared against the stage dumps or against the code under test (the one exception is asked for by name:
the mappy_compat case compares `Hit`s from the records with `Hit`s built from the dumps, attribute by attribute)."""
import ctypes as C
import re

import numpy as np
import pytest

import alnref
import util
from monica_amd import synth

pytestmark = pytest.mark.gpu

ACGT = util.ACGT
REC_FROM_REG = ("rid", "rev", "qs", "qe", "rs", "re", "mapq", "mlen", "blen", "score", "cnt", "dp_score", "dp_max", "n_ambi", "n_cigar")


def mutate(rng, piece, sub=0.04, ins=0.03, dele=0.03):
    """Substitutions, insertions (after a base) and deletions at the given per-base rates."""
    piece = np.asarray(piece, dtype=np.uint8)
    u = rng.random(len(piece))
    keep, subm, insm = u >= dele, (u >= dele) & (u < dele + sub), (u >= dele + sub) & (u < dele + sub + ins)
    new = piece.copy()
    new[subm] = ACGT[(np.searchsorted(ACGT, piece[subm]) + rng.integers(1, 4, int(subm.sum()))) % 4]
    counts = keep.astype(np.int64) + insm
    out = np.repeat(new, counts)
    out[np.cumsum(counts)[insm] - 1] = ACGT[rng.integers(0, 4, int(insm.sum()))]
    return out


def substitute(piece, at):
    p = np.asarray(piece, dtype=np.uint8).copy()
    p[at] = ACGT[(np.searchsorted(ACGT, p[at]) + 1) % 4]
    return p


class World:
    def __init__(self, capi, oracle, names, seqs):
        self.capi, self.names, self.seqs = capi, names, seqs
        self.idx = capi.Index.from_seqs(names, seqs)
        self.oidx = oracle.Index.from_seqs(names, [s.tobytes() for s in seqs])
        self.oidx.opt.cigar = 1
        self.eng = capi.Engine(self.idx, 0)

    def reference(self, reads):
        """Per read: the oracle's regions and CIGARs, and alnref's (cs, MD) of every region."""
        out = []
        for rd in reads:
            regs, cigs = self.oidx.map_cigar(np.asarray(rd, dtype=np.uint8).tobytes())
            strs = [alnref.cs_md_of_hit(g, c, self.seqs[int(g["rid"])], rd) for g, c in zip(regs, cigs)]
            out.append((regs, cigs, strs))
        return out


def check_records(capi, got, ref, min_mapq):
    """Every record field, the CSR and the CIGAR pool against the oracle."""
    off, recs, cig, _, _ = got
    n_reg = [len(r[0]) for r in ref]
    assert off.tolist() == np.concatenate([[0], np.cumsum(n_reg)]).astype(np.int64).tolist()
    assert len(recs) == sum(n_reg)
    want_words, k = [], 0
    for r, (regs, cigs, _) in enumerate(ref):
        g = recs[off[r]:off[r + 1]]
        assert (g["read"] == r).all()
        for name in REC_FROM_REG:
            assert np.array_equal(g[name], regs[name]), f"read {r}: {name}: {g[name]} != {regs[name]}"
        assert np.array_equal(g["nm"], regs["blen"] - regs["mlen"] + regs["n_ambi"]), f"read {r}: nm"
        primary = regs["id"] == regs["parent"]
        want_flags = primary.astype(np.int32) | ((primary & (regs["mapq"] >= min_mapq)).astype(np.int32) << 1) | (regs["flags"] << 8)
        assert np.array_equal(g["flags"], want_flags), f"read {r}: flags {g['flags']} != {want_flags}"
        for i, c in enumerate(cigs):
            assert int(g["cigar_off"][i]) == k, f"read {r} region {i}: cigar_off"
            want_words += [l << 4 | "MID".index(op) for l, op in c]
            k += len(c)
    assert len(cig) == k and cig.tolist() == want_words, "CIGAR pool"


def strings_of(got):
    off, recs, cig, cs, md = got
    cs_b, md_b = cs.tobytes(), md.tobytes()
    return ([cs_b[a["cs_off"]:a["cs_off"] + a["cs_len"]].decode() for a in recs],
            [md_b[a["md_off"]:a["md_off"] + a["md_len"]].decode() for a in recs])


def check_strings(got, ref, cs=True, md=True):
    off, recs, _, cs_pool, md_pool = got
    g_cs, g_md = strings_of(got)
    want = [s for _, _, strs in ref for s in strs]
    assert len(want) == len(recs)
    if cs:
        assert g_cs == [w[0] for w in want]
        assert len(cs_pool) == sum(len(w[0]) for w in want)                 # sized exactly, back to back
        assert recs["cs_off"].tolist() == np.concatenate([[0], np.cumsum(recs["cs_len"])[:-1]]).tolist()[:len(recs)]
    else:
        assert len(cs_pool) == 0 and not recs["cs_len"].any()
    if md:
        assert g_md == [w[1] for w in want]
        assert len(md_pool) == sum(len(w[1]) for w in want)
        assert recs["md_off"].tolist() == np.concatenate([[0], np.cumsum(recs["md_len"])[:-1]]).tolist()[:len(recs)]
    else:
        assert len(md_pool) == 0 and not recs["md_len"].any()


@pytest.fixture(scope="module")
def world(capi, oracle):
    names, seqs = util.small_genomes(4, 60_000, 60_000)
    return World(capi, oracle, names[:3], seqs[:3])            # two independent contigs and a 3 % diverged copy of the first


@pytest.fixture(scope="module")
def corpus(world):
    """200 reads of 2 kb at 10 % errors from both strands, 20 random reads among them; the reference, computed once."""
    rng = np.random.default_rng(0xA11)
    reads = []
    for i in range(200):
        g = world.seqs[i % 3]
        s = int(rng.integers(0, len(g) - 2000))
        rd = mutate(rng, g[s:s + 2000])
        reads.append(util.revcomp(rd) if rng.integers(0, 2) else rd)
    for i in range(20):
        reads.insert(int(rng.integers(0, len(reads) + 1)), ACGT[rng.integers(0, 4, 2000)])
    bases, offsets = util.pack_reads(reads)
    return dict(reads=reads, bases=bases, offsets=offsets, ref=world.reference(reads))


def test_records_equal_the_oracle(capi, world, corpus):
    ref = corpus["ref"]
    assert sum(len(r[0]) == 0 for r in ref) >= 20 and sum(len(r[0]) > 1 for r in ref) >= 3          # unmapped reads; reads with secondaries
    for min_mapq in (0, 60):
        world.eng.classify(corpus["bases"], corpus["offsets"], min_mapq)
        got = world.eng.alignments()
        check_records(capi, got, ref, min_mapq)
        check_strings(got, ref, cs=False, md=False)
        gated = (got[1]["flags"] & 2) != 0
        assert gated.any() and (min_mapq == 0 or not gated.all())
        # the gate bit is the gate of the call: the gated records are the engine's gated hits
        hit_off, hits = world.eng.fetch_hits()
        assert np.array_equal(got[1]["rid"][gated], hits["rid"]) and np.array_equal(got[1]["nm"][gated], hits["nm"])


def test_cs_and_md_equal_the_reference(capi, world, corpus):
    ref = corpus["ref"]
    regs = np.concatenate([r[0] for r in ref])
    want = [s for _, _, strs in ref for s in strs]
    # the corpus covers what the kernel can get wrong (asserted on the reference, so the test cannot pass vacuously)
    assert (regs["n_cigar"] > 64).any() and (regs["n_cigar"] > 128).any(), "no CIGAR beyond one / two chunks of 64 operations"
    assert (regs["rev"] == 1).any() and (regs["rev"] == 0).any()
    assert any("^" in m and re.search(r"\^[ACGTN]+0[ACGTN]", m) for _, m in want), "no mismatch right after a deletion"
    assert any(re.search(r"\+[acgtn]+\*", c) for c, _ in want), "no insertion directly followed by a mismatch"
    world.eng.classify(corpus["bases"], corpus["offsets"], 0)
    for cs, md in ((True, False), (False, True), (True, True)):
        got = world.eng.alignments(cs=cs, MD=md)
        check_records(capi, got, ref, 0)
        check_strings(got, ref, cs=cs, md=md)
    # cross-invariants, on reads without ambiguous bases (all of them here)
    g_cs, g_md = strings_of(got)
    assert not regs["n_ambi"].any()
    for a, c, cig in zip(got[1], g_cs, [c for r in ref for c in r[1]]):
        assert sum(int(x) for x in re.findall(r":(\d+)", c)) == a["mlen"]
        n_mis = c.count("*")
        n_ins = sum(l for l, op in cig if op == "I")
        n_del = sum(l for l, op in cig if op == "D")
        assert a["nm"] == n_mis + n_ins + n_del


def test_run_length_widths(capi, world):
    g = world.seqs[1]
    exact = g[10_000:13_000].copy()
    runs = [400, 9, 10, 99, 100, 999, 1000]                    # match runs between substitutions; the rest (376) follows the last
    at = np.cumsum(runs) + np.arange(len(runs))
    assert at[0] >= 60 and 3000 - at[-1] > 60 and at[-1] + 1 + 376 == 3000
    spaced = substitute(g[20_000:23_000], at)
    reads = [exact, spaced, util.revcomp(spaced)]
    ref = world.reference(reads)
    assert [s for _, _, strs in ref[:1] for s in strs][0] == (":3000", "3000")
    for k in (1, 2):
        tokens = re.findall(r":(\d+)", ref[k][2][0][0])
        assert {"9", "10", "99", "100", "999", "1000"} <= set(tokens), tokens
    bases, offsets = util.pack_reads(reads)
    world.eng.classify(bases, offsets, 0)
    got = world.eng.alignments(cs=True, MD=True)
    check_records(capi, got, ref, 0)
    check_strings(got, ref)
    assert strings_of(got)[0][0] == ":3000" and strings_of(got)[1][0] == "3000"


def test_ambiguous_bases(capi, oracle):
    names, seqs = util.small_genomes(4, 60_000, 60_000)
    seqs = [s.copy() for s in seqs[:2]]
    clean = seqs[0][29_000:31_000].copy()
    seqs[0][30_000:30_030] = ord("N")                         # a 30-base N run inside a mapped stretch
    w = World(capi, oracle, names[:2], seqs)
    over = clean.copy()                                        # real bases against the N run; Ns of its own elsewhere
    over[300:303] = ord("N")
    over[1700] = ord("n")
    same = seqs[0][29_000:31_000].copy()                       # N against N over the whole run
    reads = [over, same, util.revcomp(over)]
    ref = w.reference(reads)
    for regs, cigs, strs in ref:
        assert len(regs) >= 1 and regs["n_ambi"][0] > 0
    (cs0, md0), (cs1, md1) = ref[0][2][0], ref[1][2][0]
    assert re.search(r"\*n[acgt]", cs0) and re.search(r"\*[acgt]n", cs0) and "N" in md0
    assert "n" not in cs1 and "N" not in md1 and "*" not in cs1                # n against n: a match, inside a run
    bases, offsets = util.pack_reads(reads)
    w.eng.classify(bases, offsets, 0)
    got = w.eng.alignments(cs=True, MD=True)
    check_records(capi, got, ref, 0)
    check_strings(got, ref)


def _raw_export(capi, eng, what):
    n = [C.c_int64(-1) for _ in range(4)]
    rc = capi.lib().mnc_engine_export_alignments(eng._h, what, *[C.byref(x) for x in n])
    return rc, [int(x.value) for x in n]


def test_edges(capi, world, corpus):
    eng, L = world.eng, capi.lib()
    g = world.seqs[1]
    rng = np.random.default_rng(5)
    mapped = [mutate(rng, g[5_000:6_500]), util.revcomp(mutate(rng, g[40_000:41_500]))]
    junk = ACGT[rng.integers(0, 4, 1500)]
    # one read
    ref1 = world.reference(mapped[:1])
    eng.classify(*util.pack_reads(mapped[:1]), 0)
    got = eng.alignments(cs=True, MD=True)
    check_records(capi, got, ref1, 0)
    check_strings(got, ref1)
    # no read maps: all sizes 0, fetch succeeds with empty arrays
    eng.classify(*util.pack_reads([junk, junk[::-1].copy(), np.zeros(0, dtype=np.uint8)]), 0)
    rc, sizes = _raw_export(capi, eng, capi.ALN_CS | capi.ALN_MD)
    assert rc == 0 and sizes == [0, 0, 0, 0]
    off = np.full(4, -7, dtype=np.int64)
    assert L.mnc_engine_fetch_alignments(eng._h, off.ctypes.data, None, 0, None, 0, None, 0, None, 0) == 0
    assert off.tolist() == [0, 0, 0, 0]
    # an unmapped read between two mapped ones
    reads = [mapped[0], junk, mapped[1]]
    ref3 = world.reference(reads)
    assert len(ref3[1][0]) == 0 and len(ref3[0][0]) and len(ref3[2][0])
    bases3, offsets3 = util.pack_reads(reads)
    eng.classify(bases3, offsets3, 0)
    got3 = eng.alignments(cs=True, MD=True)
    check_records(capi, got3, ref3, 0)
    check_strings(got3, ref3)
    # export twice: identical bytes
    again = eng.alignments(cs=True, MD=True)
    for a, b in zip(got3, again):
        assert a.tobytes() == b.tobytes()
    # each cap one too small: MNC_ERR_RANGE and nothing written
    rc, sizes = _raw_export(capi, eng, capi.ALN_CS | capi.ALN_MD)
    assert rc == 0 and all(s > 0 for s in sizes) and sizes[0] == len(got3[1])
    for short in range(4):
        caps = [s - (1 if k == short else 0) for k, s in enumerate(sizes)]
        bufs = [np.full(len(offsets3), 0x55, dtype=np.int64), np.full(sizes[0] * capi.ALN_DTYPE.itemsize, 0x55, dtype=np.uint8),
                np.full(sizes[1], 0x55555555, dtype=np.uint32), np.full(sizes[2], 0x55, dtype=np.uint8), np.full(sizes[3], 0x55, dtype=np.uint8)]
        before = [b.tobytes() for b in bufs]
        rc = L.mnc_engine_fetch_alignments(eng._h, bufs[0].ctypes.data, bufs[1].ctypes.data, caps[0], bufs[2].ctypes.data, caps[1],
                                           bufs[3].ctypes.data, caps[2], bufs[4].ctypes.data, caps[3])
        assert rc == capi.ERR_RANGE, short
        assert [b.tobytes() for b in bufs] == before, short
    # the pools are counted in the engine's device bytes, and their device addresses are there
    ptrs = eng.alignments_device()
    assert all(ptrs) and eng.device_bytes() > sum(sizes[1:]) + sizes[0] * capi.ALN_DTYPE.itemsize
    # export, classify another batch, export again: it follows the new batch
    eng.classify(*util.pack_reads(mapped[:1]), 0)
    got = eng.alignments(cs=True, MD=True)
    check_records(capi, got, ref1, 0)
    check_strings(got, ref1)
    # a classify call invalidates what was exported: fetch without export is refused
    eng.classify(bases3, offsets3, 0)
    assert L.mnc_engine_fetch_alignments(eng._h, None, None, 0, None, 0, None, 0, None, 0) == capi.ERR_ARG
    assert _raw_export(capi, eng, 4)[0] == capi.ERR_ARG and _raw_export(capi, eng, -1)[0] == capi.ERR_ARG
    # an engine that has classified nothing
    fresh = capi.Engine(world.idx, 0)
    assert _raw_export(capi, fresh, 0)[0] == capi.ERR_ARG
    fresh.classify(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), 0)          # an empty batch exports as nothing
    assert _raw_export(capi, fresh, capi.ALN_CS) == (0, [0, 0, 0, 0])
    fresh.close()


def test_chain_contract_has_records_only(capi, world, corpus):
    eng = capi.Engine(world.idx, 0)
    eng.set_contract(capi.CONTRACT_CHAIN)
    n = 40
    offsets = corpus["offsets"][:n + 1]
    bases = corpus["bases"][:offsets[-1]]
    eng.classify(bases, offsets, 0)
    for what in (capi.ALN_CS, capi.ALN_MD, capi.ALN_CS | capi.ALN_MD):
        assert _raw_export(capi, eng, what)[0] == capi.ERR_ARG
    off, recs, cig, cs, md = eng.alignments()
    raw = bases.tobytes()
    world.oidx.opt.cigar = 0
    try:
        oregs = [world.oidx.map(raw[offsets[r]:offsets[r + 1]]) for r in range(n)]
    finally:
        world.oidx.opt.cigar = 1
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in oregs])]).tolist() and len(recs) > 20
    assert len(cig) == 0 and len(cs) == 0 and len(md) == 0 and not recs["n_cigar"].any()
    o = np.concatenate(oregs)
    for name in ("rid", "rev", "qs", "qe", "rs", "re", "mapq", "mlen", "blen", "score", "cnt"):
        assert np.array_equal(recs[name], o[name]), name
    assert np.array_equal(recs["nm"], o["blen"] - o["mlen"]) and np.array_equal(recs["flags"] & 1, (o["id"] == o["parent"]).astype(np.int32))
    eng.close()


def test_long_forms(capi, oracle):
    names, seqs = util.small_genomes(2, 110_000, 110_000, seed=0x77)
    w = World(capi, oracle, names, seqs)
    rng = np.random.default_rng(70)
    g0 = seqs[0]
    long_read = mutate(rng, g0[20_000:90_000], sub=0.03, ins=0.025, dele=0.025)       # 70 kb at 8 % errors
    assert len(long_read) > 65_536
    inversion = np.concatenate([g0[40_000:42_000], util.revcomp(g0[42_000:42_700]), g0[42_700:44_700]])
    reads = [util.revcomp(long_read), inversion]
    ref = w.reference(reads)
    assert ref[0][0]["n_cigar"].max() > 2000                                      # thousands of operations in one region
    assert (ref[1][0]["flags"] & 16).any() and (ref[1][0]["flags"] & (2 | 4)).any()   # an inversion region and the halves of the split
    bases, offsets = util.pack_reads(reads)
    w.eng.classify(bases, offsets, 0)
    got = w.eng.alignments(cs=True, MD=True)
    check_records(capi, got, ref, 0)
    check_strings(got, ref)


def test_mappy_compat(capi, world, corpus, tmp_path):
    from monica_amd import mappy_compat
    path = str(tmp_path / "three.idx")
    world.idx.save(path)
    al = mappy_compat.Aligner(fn_idx_in=path, device=0)
    assert al
    attrs = [a for a in mappy_compat.Hit.__slots__ if a not in ("cs", "MD")]
    some = [r for r in range(len(corpus["reads"])) if len(corpus["ref"][r][0]) > 0][:9] + \
           [r for r in range(len(corpus["reads"])) if len(corpus["ref"][r][0]) == 0][:1]
    per_read = []
    for r in some:
        rd = corpus["reads"][r]
        hits = list(al.map(rd.tobytes().decode(), cs=True, MD=True))
        eng = al.engine()
        regs, cigs = eng.dump(capi.DUMP_REGS, capi.REG_DTYPE), eng.cigars()
        assert len(hits) == len(regs) == len(corpus["ref"][r][0])
        for h, reg, cig, (cs, md) in zip(hits, regs, cigs, corpus["ref"][r][2]):
            old = mappy_compat.Hit(reg, al.index, cig)
            for a in attrs:
                assert getattr(h, a) == getattr(old, a), a
            assert h.cigar_str == old.cigar_str and repr(h) == repr(old)
            assert (h.cs, h.MD) == (cs, md) and h.trans_strand == 0 and h.read_num == 1
        plain = list(al.map(rd.tobytes()))                     # without the flags: empty strings, as mappy
        assert [(h.cs, h.MD) for h in plain] == [("", "")] * len(hits)
        per_read.append(hits)
    # the batch form equals per-read map()
    bases, offsets = util.pack_reads([corpus["reads"][r] for r in some])
    off, recs, cig, cs_b, md_b = al.map_batch_alignments(bases, offsets, cs=True, MD=True)
    assert np.diff(off).tolist() == [len(h) for h in per_read]
    for k, hits in enumerate(per_read):
        for h, rec in zip(hits, recs[off[k]:off[k + 1]]):
            b = mappy_compat.Hit.from_record(rec, al.index, cig, cs_b, md_b)
            assert rec["read"] == k and all(getattr(b, a) == getattr(h, a) for a in mappy_compat.Hit.__slots__)
    # PAF after a real batch parses back to the records
    fq = str(tmp_path / "ten.fastq")
    synth.write_fastq(fq, bases, offsets, ids=[f"r{k} extra" for k in range(len(some))])
    rd = capi.FastqReader(fq)
    assert rd.next() == len(some)
    eng = al.engine()
    eng.classify_ptr(rd.bases_ptr, rd.offsets_ptr, rd.n, 0)
    out = eng.alignments(cs=True, MD=True)
    paf = str(tmp_path / "ten.paf")
    rd.write_paf(al.index, out[0], out[1], paf, cigar=out[2], cs=out[3], md=out[4])
    lines = open(paf).read().splitlines()
    assert len(lines) == len(recs)
    g_cs, g_md = strings_of(out)
    for ln, a, c, m in zip(lines, out[1], g_cs, g_md):
        f = ln.split("\t")
        assert f[0] == f"r{a['read']}" and int(f[1]) == offsets[a["read"] + 1] - offsets[a["read"]]
        assert [int(x) for x in f[2:4] + f[7:12]] == [a[k] for k in ("qs", "qe", "rs", "re", "mlen", "blen", "mapq")]
        assert f[4] == "+-"[a["rev"]] and f[5] == al.index.contig_names[a["rid"]] and int(f[6]) == al.index.contig_lens[a["rid"]]
        tags = dict((t[:2], t[5:]) for t in f[12:])
        assert tags["tp"] == ("P" if a["flags"] & 1 else "S") and int(tags["NM"]) == a["nm"] and int(tags["AS"]) == a["dp_score"]
        assert int(tags["cm"]) == a["cnt"] and int(tags["s1"]) == a["score"] and int(tags["ms"]) == a["dp_max"] and int(tags["nn"]) == a["n_ambi"]
        words = out[2][a["cigar_off"]:a["cigar_off"] + a["n_cigar"]]
        assert tags["cg"] == "".join(f"{int(x) >> 4}{'MID'[int(x) & 15]}" for x in words) and tags["cs"] == c and tags["MD"] == m
