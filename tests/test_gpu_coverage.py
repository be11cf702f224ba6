"""Depth and breadth of coverage accumulated on the device (mnc_coverage_*, mnc_engine_add_coverage; csrc/k_coverage.hip).

Reference: tests/covref.py -- the contract in plain numpy -- applied to the CPU ORACLE's regions and CIGARs
(oracle.Index.map_cigar, opt.cigar = 1; oracle.Index.map for the chain contract), with the oracle's own gate and covref's
plain-Python best_hit for the selectors.  Nothing is compared against the engine's export or dumps."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import covref
import util
from monica_amd import synth
from test_gpu_alignments import mutate

pytestmark = pytest.mark.gpu

ACGT = util.ACGT
LENS = (60_001, 40_003, 50_000)          # no multiple of a bin width, of 64 or of the scan's tile (1 024)
MIN_MAPQ = 60
SELECTORS = (covref.GATED, covref.PRIMARY, covref.ALL, covref.ASSIGNED)


class World:
    def __init__(self, capi, oracle):
        names, seqs = util.small_genomes(4, 70_000, 70_000)
        # contig 2 is a 1 % diverged copy of contig 0's first 50 000 bases: secondaries, primaries below MAPQ 60
        copy = synth.diverge(seqs[0], 0x77, 10_000)
        self.names, self.seqs = names[:3], [seqs[0][:LENS[0]].copy(), seqs[1][:LENS[1]].copy(), copy[:LENS[2]].copy()]
        self.capi = capi
        self.idx = capi.Index.from_seqs(self.names, self.seqs)
        self.oidx = oracle.Index.from_seqs(self.names, [s.tobytes() for s in self.seqs])
        self.oidx.opt.cigar = 1
        self.eng = capi.Engine(self.idx, 0)
        self._want = {}

    def oracle_dp(self, reads):
        return [self.oidx.map_cigar(np.asarray(rd, dtype=np.uint8).tobytes()) for rd in reads]

    def want(self, key, per_read, what, min_mapq=MIN_MAPQ):
        """covref's tracks and summary for one selector / modifier over the oracle's records, computed once."""
        k = (key, what, min_mapq)
        if k not in self._want:
            recs = covref.records_of(per_read, what, min_mapq)
            tracks = covref.depth(recs, LENS, span=bool(what & covref.SPAN))
            self._want[k] = (tracks, covref.summary(recs, tracks))
        return self._want[k]


def check(cov, want, scale=1):
    """summary, the bins of every contig and the depth of every whole contig, exactly."""
    tracks, summ = want
    got = cov.summary()
    for name in covref.SUMMARY_DTYPE.names:                     # (the same records `scale` times over: the covered bases stay)
        w = summ[name] * (1 if name == "covered" else scale)
        assert np.array_equal(got[name], w), f"summary {name}: {got[name]} != {w}"
    for rid, t in enumerate(tracks):
        d = cov.depth(rid)
        assert d.dtype == np.int32 and len(d) == len(t)
        bad = np.flatnonzero(d != t * scale)
        assert not len(bad), f"contig {rid}: depth differs at {bad[:8]}: {d[bad[:8]]} != {(t * scale)[bad[:8]]}"
        bc, bs = cov.bins(rid)
        wc, ws = covref.bins(t * scale, cov.bin_bases)
        assert bc.dtype == np.int32 and bs.dtype == np.int64
        assert np.array_equal(bc, wc), f"contig {rid}: covered bases per bin"
        assert np.array_equal(bs, ws), f"contig {rid}: depth sum per bin"


@pytest.fixture(scope="module")
def world(capi, oracle):
    return World(capi, oracle)


@pytest.fixture(scope="module")
def corpus(world):
    """~150 reads of 1.5-2 kb at 10 % errors from both strands, random reads among them, and the cases the kernel can get
    wrong: a read that ends on contig 0's last base, one that starts on contig 1's first, a 60-base deletion, a 60-base
    insertion, four chimeras of two contigs (two gated records each).  The oracle's answer is computed once -- and the
    corpus is checked to hold what the tests rely on."""
    rng = np.random.default_rng(0xC0FE)
    reads = []
    for i in range(132):
        g = world.seqs[i % 3]
        n = int(rng.integers(1500, 2001))
        s = int(rng.integers(0, len(g) - n))
        rd = mutate(rng, g[s:s + n])
        reads.append(util.revcomp(rd) if rng.integers(0, 2) else rd)
    for i in range(12):
        reads.insert(int(rng.integers(0, len(reads) + 1)), ACGT[rng.integers(0, 4, 1800)])
    g0, g1 = world.seqs[0], world.seqs[1]
    reads.append(g0[-1500:].copy())                                            # ends on the last base of contig 0
    reads.append(g1[:1500].copy())                                             # starts on the first base of contig 1
    reads.append(np.concatenate([g1[20_000:20_900], g1[20_960:21_800]]))       # a 60-base deletion
    reads.append(np.concatenate([g1[30_000:30_900], ACGT[rng.integers(0, 4, 60)], g1[30_900:31_800]]))   # a 60-base insertion
    for i in range(4):                                                          # chimeras: two gated primaries, best_hit takes one
        reads.append(np.concatenate([mutate(rng, g1[2_000 + 3_000 * i:2_900 + 3_000 * i]), mutate(rng, g0[52_000 + 1_000 * i:53_200 + 1_000 * i])]))
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    bases, offsets = util.pack_reads(reads)
    ref = world.oracle_dp(reads)
    # ---- what keeps the tests honest, on the oracle's output
    regs = np.concatenate([r for r, _ in ref])
    ops = [(l, op) for _, cigs in ref for c in cigs for l, op in c]
    at_end = [g for g in regs if g["re"] == LENS[g["rid"]] and g["rid"] + 1 < len(LENS)]
    assert at_end, "no record that ends on its contig's last base"
    assert any(g["rid"] == at_end[0]["rid"] + 1 and g["rs"] == 0 for g in regs), "the next contig's base 0 is not covered"
    assert sum(len(r) > 1 for r, _ in ref) >= 3, "reads with secondaries"
    assert (regs["rev"] == 1).sum() >= 20
    assert any(op == "D" and l >= 50 for l, op in ops) and any(op == "I" and l >= 50 for l, op in ops)
    assert sum(len(r) == 0 for r, _ in ref) >= 10, "reads without any record"
    primary = regs["id"] == regs["parent"]
    assert (primary & (regs["mapq"] >= MIN_MAPQ)).any() and (primary & (regs["mapq"] < MIN_MAPQ)).any()
    assert (~primary).any()
    n_gated = [int(((r["id"] == r["parent"]) & (r["mapq"] >= MIN_MAPQ)).sum()) for r, _ in ref]
    assert sum(n > 1 for n in n_gated) >= 2, "reads with more than one gated record (ASSIGNED must differ from GATED)"
    return dict(reads=reads, bases=bases, offsets=offsets, ref=ref)


def raw_add(capi, eng, cov, what):
    return capi.lib().mnc_engine_add_coverage(eng._h, cov._h, what)


@pytest.mark.parametrize("bin_bases", [1, 1000, 1024])
def test_every_selector_equals_the_reference(capi, world, corpus, bin_bases):
    world.eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    cov = capi.Coverage(world.idx, 0, bin_bases)
    assert cov.device_bytes() >= 4 * sum(LENS) and cov.device_bytes() < 4 * sum(LENS) + (1 << 16)
    sums = set()
    for sel in SELECTORS:
        for span in (0, covref.SPAN):
            cov.reset()
            world.eng.add_coverage(cov, sel | span)
            want = world.want("corpus", corpus["ref"], sel | span)
            check(cov, want)
            sums.add(int(want[1]["depth_sum"].sum()))
    assert len(sums) == 8 and min(sums) > 0                    # the eight cases are eight different answers
    cov.close()


def test_accumulation_reset_and_a_second_engine(capi, world, corpus):
    n = len(corpus["reads"])
    half = n // 2
    off = corpus["offsets"]
    cov = capi.Coverage(world.idx, 0, 1000)
    what = capi.COV_ALL
    want = world.want("corpus", corpus["ref"], what)
    world.eng.classify(corpus["bases"][:off[half]], off[:half + 1], MIN_MAPQ)
    world.eng.add_coverage(cov, what)
    between = cov.summary()                                     # between the batches of a run: changes nothing
    want_half = world.want("first half", corpus["ref"][:half], what)
    assert np.array_equal(between["depth_sum"], want_half[1]["depth_sum"]) and np.array_equal(between["n_aln"], want_half[1]["n_aln"])
    world.eng.classify(corpus["bases"][off[half]:], off[half:] - off[half], MIN_MAPQ)
    world.eng.add_coverage(cov, what)
    check(cov, want)
    check(cov, want)                                            # reading does not change it
    # a second engine of the same index adds into the same accumulator: the sum
    other = capi.Engine(world.idx, 0)
    other.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    other.add_coverage(cov, what)
    check(cov, want, scale=2)
    cov.reset()
    zero = cov.summary()
    assert not any(zero[k].any() for k in zero.dtype.names)
    assert not cov.depth(0).any() and not cov.bins(1)[0].any() and not cov.bins(2)[1].any()
    other.add_coverage(cov, what)                               # and on after a reset
    check(cov, want)
    other.close()
    cov.close()


@pytest.mark.parametrize("span", [0, covref.SPAN])
def test_two_engines_on_threads_add_into_one_coverage(capi, world, corpus, span):
    """test_gpu_pileup.py's test_two_engines_on_threads_add_into_one_pileup for the coverage accumulator: an add is one
    piece against another thread's, for either kernel."""
    off = corpus["offsets"]
    cut = len(corpus["reads"]) // 2
    what = capi.COV_ALL | span
    cov = capi.Coverage(world.idx, 0, 1000)
    halves = [(corpus["bases"][:off[cut]], off[:cut + 1]), (corpus["bases"][off[cut]:], off[cut:] - off[cut])]
    errors = []

    def work(bases, offsets):
        try:
            eng = capi.Engine(world.idx, 0)
            eng.classify(bases, offsets, MIN_MAPQ)
            eng.add_coverage(cov, what)
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
    want = world.want("corpus", corpus["ref"], what)
    check(cov, want)
    cov.reset()                                                 # and a reset behind them: one add gives the single answer again
    world.eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    world.eng.add_coverage(cov, what)
    check(cov, want)
    cov.close()


def test_a_run_that_ends_on_a_contig_does_not_touch_the_next(capi, world, corpus):
    world.eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    for what in (capi.COV_ALL, capi.COV_ALL | capi.COV_SPAN):
        cov = capi.Coverage(world.idx, 0, 1024)
        world.eng.add_coverage(cov, what)
        tracks, _ = world.want("corpus", corpus["ref"], what)
        assert tracks[0][-1] >= 1 and tracks[1][0] >= 1
        assert int(cov.depth(1, 0, 1)[0]) == int(tracks[1][0])                 # not one less
        assert int(cov.depth(0, LENS[0] - 1, LENS[0])[0]) == int(tracks[0][-1])
        assert np.array_equal(cov.depth(1, 0, 2000), tracks[1][:2000])
        assert np.array_equal(cov.depth(0, LENS[0] - 1700, LENS[0]), tracks[0][-1700:])
        assert len(cov.depth(2, 77, 77)) == 0
        cov.close()


def test_export_is_not_disturbed_and_not_needed(capi, world, corpus):
    eng = world.eng
    eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    plain = eng.alignments(cs=True, MD=True)
    eng.classify(corpus["bases"], corpus["offsets"], MIN_MAPQ)
    before, after = capi.Coverage(world.idx, 0, 1000), capi.Coverage(world.idx, 0, 1000)
    eng.add_coverage(before, capi.COV_GATED)                    # no export has been made for this batch
    sizes = eng.export_alignments(cs=True, MD=True)
    eng.add_coverage(after, capi.COV_GATED)                     # between export and fetch
    got = eng.fetch_alignments(sizes)
    assert len(plain[1]) > 100
    for a, b in zip(plain, got):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    want = world.want("corpus", corpus["ref"], capi.COV_GATED)
    check(before, want)
    check(after, want)
    before.close(), after.close()


def test_chain_contract_needs_span(capi, world, corpus):
    n = 40
    off = corpus["offsets"][:n + 1]
    eng = capi.Engine(world.idx, 0)
    eng.set_contract(capi.CONTRACT_CHAIN)
    eng.classify(corpus["bases"][:off[-1]], off, MIN_MAPQ)
    cov = capi.Coverage(world.idx, 0, 1000)
    for sel in SELECTORS:
        assert raw_add(capi, eng, cov, sel) == capi.ERR_ARG
    zero = cov.summary()
    assert not any(zero[k].any() for k in zero.dtype.names)     # unchanged
    try:
        world.oidx.opt.cigar = 0
        ref = [(world.oidx.map(np.asarray(rd, dtype=np.uint8).tobytes()), None) for rd in corpus["reads"][:n]]
    finally:
        world.oidx.opt.cigar = 1
    assert sum(len(r) for r, _ in ref) >= 20
    for sel in (capi.COV_ALL, capi.COV_ASSIGNED):
        cov.reset()
        eng.add_coverage(cov, sel | capi.COV_SPAN)
        check(cov, world.want("chain", ref, sel | capi.COV_SPAN))
    cov.close()
    eng.close()


def test_a_cigar_longer_than_two_chunks(capi, world):
    rng = np.random.default_rng(66)
    g = world.seqs[1]
    reads = [mutate(rng, g[5_000:11_000], sub=0.04, ins=0.04, dele=0.04), util.revcomp(mutate(rng, g[30_000:36_000], sub=0.04, ins=0.04, dele=0.04))]
    ref = world.oracle_dp(reads)
    assert all(len(r) >= 1 for r, _ in ref) and all(len(c[0]) > 128 for _, c in ref), "CIGARs of more than 128 operations"
    world.eng.classify(*util.pack_reads(reads), 0)
    cov = capi.Coverage(world.idx, 0, 1000)
    world.eng.add_coverage(cov, capi.COV_ALL)
    check(cov, world.want("long cigar", ref, capi.COV_ALL, 0))
    cov.close()


def test_long_reads_alone_and_in_a_mixed_call(capi, oracle):
    n = (1 << 20) + 5000
    g = synth.genome(0x5151, 1_100_000)
    names = [synth.contig_name(0)]
    idx = capi.Index.from_seqs(names, [g])
    oidx = oracle.Index.from_seqs(names, [g.tobytes()])
    oidx.opt.cigar = 1
    eng = capi.Engine(idx, 0)
    eng.set_long_reads(True)
    long_read = g[20_000:20_000 + n].copy()
    assign, _, _ = eng.classify(*util.pack_reads([long_read]), MIN_MAPQ)
    assert assign.tolist() == [0]
    cov = capi.Coverage(idx, 0, 1024)
    what = capi.COV_ASSIGNED | capi.COV_SPAN
    eng.add_coverage(cov, what)                                 # a call whose reads are all long adds like any other
    regs, _ = oidx.map_cigar(long_read.tobytes())
    recs = covref.records_of([(regs, None)], what, MIN_MAPQ)
    assert len(recs) >= 1 and sum(r[2] - r[1] for r in recs if r[4]) >= n - 100
    want = covref.summary(recs, covref.depth(recs, [len(g)], span=True))
    got = cov.summary()
    for name in covref.SUMMARY_DTYPE.names:
        assert np.array_equal(got[name], want[name]), name
    # a mixed call leaves the wide pass alone in the engine: nothing is added
    assign, _, _ = eng.classify(*util.pack_reads([long_read, g[500_000:502_000]]), MIN_MAPQ)
    assert assign.tolist() == [0, 0]
    for w in (what, capi.COV_ALL):
        assert raw_add(capi, eng, cov, w) == capi.ERR_UNSUPPORTED
    again = cov.summary()
    for name in covref.SUMMARY_DTYPE.names:
        assert np.array_equal(again[name], want[name]), name
    cov.close()
    eng.close()


def test_errors(capi, world, corpus):
    L = capi.lib()
    cov = capi.Coverage(world.idx, 0, 1000)
    fresh = capi.Engine(world.idx, 0)
    assert raw_add(capi, fresh, cov, capi.COV_ALL) == capi.ERR_ARG                     # no batch has been classified
    fresh.close()
    world.eng.classify(corpus["bases"][:corpus["offsets"][20]], corpus["offsets"][:21], MIN_MAPQ)
    other_idx = capi.Index.from_seqs(world.names[:1], [world.seqs[1][:20_000]])
    other = capi.Coverage(other_idx, 0, 1000)
    assert raw_add(capi, world.eng, other, capi.COV_ALL) == capi.ERR_ARG               # an accumulator of another index
    for what in (capi.COV_GATED | capi.COV_ALL, capi.COV_ASSIGNED | capi.COV_PRIMARY | capi.COV_SPAN, 15, 0, capi.COV_SPAN, 32, capi.COV_ALL | 64):
        assert raw_add(capi, world.eng, cov, what) == capi.ERR_ARG, what
    for c in (cov, other):
        zero = c.summary()
        assert not any(zero[k].any() for k in zero.dtype.names)
    # fetch_bins: a short cap reports the size and writes nothing
    world.eng.add_coverage(cov, capi.COV_ALL)
    n_bins = (LENS[0] + 999) // 1000
    bc = np.full(n_bins, -7, dtype=np.int32)
    bs = np.full(n_bins, -7, dtype=np.int64)
    n = C.c_int64(0)
    assert L.mnc_coverage_fetch_bins(cov._h, 0, bc.ctypes.data, bs.ctypes.data, n_bins - 1, C.byref(n)) == capi.ERR_RANGE
    assert n.value == n_bins and (bc == -7).all() and (bs == -7).all()
    assert L.mnc_coverage_fetch_bins(cov._h, 0, bc.ctypes.data, bs.ctypes.data, n_bins, C.byref(n)) == capi.OK
    assert n.value == n_bins and (bc >= 0).all() and bc.sum() > 0 and bc[-1] <= 1
    for rid in (-1, 3):
        assert L.mnc_coverage_fetch_bins(cov._h, rid, bc.ctypes.data, bs.ctypes.data, n_bins, C.byref(n)) == capi.ERR_ARG
        assert L.mnc_coverage_fetch_depth(cov._h, rid, 0, 1, bc.ctypes.data) == capi.ERR_ARG
    for start, end in ((-1, 5), (5, 4), (0, LENS[1] + 1)):
        assert L.mnc_coverage_fetch_depth(cov._h, 1, start, end, bc.ctypes.data) == capi.ERR_ARG
    ptr, words = cov.device_track()
    assert ptr and words == sum(LENS)
    cov.close(), other.close()


def test_python_map_batch_and_the_aligner_loop(capi, world, corpus, tmp_path, monkeypatch):
    from monica_amd import aligner, mappy_compat
    dbs = tmp_path / "databases"
    dbs.mkdir()
    synth.write_fasta(str(dbs / "database0.fna.gz"), world.names, world.seqs)
    paths = aligner.indexer(str(dbs), str(tmp_path / "indexes"))
    want = world.want("corpus", corpus["ref"], capi.COV_ASSIGNED)
    # ---- Aligner.map_batch(coverage=)
    al = mappy_compat.Aligner(fn_idx_in=paths[0])
    assert al and al.index.contig_lens == list(LENS)
    cov = al.coverage(bin_bases=1000)
    out = al.map_batch(corpus["bases"], corpus["offsets"], MIN_MAPQ, coverage=cov)
    assert len(out) == 5 and (out[0] >= 0).sum() > 50
    check(cov, want)
    cov.reset()
    al.map_batch(corpus["bases"], corpus["offsets"], MIN_MAPQ, coverage=cov, coverage_what=capi.COV_ALL | capi.COV_SPAN)
    check(cov, world.want("corpus", corpus["ref"], capi.COV_ALL | capi.COV_SPAN))
    cov.close()
    # ---- the loop: several batches of one sample, coverage.csv beside the routed files
    query, outdir = tmp_path / "query", tmp_path / "output"
    query.mkdir(), outdir.mkdir()
    n = len(corpus["reads"])
    synth.write_fastq(str(query / "cov.fastq"), corpus["bases"], corpus["offsets"], ids=[f"r{i}" for i in range(n)])
    monkeypatch.setattr(aligner, "BATCH_READS", 100)
    monkeypatch.setattr(aligner, "BATCH_RAMP", (1.0,))                 # a first batch of 100 reads, the rest behind it
    monkeypatch.setattr(aligner, "PIPE_TRACE", [])
    cwd = os.getcwd()
    try:
        alignment = aligner.multi_threaded_aligner(str(query), paths, mode="basic", mapping_quality=MIN_MAPQ, n_threads=1,
                                                   output_folder=str(outdir), coverage=1000)
    finally:
        os.chdir(cwd)
    assert sum(1 for t in aligner.PIPE_TRACE if t[0] == "classify") >= 2, "one batch only"
    assert sum(sum(c.values()) for c in alignment["cov"].values()) == int(want[1]["n_aln"].sum())   # one record per mapped read
    lines = (query / "mapped" / "cov.coverage.csv").read_text().splitlines()
    assert lines[0] == "genome,contig,length,covered_bases,breadth,mean_depth,alignments"
    assert len(lines) == 1 + len(LENS)
    for rid, line in enumerate(lines[1:]):
        s = want[1][rid]
        assert line == "{},{},{},{},{:.6f},{:.6f},{}".format(world.names[rid], world.names[rid], LENS[rid], int(s["covered"]),
                                                            int(s["covered"]) / LENS[rid], int(s["depth_sum"]) / LENS[rid], int(s["n_aln"]))
    assert sorted(os.listdir(query / "mapped")) == ["cov.coverage.csv", "cov.fastq"]
