"""Reads of 2^20 bases or more (mnc_engine_set_long_reads): index.map() takes a read of any length
(monica/genomes/aligner.py:193, 215).  With the switch on such reads take a second pass whose probe records hold a
24-bit query position (csrc/k_probe.hip, device.h: QPOS_BITS_WIDE); everything from the anchors on is the usual
path.  Known answers, region-by-region parity with the CPU oracle, a mixed batch, the default (still MNC_SKIPPED),
the chain contract and the device-resident entry point."""
import numpy as np
import pytest

from monica_amd import synth
import util
from test_gpu_dp import _noisy_indels
from test_gpu_parity import _world_from

pytestmark = pytest.mark.gpu

LIMIT = 1 << 20
# the errorful reads: this many genome bases, a 5 kb deletion among them placed behind query position 2^20
# (8 % errors with as many insertions as deletions leave the length within a few hundred bases)
NOISY_GENOME_BASES = LIMIT + 40_000
NOISY_FIRST_PIECE = LIMIT + 15_000


@pytest.fixture(scope="module")
def world(capi, oracle):
    g = synth.genome(0x2C2C, 2_300_000)
    other = synth.genome(0x2C2D, 300_000)
    w = _world_from(capi, oracle, [synth.contig_name(0), synth.contig_name(1)], [g, other])
    w["eng"].set_long_reads(True)
    return w


@pytest.fixture(scope="module")
def long_pair(world):
    """The two errorful reads of 2^20 bases and more, the second on the reverse strand."""
    g = world["seqs"][0]
    rng = np.random.default_rng(2020)

    def long_read(start):
        return np.concatenate([_noisy_indels(rng, g[start:start + NOISY_FIRST_PIECE], 0.08),
                               _noisy_indels(rng, g[start + NOISY_FIRST_PIECE + 5000:start + NOISY_GENOME_BASES], 0.08)])

    reads = [long_read(150_000), util.revcomp(long_read(900_000))]
    assert all(len(r) >= LIMIT for r in reads)
    return reads


@pytest.fixture(scope="module")
def long_pair_answers(capi, world, long_pair):
    """What a batch of only the two long reads comes to at min_mapq 60 -- checked against the oracle by
    test_parity_with_the_oracle, used by the tests of the other entry points."""
    eng = world["eng"]
    eng.set_contract(capi.CONTRACT_DP)
    bases, offsets = util.pack_reads(long_pair)
    assign, best, nhits = eng.classify(bases, offsets, 60)
    hit_off, hits = eng.fetch_hits()
    return dict(bases=bases, offsets=offsets, assign=assign.copy(), best=best.copy(), nhits=nhits.copy(),
                hit_off=hit_off.copy(), hits=hits.copy())


@pytest.fixture(scope="module")
def long_pair_oracle(world, long_pair_answers):
    """The oracle's side of the parity test, computed once: regions and CIGARs of each read, decisions and gated hits at
    min_mapq 0 and 60.  Its scalar DP over 1.1 Mb is the long pole (seconds a read), so the four runs go side by side."""
    from concurrent.futures import ThreadPoolExecutor
    oidx = world["oidx"]
    oidx.opt.cigar = 1
    bases, offsets = long_pair_answers["bases"], long_pair_answers["offsets"]
    raw = bases.tobytes()
    with ThreadPoolExecutor(4) as pool:
        per_read = [pool.submit(oidx.map_cigar, raw[offsets[r]:offsets[r + 1]]) for r in range(2)]
        per_mq = {mq: pool.submit(oidx.classify, bases, offsets, mq, 2) for mq in (0, 60)}
        return dict(per_read=[f.result() for f in per_read], per_mq={mq: f.result() for mq, f in per_mq.items()})


def test_known_answers(capi, world):
    g = world["seqs"][0]
    eng = world["eng"]
    eng.set_contract(capi.CONTRACT_DP)
    exact = g[100_000:100_000 + LIMIT].copy()                            # exactly 2^20 bases: the first length of the wide pass
    assign, best, nhits = eng.classify(*util.pack_reads([exact]), 60)
    assert assign.tolist() == [0] and nhits.tolist() == [1]
    assert (int(best["mlen"][0]), int(best["nm"][0]), int(best["mapq"][0])) == (LIMIT, 0, 60)
    regs = eng.dump(capi.DUMP_REGS, capi.REG_DTYPE)
    assert (regs["qs"][0], regs["qe"][0], regs["rs"][0], regs["re"][0]) == (0, LIMIT, 100_000, 100_000 + LIMIT)
    assert eng.cigars()[0] == [(LIMIT, "M")]


def test_known_answer_on_the_reverse_strand_through_aligner_map(capi, world):
    """2^21 + 10 000 bases, reverse-complemented: bit 21 of a query position, and positions counted from the other end."""
    from monica_amd import mappy_compat
    g = world["seqs"][0]
    n = (1 << 21) + 10_000
    al = mappy_compat.Aligner(seq=g.tobytes(), long_reads=True)
    assert al
    hits = list(al.map(util.revcomp(g[50_000:50_000 + n]).tobytes()))
    assert len(hits) == 1
    h = hits[0]
    assert (h.strand, h.mlen, h.blen, h.NM, h.mapq) == (-1, n, n, 0, 60)
    assert (h.q_st, h.q_en, h.r_st, h.r_en) == (0, n, 50_000, 50_000 + n)
    assert h.cigar == [[n, 0]] and h.is_primary
    # the same object without the switch: no hit (the read comes back SKIPPED underneath)
    assert list(mappy_compat.Aligner(seq=g[:400_000].tobytes(), long_reads=False).map(g[:LIMIT].tobytes())) == []


def test_limits_of_the_device_entry_point(capi, world):
    """Nothing runs for a max_read_len of 2^24, for more than 2^16 reads in a wide call, or -- without the switch -- for 2^20."""
    import torch
    dev = torch.device("cuda:0")
    d_bases = torch.zeros(64, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(2, dtype=torch.int64, device=dev)
    d_assign = torch.zeros(1, dtype=torch.int32, device=dev)
    eng = world["eng"]
    for n_reads, max_len in ((1, 1 << 24), (capi.MAX_READS_WIDE + 1, LIMIT)):
        with pytest.raises(capi.MncError) as err:
            eng.classify_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, 0, max_len, 60, d_assign.data_ptr())
        assert err.value.code == capi.ERR_UNSUPPORTED
    plain = capi.Engine(world["idx"], 0)
    with pytest.raises(capi.MncError) as err:
        plain.classify_device(d_bases.data_ptr(), d_off.data_ptr(), 1, 0, LIMIT, 60, d_assign.data_ptr())
    assert err.value.code == capi.ERR_UNSUPPORTED
    plain.close()


def test_parity_with_the_oracle(capi, world, long_pair_answers, long_pair_oracle):
    """Region by region, field by field and CIGAR by CIGAR, gated hits and decisions: a batch of only the two errorful
    reads, at min_mapq 0 and 60 -- the comparisons of test_gpu_parity._compare_dp, against oracle runs made once."""
    bases, offsets = long_pair_answers["bases"], long_pair_answers["offsets"]
    eng = world["eng"]
    eng.set_contract(capi.CONTRACT_DP)
    for mq in (0, 60):
        assign, best, nhits = eng.classify(bases, offsets, mq)
        regs = eng.dump(capi.DUMP_REGS, capi.REG_DTYPE)
        reg_off = eng.dump(capi.DUMP_REG_OFFSETS, np.int64)
        cigs = eng.cigars()
        hit_off, hits = eng.fetch_hits()
        for r in range(2):
            oregs, ocigs = long_pair_oracle["per_read"][r]
            gr = regs[reg_off[r]:reg_off[r + 1]]
            assert len(gr) == len(oregs), f"read {r}: region count {len(gr)} != {len(oregs)} after base-level alignment"
            for name in capi.REG_DTYPE.names:
                assert np.array_equal(gr[name], oregs[name]), f"read {r}: region field {name}: {gr[name]} != {oregs[name]}"
            assert cigs[reg_off[r]:reg_off[r + 1]] == ocigs, f"read {r}: CIGAR"
        oassign, obest, onh, oflat = long_pair_oracle["per_mq"][mq]
        assert np.array_equal(assign, oassign) and np.array_equal(nhits, onh)
        for name in capi.HIT_DTYPE.names:
            assert np.array_equal(best[name], obest[name]), name
            assert np.array_equal(hits[name], oflat[name]), name
        assert np.array_equal(np.diff(hit_off), onh)
    assert assign.tolist() == [0, 0]
    assert np.array_equal(assign, long_pair_answers["assign"]) and np.array_equal(nhits, long_pair_answers["nhits"])
    for r in range(2):
        rr = regs[reg_off[r]:reg_off[r + 1]]
        assert ((rr["qs"] < LIMIT) & (rr["qe"] > LIMIT)).any(), f"read {r}: no region spans query position 2^20"
    assert regs["n_cigar"].max() > 50_000


def test_mixed_batch(capi, world, long_pair, long_pair_answers):
    """40 ordinary reads with the two long ones in the middle and at the end: the ordinary reads come out as in the batch
    without the long ones, the long ones as in a batch of their own, and the gated hits are one CSR in read order."""
    eng = world["eng"]
    eng.set_contract(capi.CONTRACT_DP)
    b, o, _ = synth.reads(world["seqs"], 40, 4000, seed=3)
    normal = [b[o[i]:o[i + 1]] for i in range(40)]
    a0, best0, nh0 = eng.classify(b, o, 60)
    off0, hits0 = eng.fetch_hits()
    c0 = eng.counters()
    assert (a0 >= 0).sum() >= 35
    reads = normal[:20] + [long_pair[0]] + normal[20:] + [long_pair[1]]
    bases, offsets = util.pack_reads(reads)
    assign, best, nhits = eng.classify(bases, offsets, 60)
    hit_off, hits = eng.fetch_hits()
    c1 = eng.counters()
    keep = np.array([i for i in range(42) if i not in (20, 41)])
    assert np.array_equal(assign[keep], a0) and np.array_equal(nhits[keep], nh0) and best[keep].tobytes() == best0.tobytes()
    want = long_pair_answers
    assert np.array_equal(assign[[20, 41]], want["assign"]) and np.array_equal(nhits[[20, 41]], want["nhits"])
    assert best[[20, 41]].tobytes() == want["best"].tobytes()
    assert len(hit_off) == 43 and hit_off[0] == 0 and np.array_equal(np.diff(hit_off), nhits) and hit_off[-1] == len(hits)
    for k, r in enumerate(keep):
        assert hits[hit_off[r]:hit_off[r + 1]].tobytes() == hits0[off0[k]:off0[k + 1]].tobytes(), f"read {r}"
    for k, r in enumerate((20, 41)):
        assert hits[hit_off[r]:hit_off[r + 1]].tobytes() == want["hits"][want["hit_off"][k]:want["hit_off"][k + 1]].tobytes()
    # the counters cover both passes
    assert c1["gated_hits"] == int(nhits.sum()) and c1["minimizers"] > c0["minimizers"] + 2 * LIMIT // 8
    # ... and the next plain batch is a plain batch again
    a2, best2, nh2 = eng.classify(b, o, 60)
    off2, hits2 = eng.fetch_hits()
    assert np.array_equal(a2, a0) and np.array_equal(off2, off0) and hits2.tobytes() == hits0.tobytes()


def test_the_default_is_unchanged(capi, world):
    g = world["seqs"][0]
    exact = g[100_000:100_000 + LIMIT].copy()
    short = g[700_000:704_000].copy()
    bases, offsets = util.pack_reads([exact, short])
    fresh = capi.Engine(world["idx"], 0)
    try:
        assign, best, nhits = fresh.classify(bases, offsets, 60)
        assert assign.tolist() == [capi.SKIPPED, 0] and nhits.tolist() == [0, 1] and best[0].tolist() == (0, 0, 0, 0)
        fresh.set_long_reads(True)
        assign, best, nhits = fresh.classify(bases, offsets, 60)
        assert assign.tolist() == [0, 0] and best["mlen"].tolist() == [LIMIT, 4000]
        off, hits = fresh.fetch_hits()
        assert off.tolist() == [0, 1, 2] and hits["mlen"].tolist() == [LIMIT, 4000]
        fresh.set_long_reads(False)
        assign, best, nhits = fresh.classify(bases, offsets, 60)
        assert assign.tolist() == [capi.SKIPPED, 0] and nhits.tolist() == [0, 1]
        off, hits = fresh.fetch_hits()
        assert off.tolist() == [0, 0, 1]
    finally:
        fresh.close()


def test_chain_contract(capi, oracle, world, long_pair):
    """MNC_CONTRACT_CHAIN: regions, decisions and gated hits of the first errorful read equal the oracle's."""
    eng, oidx = world["eng"], world["oidx"]
    bases, offsets = util.pack_reads(long_pair[:1])
    try:
        eng.set_contract(capi.CONTRACT_CHAIN)
        oidx.opt.cigar = 0
        assign, best, nhits = eng.classify(bases, offsets, 60)
        regs = eng.dump(capi.DUMP_REGS, capi.REG_DTYPE)
        hit_off, hits = eng.fetch_hits()
        oregs = oidx.map(bases.tobytes())
        assert len(regs) == len(oregs) > 0
        for name in capi.REG_DTYPE.names:
            assert np.array_equal(regs[name], oregs[name]), name
        oassign, obest, onh, oflat = oidx.classify(bases, offsets, 60)
        assert np.array_equal(assign, oassign) and np.array_equal(nhits, onh) and assign[0] == 0
        for name in capi.HIT_DTYPE.names:
            assert np.array_equal(best[name], obest[name]) and np.array_equal(hits[name], oflat[name]), name
        assert ((regs["qs"] < LIMIT) & (regs["qe"] > LIMIT)).any()
    finally:
        eng.set_contract(capi.CONTRACT_DP)
        oidx.opt.cigar = 1


def test_device_entry_point(capi, world, long_pair_answers):
    """mnc_classify_device on device buffers, the whole call wide: the outputs of mnc_classify_batch."""
    import torch
    dev = torch.device("cuda:0")
    want = long_pair_answers
    bases, offsets = want["bases"], want["offsets"]
    eng = world["eng"]
    eng.set_contract(capi.CONTRACT_DP)
    pad = (-len(bases)) % 16 + 32
    d_bases = torch.from_numpy(np.concatenate([bases, np.zeros(pad, dtype=np.uint8)])).to(dev)
    d_off = torch.from_numpy(offsets).to(dev)
    d_assign = torch.full((2,), -9, dtype=torch.int32, device=dev)
    d_best = torch.zeros(2 * 4, dtype=torch.int32, device=dev)
    d_nhits = torch.zeros(2, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(len(world["idx"].genome_names) * 3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    eng.classify_device(d_bases.data_ptr(), d_off.data_ptr(), 2, int(offsets[-1]), int(np.diff(offsets).max()), 60,
                        d_assign.data_ptr(), d_best.data_ptr(), d_nhits.data_ptr(), d_counts.data_ptr())
    eng.sync()
    assert np.array_equal(d_assign.cpu().numpy(), want["assign"]) and np.array_equal(d_nhits.cpu().numpy(), want["nhits"])
    assert d_best.cpu().numpy().tobytes() == want["best"].tobytes()
    hit_off, hits = eng.fetch_hits()
    assert np.array_equal(hit_off, want["hit_off"]) and hits.tobytes() == want["hits"].tobytes()
    got = d_counts.cpu().numpy().reshape(-1, 3)
    for mode in (1, 2, 3):
        assert np.array_equal(got[:, mode - 1], capi.counts(world["idx"], want["assign"], want["best"], offsets, mode))
