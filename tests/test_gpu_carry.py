"""Abundance over a database of several index parts: the candidate carry on the device (mnc_carry_*, mnc_engine_carry_candidates,
mnc_abundance_create_global, mnc_abundance_add_carry; csrc/k_carry.hip).

Reference: tests/carryref.py -- the header's merge rule in plain dicts, pairs offered without the per-part pre-filter --
applied to the CPU ORACLE's regions of each part, and tests/abundref.py behind it.  Nothing is compared against the engine's
own dumps or export.  Rows are compared exactly, the EM bit for bit."""
import ctypes as C
import os
import pickle
import threading

import numpy as np
import pytest

import abundref
import carryref
import util
from monica_amd import synth
from test_gpu_abundance import World
from test_gpu_alignments import mutate

pytestmark = pytest.mark.gpu

ACGT = util.ACGT
MIN_MAPQ = 60
MAX_DELTA = 80


class Part:
    """One index part of the split world: the product's index and engine, the oracle's index, and where its genomes start."""

    def __init__(self, capi, oracle, names, seqs, genome_offset):
        self.names, self.seqs, self.genome_offset = names, seqs, genome_offset
        self.idx = capi.Index.from_seqs(names, seqs)
        self.oidx = oracle.Index.from_seqs(names, [s.tobytes() for s in seqs])
        self.oidx.opt.cigar = 1
        self.eng = capi.Engine(self.idx, 0)
        self.cg = [int(g) for g in self.idx.contig_genome]
        self.G = len(self.idx.genome_names)

    def oracle_regs(self, reads):
        return [self.oidx.map_cigar(np.asarray(rd, dtype=np.uint8).tobytes())[0] for rd in reads]


def reference(parts_pairs, width, max_delta, deliveries=None):
    """The rows after `deliveries` = [(part, first, last)] in that order (default: every part whole, in part order)."""
    n = len(parts_pairs[0])
    rows = [carryref.empty() for _ in range(n)]
    for p, a, b in deliveries or [(p, 0, n) for p in range(len(parts_pairs))]:
        for r in range(a, b):
            carryref.merge(rows[r], parts_pairs[p][r], width, max_delta)
    return rows


@pytest.fixture(scope="module")
def split(capi, oracle):
    """test_gpu_abundance.World's five contigs as two parts: part 0 = A, B and A's second contig (global genomes 0 and 1),
    part 1 = C and D (genome_offset 2); its ~150 reads; the oracle's regions of each part, computed once on the CPU, and
    checked to hold what the tests rely on."""
    w = World(capi, oracle)
    w.eng.close()
    parts = [Part(capi, oracle, [w.names[0], w.names[1], w.names[4]], [w.seqs[0], w.seqs[1], w.seqs[4]], 0),
             Part(capi, oracle, [w.names[2], w.names[3]], [w.seqs[2], w.seqs[3]], 2)]
    assert parts[0].G == 2 and parts[0].cg == [0, 1, 0] and parts[1].G == 2 and parts[1].cg == [0, 1]
    rng = np.random.default_rng(0xAB0D)
    reads = []
    for i in range(140):
        g = w.seqs[i % 5]
        n = int(rng.integers(1500, 2001))
        s = int(rng.integers(0, len(g) - n))
        rd = mutate(rng, g[s:s + n])
        reads.append(util.revcomp(rd) if rng.integers(0, 2) else rd)
    for i in range(8):
        reads.insert(int(rng.integers(0, len(reads) + 1)), ACGT[rng.integers(0, 4, 1800)])
    reads.append(np.concatenate([mutate(rng, w.seqs[1][2_000:2_900]), mutate(rng, w.seqs[0][52_000:53_200])]))
    reads = [reads[i] for i in rng.permutation(len(reads))]
    bases, offsets = util.pack_reads(reads)
    pairs = [[carryref.offered(regs, p.cg, p.genome_offset) for regs in p.oracle_regs(reads)] for p in parts]
    out = dict(parts=parts, reads=reads, bases=bases, offsets=offsets, pairs=pairs, n=len(reads), G=4,
               names=list(parts[0].idx.genome_names) + list(parts[1].idx.genome_names))
    check_the_world(out)
    return out


def check_the_world(split):
    """What keeps the tests honest, on the oracle's output alone, at max_delta 80."""
    pairs, n = split["pairs"], split["n"]
    rows = reference(pairs, 64, MAX_DELTA)
    cands = [carryref.candidates(r) for r in rows]
    assert sum(len(c) >= 2 for c in cands) >= 30, "rows of two or more candidates"
    assert sum(len(c) >= 3 for c in cands) >= 5, "rows with three candidates, so width = 2 truncates"
    assert sum(1 for c in cands if any(g < 2 for g, _ in c) and any(g >= 2 for g, _ in c)) >= 20, "rows whose candidates come from both parts"
    cut = [0, 0]                                                  # reads where a pair part p would keep is cut by the other part's higher best
    for r in range(n):
        for p in (0, 1):
            own = carryref.candidates(carryref.merge(carryref.empty(), pairs[p][r], 64, MAX_DELTA))
            cut[p] += any(g not in rows[r]["pairs"] for g, _ in own)
    assert cut[0] >= 5 and cut[1] >= 1, cut
    assert sum(1 for r in range(n) if not pairs[0][r] and not pairs[1][r]) >= 1, "a read with no record"
    assert any(d > 0 for c in cands for _, d in c)


def fetched(rows, width):
    """The reference rows as Carry.fetch returns them."""
    f = [carryref.fetched(r, width) for r in rows]
    return (np.array([x[0] for x in f], dtype=np.int32), np.array([x[1] for x in f], dtype=np.int32),
            np.array([x[2] for x in f], dtype=np.int32).reshape(len(f), width), np.array([x[3] for x in f], dtype=np.int32).reshape(len(f), width))


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def raw(fetch):
    return b"".join(a.tobytes() for a in fetch)


def check_carry(carry, rows, n_truncated=None):
    want = fetched(rows, carry.width)
    got = carry.fetch(0, len(rows))
    for name, g, w in zip(("count", "best", "genome", "score"), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (name, np.flatnonzero((g != w).reshape(len(rows), -1).any(axis=1))[:5])
    used, n_cands, trunc = carryref.info(rows)
    info = carry.info()
    assert info["cap_reads"] >= len(rows) and (info["n_rows_used"], info["n_cands"]) == (used, n_cands)
    assert info["n_truncated_reads"] == (trunc if n_truncated is None else n_truncated)
    return got


def collected(rows, G):
    """What a global accumulator holds after add_carry of these rows, in abundref's terms: (unique, sorted rows, n_reads)."""
    unique = np.zeros(G, dtype=np.int64)
    stored, n_reads = [], 0
    for c in (carryref.candidates(r) for r in rows):
        if not c:
            continue
        n_reads += 1
        if len(c) == 1:
            unique[c[0][0]] += 1
        else:
            stored.append(c)
    return unique, abundref.sort_rows(stored), n_reads


def held(ab):
    off, gen, dlt = ab.lists()
    return ab.unique(), abundref.csr_to_rows(off, gen, dlt), ab.info()


def classify(part, split, a=0, b=None):
    b = split["n"] if b is None else b
    off = split["offsets"]
    part.eng.classify(split["bases"][off[a]:off[b]], off[a:b + 1] - off[a], MIN_MAPQ)


# ---------------------------------------------------------------- 1. fetch equals the reference
def test_two_parts_equal_the_reference(capi, split):
    n, G = split["n"], split["G"]
    carry = capi.Carry(0, n)
    assert carry.device_bytes() >= n * (8 * 16 + 8) and carry.device_bytes() < n * (8 * 16 + 8) + (1 << 12)
    for part in split["parts"]:
        classify(part, split)
        part.eng.carry_candidates(carry, 0, part.genome_offset)
    rows = reference(split["pairs"], 16, MAX_DELTA)
    first = check_carry(carry, rows)
    assert raw(check_carry(carry, rows)) == raw(first)              # reading does not change it
    head, slots, cap, width = carry.device_rows()
    assert head and slots and cap == n and width == 16
    # ---- the rows into an accumulator for the genomes of both parts
    ab = capi.Abundance.global_(0, G, cap_cands=4096)
    ab.add_carry(carry, 0, n)
    unique, stored, n_reads = collected(rows, G)
    assert len(stored) >= 30 and int(unique.sum()) >= 20
    got_unique, got_rows, info = held(ab)
    assert got_unique.dtype == np.int64 and np.array_equal(got_unique, unique) and got_rows == stored
    assert info == dict(n_reads=n_reads, n_stored_reads=len(stored), n_cands=sum(len(r) for r in stored), n_dropped=0)
    theta, expected, iters = ab.solve()
    w_theta, w_expected, w_iters = abundref.solve(unique, stored, G)
    assert iters == w_iters and np.array_equal(theta, w_theta) and np.array_equal(expected, w_expected)
    assert raw(carry.fetch(0, n)) == raw(first)                     # the carry is left as it is
    # rows in two pieces = rows at once
    two = capi.Abundance.global_(0, G, cap_cands=4096)
    two.add_carry(carry, 0, 50), two.add_carry(carry, 50, n - 50)
    t2 = held(two)
    assert np.array_equal(t2[0], unique) and t2[1] == stored and t2[2] == info
    # a tighter cut
    tight = capi.Carry(0, n, max_delta=20)
    for part in split["parts"][::-1]:                               # (each part's engine still holds its batch)
        part.eng.carry_candidates(tight, 0, part.genome_offset)
    rows20 = reference(split["pairs"], 16, 20)
    check_carry(tight, rows20)
    assert carryref.info(rows20)[1] < carryref.info(rows)[1]
    for x in (ab, two, tight, carry):
        x.close()


# ---------------------------------------------------------------- 2. order and batch cut
def test_rows_do_not_depend_on_order_batch_cut_or_thread(capi, split):
    n = split["n"]
    p0, p1 = split["parts"]
    want = fetched(reference(split["pairs"], 16, MAX_DELTA), 16)
    c_rev, c_cut, c_twice, c_a, c_b = (capi.Carry(0, n) for _ in range(5))
    classify(p1, split)
    for c in (c_rev, c_twice, c_twice, c_b):                          # part 1 first; a part carried twice; part 1 alone
        p1.eng.carry_candidates(c, 0, 2)
    classify(p0, split)
    for c in (c_rev, c_cut, c_twice, c_a):                            # part 0 in one batch
        p0.eng.carry_candidates(c, 0, 0)
    for a, b in ((0, 7), (7, 71), (71, n)):                           # part 1 in batches of 7, 64 and the rest
        classify(p1, split, a, b)
        p1.eng.carry_candidates(c_cut, a, 2)
    for c in (c_rev, c_cut, c_twice):
        assert same(c.fetch(0, n), want)
        assert raw(c.fetch(0, n)) == raw(want)
    assert not same(c_a.fetch(0, n), want) and not same(c_b.fetch(0, n), want)
    c_a.merge(c_b)                                                    # two carries merged
    assert raw(c_a.fetch(0, n)) == raw(want)
    assert raw(c_b.fetch(0, n)) == raw(fetched(reference(split["pairs"], 16, MAX_DELTA, [(1, 0, n)]), 16))   # src as it was
    c_a.merge(c_b)
    assert raw(c_a.fetch(0, n)) == raw(want) and c_a.info()["n_truncated_reads"] == 0
    # two engines on two threads into one carry
    c_thr = capi.Carry(0, n)
    errors = []

    def run(part):
        try:
            classify(part, split)
            part.eng.carry_candidates(c_thr, 0, part.genome_offset)
            part.eng.sync()
        except BaseException as e:                                    # noqa: B036 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=run, args=(p,)) for p in (p0, p1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert raw(c_thr.fetch(0, n)) == raw(want)
    for c in (c_rev, c_cut, c_twice, c_a, c_b, c_thr):
        c.close()


# ---------------------------------------------------------------- 3. width 2 and width 1
@pytest.mark.parametrize("width", [2, 1])
def test_truncation(capi, split, width):
    n = split["n"]
    carry, back = capi.Carry(0, n, width=width), capi.Carry(0, n, width=width)
    p0, p1 = split["parts"]
    classify(p0, split), classify(p1, split)                          # (each part has its own engine, which keeps its batch)
    p0.eng.carry_candidates(carry, 0, 0)
    p1.eng.carry_candidates(carry, 0, 2)
    p1.eng.carry_candidates(back, 0, 2)
    p0.eng.carry_candidates(back, 0, 0)
    rows = reference(split["pairs"], width, MAX_DELTA)                # part 0, then part 1
    rows_back = reference(split["pairs"], width, MAX_DELTA, [(1, 0, n), (0, 0, n)])
    assert carryref.info(rows)[2] >= 5
    check_carry(carry, rows)                                          # n_truncated_reads: the reference simulated in the same order
    check_carry(back, rows_back)
    assert raw(carry.fetch(0, n)) == raw(back.fetch(0, n))
    # the rows are the closed form's
    for r, row in enumerate(rows):
        assert row["pairs"] == carryref.closed_form(split["pairs"][0][r] + split["pairs"][1][r], width, MAX_DELTA)
    carry.close(), back.close()


# ---------------------------------------------------------------- 4. without alignment, through add_lists
def csr(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, np.array([g for r in rows for g, _ in r], dtype=np.int32), np.array([s for r in rows for _, s in r], dtype=np.int32)


def via_add_lists(capi, deliveries, cap, width, max_delta):
    """deliveries: [(first_read, rows)]; the carry against carryref, delivery by delivery."""
    carry = capi.Carry(0, cap, width=width, max_delta=max_delta)
    ref = [carryref.empty() for _ in range(cap)]
    for first, rows in deliveries:
        carry.add_lists(first, *csr(rows))
        for r, row in enumerate(rows):
            carryref.merge(ref[first + r], row, width, max_delta)
        check_carry(carry, ref)
    return carry, ref


def test_add_lists_edges(capi):
    rng = np.random.default_rng(64)
    wide = [(g, int(rng.integers(900, 981))) for g in range(0, 130, 2)]                  # 65 genomes within 80 of one another
    # one read with 64 genomes at width 64, and with 65
    carry, ref = via_add_lists(capi, [(0, [wide[:64]])], 1, 64, 80)
    assert carry.info()["n_cands"] == 64 and carry.info()["n_truncated_reads"] == 0
    carry.close()
    carry, ref = via_add_lists(capi, [(0, [wide])], 1, 64, 200)
    assert carry.info()["n_cands"] == 64 and carry.info()["n_truncated_reads"] == 1
    carry.close()
    carry, ref = via_add_lists(capi, [(0, [wide[:40]]), (0, [wide[30:]])], 1, 64, 200)       # ... the 65th in a second delivery
    assert carry.info()["n_truncated_reads"] == 1
    carry.close()
    # a genome repeated with a lower and with a higher score; three reads, so a partial workgroup of waves
    carry, ref = via_add_lists(capi, [(0, [[(4, 100), (9, 90)], [(1, 50)], [(2, 7), (3, 7), (5, 7)]]),
                                      (0, [[(4, 60), (9, 95)], [(1, 70)], [(3, 6)]]),
                                      (1, [[(1, 160), (2, 80)], [(2, 9), (3, 1), (5, 7)]])], 3, 4, 80)
    assert carryref.fetched(ref[0], 4) == (2, 100, [4, 9, -1, -1], [100, 95, 0, 0])
    assert carryref.fetched(ref[1], 4) == (2, 160, [1, 2, -1, -1], [160, 80, 0, 0])
    carry.close()
    # equal scores: the tie goes to the smaller id, whichever comes first
    for rows in ([[(7, 50), (8, 50), (9, 50)]], [[(9, 50)]], ):
        carry, ref = via_add_lists(capi, [(0, rows), (0, [[(3, 50), (8, 50)]]), (0, [[(5, 50)]])], 1, 2, 10)
        assert sorted(ref[0]["pairs"]) == [3, 5] and ref[0]["truncated"]
        carry.close()
    # max_delta = 0: only the best's equals stay
    carry, ref = via_add_lists(capi, [(0, [[(1, 10), (2, 9), (6, 10)]]), (0, [[(0, 11)]]), (0, [[(3, 11), (4, 10)]])], 1, 8, 0)
    assert ref[0]["pairs"] == {0: 11, 3: 11} and not ref[0]["truncated"]
    carry.close()
    # first_read = cap_reads - n, negative scores, and rows that nobody touched stay empty
    carry, ref = via_add_lists(capi, [(5, [[(0, -5), (2, -90)], [(1, -2147483648), (3, 2147483647)], [(2, 0)]])], 8, 3, 80)
    assert carry.info()["n_rows_used"] == 3 and carry.fetch(0, 5)[0].tolist() == [0] * 5
    carry.close()
    # random rows against the reference, widths around the row lengths
    def rows():
        return [sorted({int(g): int(rng.integers(0, 40)) for g in rng.choice(12, size=int(rng.integers(1, 7)), replace=False)}.items()) for _ in range(300)]

    for width, max_delta in ((1, 80), (2, 0), (3, 15), (64, 80)):
        carry, ref = via_add_lists(capi, [(0, rows()), (0, rows()), (100, rows()[:200]), (0, rows())], 300, width, max_delta)
        carry.close()


# ---------------------------------------------------------------- 5. reserve, errors, capacity
def test_reserve_keeps_contents_and_empties_new_rows(capi):
    rows = [[(0, 5), (3, 9)], [(2, 1)], [(1, 4), (2, 4), (7, 3)]]
    carry, ref = via_add_lists(capi, [(0, rows)], 3, 4, 80)
    bytes3 = carry.device_bytes()
    carry.reserve(2)                                                  # nothing to do
    assert carry.info()["cap_reads"] == 3 and carry.device_bytes() == bytes3
    carry.reserve(1000)
    cap = carry.info()["cap_reads"]
    assert cap >= 1000 and carry.device_bytes() >= cap * 40
    check_carry(carry, ref + [carryref.empty() for _ in range(cap - 3)])
    carry.add_lists(cap - 1, *csr([[(6, 1)]]))
    assert carry.fetch(cap - 1, 1)[2].tolist() == [[6, -1, -1, -1]] and carry.info()["n_rows_used"] == 4
    carry.reset()
    assert carry.info() == dict(cap_reads=cap, n_rows_used=0, n_cands=0, n_truncated_reads=0) and not carry.fetch(0, cap)[0].any()
    carry.close()
    empty = capi.Carry(0, 0)                                          # a carry that starts with no rows, as the aligner's does
    assert empty.info()["cap_reads"] == 0
    empty.reserve(5)
    empty.add_lists(4, *csr([[(1, 1), (2, 1)]]))
    assert empty.fetch(0, 5)[0].tolist() == [0, 0, 0, 0, 2]
    empty.close()


def test_errors_leave_the_carry_untouched(capi, split):
    L = capi.lib()
    n = split["n"]
    p0, p1 = split["parts"]
    carry, ref = via_add_lists(capi, [(0, [[(0, 5), (3, 9)], [(2, 1)]])], 20, 4, 80)
    before = (raw(carry.fetch(0, 20)), carry.info())

    def unchanged():
        return (raw(carry.fetch(0, 20)), carry.info()) == before

    h = C.c_void_p()
    for args in ((-1, 16, 80), (10, 0, 80), (10, 65, 80), (10, 16, -1)):
        assert L.mnc_carry_create(0, *args, C.byref(h)) == capi.ERR_ARG and not h.value
    fresh = capi.Engine(p0.idx, 0)
    assert L.mnc_engine_carry_candidates(fresh._h, carry._h, 0, 0) == capi.ERR_ARG              # no batch has been classified
    fresh.set_contract(capi.CONTRACT_CHAIN)
    off = split["offsets"][:21]
    fresh.classify(split["bases"][:off[-1]], off, MIN_MAPQ)
    assert L.mnc_engine_carry_candidates(fresh._h, carry._h, 0, 0) == capi.ERR_ARG              # MNC_CONTRACT_CHAIN: no dp_max
    fresh.close()
    classify(p0, split, 0, 20)
    assert L.mnc_engine_carry_candidates(p0.eng._h, carry._h, -1, 0) == capi.ERR_ARG
    assert L.mnc_engine_carry_candidates(p0.eng._h, carry._h, 0, -1) == capi.ERR_ARG
    assert L.mnc_engine_carry_candidates(p0.eng._h, carry._h, 0, 2 ** 31 - 1) == capi.ERR_ARG   # a global id beyond int32
    assert L.mnc_engine_carry_candidates(p0.eng._h, carry._h, 1, 0) == capi.ERR_RANGE           # 1 + 20 > 20 rows
    assert L.mnc_engine_carry_candidates(p0.eng._h, carry._h, 1 << 40, 0) == capi.ERR_RANGE
    if capi.device_count() > 1:                                                                 # a carry on another device
        far = capi.Carry(1, 20)
        assert L.mnc_engine_carry_candidates(p0.eng._h, far._h, 0, 0) == capi.ERR_ARG
        far.close()
    assert unchanged()
    # add_lists: every malformed row, checked before anything is touched
    for rows in ([[(0, 1), (0, 2)]], [[(2, 1), (1, 1)]], [[(-1, 1), (1, 1)]], [[(0, 1), (1, 1)], [(3, 0), (3, 0)]]):
        o, g, s = csr(rows)
        assert L.mnc_carry_add_lists(carry._h, 0, len(rows), o.ctypes.data, g.ctypes.data, s.ctypes.data) == capi.ERR_ARG, rows
    o = np.array([0, 2, 2], dtype=np.int64)                                                      # an empty row
    g, s = np.array([0, 1], dtype=np.int32), np.zeros(2, dtype=np.int32)
    assert L.mnc_carry_add_lists(carry._h, 0, 2, o.ctypes.data, g.ctypes.data, s.ctypes.data) == capi.ERR_ARG
    assert L.mnc_carry_add_lists(carry._h, -1, 1, o.ctypes.data, g.ctypes.data, s.ctypes.data) == capi.ERR_ARG
    assert L.mnc_carry_add_lists(carry._h, 20, 1, o.ctypes.data, g.ctypes.data, s.ctypes.data) == capi.ERR_RANGE
    assert L.mnc_carry_fetch(carry._h, 19, 2, None, None, None, None) == capi.ERR_RANGE
    assert L.mnc_carry_fetch(carry._h, -1, 1, None, None, None, None) == capi.ERR_ARG
    # merge: another width, another max_delta, itself, more rows than dst has
    for other in (capi.Carry(0, 20, width=5), capi.Carry(0, 20, width=4, max_delta=79)):
        assert L.mnc_carry_merge(carry._h, other._h) == capi.ERR_ARG
        other.close()
    assert L.mnc_carry_merge(carry._h, carry._h) == capi.ERR_ARG
    big = capi.Carry(0, 21, width=4)
    assert L.mnc_carry_merge(carry._h, big._h) == capi.ERR_RANGE
    big.close()
    assert unchanged()
    # ---- the global accumulator's refusals
    ab = capi.Abundance.global_(0, 4, cap_cands=64)
    assert L.mnc_engine_add_abundance(p0.eng._h, ab._h) == capi.ERR_ARG                          # it is for no index
    assert L.mnc_abundance_add_carry(ab._h, carry._h, 0, 21) == capi.ERR_RANGE
    assert L.mnc_abundance_add_carry(ab._h, carry._h, -1, 1) == capi.ERR_ARG
    small = capi.Abundance.global_(0, 3, cap_cands=64)                                            # the carry holds genome 3
    assert L.mnc_abundance_add_carry(small._h, carry._h, 0, 20) == capi.ERR_ARG
    assert L.mnc_abundance_add_carry(small._h, carry._h, 1, 1) == capi.ERR_ARG                    # ... whichever rows are asked for
    other_delta = capi.Abundance.global_(0, 4, cap_cands=64, max_delta=70)
    assert L.mnc_abundance_add_carry(other_delta._h, carry._h, 0, 20) == capi.ERR_ARG
    nothing = dict(n_reads=0, n_stored_reads=0, n_cands=0, n_dropped=0)
    assert ab.info() == small.info() == other_delta.info() == nothing and not small.unique().any()
    ab.add_carry(carry, 0, 20)
    assert ab.info() == dict(n_reads=2, n_stored_reads=1, n_cands=2, n_dropped=0) and ab.unique().tolist() == [0, 0, 1, 0]
    assert ab.lists()[1].tolist() == [0, 3] and ab.lists()[2].tolist() == [4, 0]
    ab.add_lists(*abundref.rows_to_csr([[(1, 0)], [(0, 0), (1, 3)]]))                            # add_lists works on it unchanged
    assert ab.info() == dict(n_reads=4, n_stored_reads=2, n_cands=4, n_dropped=0)
    assert unchanged()
    for x in (ab, small, other_delta, carry):
        x.close()


def test_add_carry_into_a_short_accumulator_counts_dropped_rows(capi, split):
    n, G = split["n"], split["G"]
    rows = reference(split["pairs"], 16, MAX_DELTA)
    carry = capi.Carry(0, n)
    for p in (0, 1):                                                  # the oracle's pairs through add_lists: rows r with a pair, in runs
        r = 0
        while r < n:
            if not split["pairs"][p][r]:
                r += 1
                continue
            e = r
            while e < n and split["pairs"][p][e]:
                e += 1
            carry.add_lists(r, *csr(split["pairs"][p][r:e]))
            r = e
    check_carry(carry, rows)                                          # add_lists and the engines deliver the same rows
    unique, stored, n_reads = collected(rows, G)
    n_cands = sum(len(r) for r in stored)
    short = capi.Abundance.global_(0, G, cap_cands=n_cands - 1)
    short.add_carry(carry, 0, n)
    got_unique, got_rows, info = held(short)
    assert info["n_dropped"] >= 1 and info["n_cands"] <= n_cands - 1
    left = list(stored)                                               # nothing lies beyond the buffer: a sub-multiset of the reference's rows
    for r in got_rows:
        left.remove(r)
    assert info["n_stored_reads"] == len(got_rows) == len(stored) - info["n_dropped"] and info["n_cands"] == sum(len(r) for r in got_rows)
    assert info["n_reads"] == n_reads - info["n_dropped"] and np.array_equal(got_unique, unique)
    with pytest.raises(capi.MncError) as err:
        short.solve()
    assert err.value.code == capi.ERR_RANGE
    enough = capi.Abundance.global_(0, G, cap_cands=n_cands)
    enough.add_carry(carry, 0, n)
    assert held(enough)[1] == stored and enough.info()["n_dropped"] == 0
    for x in (short, enough, carry):
        x.close()


def test_a_mixed_call_of_long_and_short_reads_is_refused(capi):
    n = (1 << 20) + 5000
    g = synth.genome(0x5151, 1_100_000)
    idx = capi.Index.from_seqs([synth.contig_name(0)], [g])
    eng = capi.Engine(idx, 0)
    eng.set_long_reads(True)
    carry = capi.Carry(0, 2)
    assign, _, _ = eng.classify(*util.pack_reads([g[20_000:20_000 + n].copy(), g[500_000:502_000]]), MIN_MAPQ)
    assert assign.tolist() == [0, 0]
    assert capi.lib().mnc_engine_carry_candidates(eng._h, carry._h, 0, 0) == capi.ERR_UNSUPPORTED   # the engine holds the wide pass alone
    assert carry.info() == dict(cap_reads=2, n_rows_used=0, n_cands=0, n_truncated_reads=0)
    carry.close(), eng.close()


# ---------------------------------------------------------------- 6. files
def test_the_aligner_loop_on_two_parts(capi, split, tmp_path, monkeypatch, capsys):
    from monica_amd import aligner
    n, G = split["n"], split["G"]
    dbs = tmp_path / "databases"
    dbs.mkdir()
    for k, part in enumerate(split["parts"]):
        synth.write_fasta(str(dbs / f"database{k}.fna.gz"), part.names, part.seqs)
    paths = sorted(aligner.indexer(str(dbs), str(tmp_path / "indexes")))
    assert len(paths) == 2
    monkeypatch.setattr(aligner, "BATCH_READS", 60)
    monkeypatch.setattr(aligner, "BATCH_RAMP", (1.0,))
    monkeypatch.setattr(aligner, "PIPE_TRACE", [])
    listing, pkl = {}, {}
    # (width 2, so that reads are truncated and the run says so; the default width is test_two_parts_equal_the_reference's)
    for label, kw in (("plain", {}), ("abundance", dict(abundance={"across_parts": True, "width": 2}))):
        query, outdir = tmp_path / f"query {label}", tmp_path / f"output {label}"
        query.mkdir(), outdir.mkdir()
        synth.write_fastq(str(query / "s.fastq"), split["bases"], split["offsets"], ids=[f"r{i}" for i in range(n)])
        cwd = os.getcwd()
        try:
            aligner.multi_threaded_aligner(str(query), paths, mode="basic", mapping_quality=MIN_MAPQ, n_threads=1, output_folder=str(outdir), **kw)
        finally:
            os.chdir(cwd)
        listing[label] = {os.path.relpath(os.path.join(d, f), query): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(query) for f in fs}
        pkl[label] = (outdir / "alignment.pkl").read_bytes()
    assert sum(1 for t in aligner.PIPE_TRACE if t[0] == "classify") >= 8, "one batch only"
    csv = os.path.join("mapped", "s.abundance.csv")
    said = capsys.readouterr().out
    assert said.count("abundance width = 2") == 1                     # truncated reads: said once per sample, with the width
    for label, width in (("abundance", 2),):
        assert csv not in listing["plain"] and sorted(listing[label]) == sorted(list(listing["plain"]) + [csv])
        for name, data in listing["plain"].items():                   # every other output file is byte-identical
            assert listing[label][name] == data, name
        assert pkl["plain"] == pkl[label] and pickle.loads(pkl["plain"])
        unique, stored, _ = collected(reference(split["pairs"], width, MAX_DELTA), G)
        theta, expected, _ = abundref.solve(unique, stored, G)
        lines = listing[label][csv].decode().splitlines()
        assert lines[0] == "genome,theta,expected_reads,unique_reads" and len(lines) == 1 + G
        for g, line in enumerate(lines[1:]):
            name, t, e, u = line.split(",")
            assert name == split["names"][g] and float(t) == theta[g] and float(e) == expected[g] and int(u) == unique[g]
    assert any(name.endswith("fastq") and data for name, data in listing["plain"].items())
    # a genome name that occurs in two parts: a ValueError naming it, and no abundance file
    dup = tmp_path / "dup databases"
    dup.mkdir()
    synth.write_fasta(str(dup / "database0.fna.gz"), split["parts"][0].names, split["parts"][0].seqs)
    synth.write_fasta(str(dup / "database1.fna.gz"), [split["parts"][1].names[0], split["parts"][0].names[1]], split["parts"][1].seqs)
    dup_paths = sorted(aligner.indexer(str(dup), str(tmp_path / "dup indexes")))
    query = tmp_path / "query dup"
    query.mkdir()
    synth.write_fastq(str(query / "s.fastq"), split["bases"][:split["offsets"][20]], split["offsets"][:21], ids=[f"r{i}" for i in range(20)])
    cwd = os.getcwd()
    try:
        with pytest.raises(ValueError, match="occurs in two index parts") as err:
            aligner.multi_threaded_aligner(str(query), dup_paths, mode="basic", mapping_quality=MIN_MAPQ, n_threads=1, output_folder=str(tmp_path),
                                           abundance={"across_parts": True})
    finally:
        os.chdir(cwd)
    assert split["parts"][0].idx.genome_names[1] in str(err.value)
    assert not [f for d, _, fs in os.walk(query) for f in fs if f.endswith("abundance.csv")]
