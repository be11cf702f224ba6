"""Every kernel call of the base-level alignment stage (csrc/k_align.hip, csrc/k_fill.hip) against ksw2's literal form with the
call's own inputs (tests/segments.py), on batches built so that calls sit on both sides of every limit of plan_seg_class -- the
whole-pipeline comparison of test_gpu_dp.py sees a kernel's result only where a later step happens to consume it, and which
kernel sees which shape there is an accident of the seeds.

How the shapes are placed.  mm_align1 cuts a region's calls at seed mid-points: a 15-mer that is the smallest of the ten that
START at it is a minimizer of the contig and of any read that holds those 24 bases, whatever precedes them (`_starts`); one that
is the smallest of the ten that END at it likewise (`_ends`).  A read whose matching stretch starts / ends with such a 15-mer has
its first / last seed there, so the extension beside it has qlen = flank + 7 (left) or flank + 8 (right) exactly -- which is
also why no extension is shorter than 7 bases -- and a gap filling between two such 15-mers at contig positions a and b with
fewer than 200 matching bases in front has tlen = b - a exactly (mm_align1 fills once 200 bases have gone by)."""
import numpy as np
import pytest

from monica_amd import synth
import segments
import util
from test_gpu_parity import _compare_dp, _world_from

K = 15


@pytest.fixture(scope="module")
def world(capi, oracle):
    names, seqs = util.small_genomes()
    return _world_from(capi, oracle, names, seqs)


def _classify_and_replay(capi, oracle, world, bases, offsets, cache=None, with_cigars=False):
    eng = world["eng"]
    eng.set_contract(capi.CONTRACT_DP)
    eng.classify(bases, offsets, 0)
    return segments.replay(capi, oracle, world, bases, offsets, cache=cache, with_cigars=with_cigars)


def _summary(name, segs):
    kinds = {k: int((segs["kind"] == k).sum()) for k in (0, 1, 2)}
    print(f"{name}: {len(segs)} calls replayed (left ext {kinds[0]}, gap fillings {kinds[1]}, right ext {kinds[2]}); "
          f"classes {sorted(set(segs['big'].tolist()))}")


def _minimizer_starts(oracle, piece):
    mz = oracle.sketch(piece.tobytes())
    return ((mz["y"] & 0xffffffff) >> 1).astype(np.int64) - (K - 1)


def _starts(oracle, g, p):
    """The 15-mer at g[p:p+15] is the minimizer of the window of ten 15-mers that starts at it."""
    return 0 in _minimizer_starts(oracle, g[p:p + K + 9]).tolist()


def _ends(oracle, g, p):
    """... of the window of ten that ends at it."""
    return 9 in _minimizer_starts(oracle, g[p - 9:p + K]).tolist()


def _other(base):
    """A base that is not `base`: the read's base next to an anchoring 15-mer, so that no 15-mer across the junction matches."""
    return util.ACGT[(int(np.searchsorted(util.ACGT, base)) + 1) % 4]


# ---------------------------------------------------------------- (a)
@pytest.mark.gpu
def test_every_call_of_noisy_reads_replays(capi, oracle, world):
    total = 0
    for name, rate in (("2 %", (100, 50, 50)), ("10 %", (400, 300, 300)), ("16 %", (700, 450, 450))):
        b, o, _ = synth.reads(world["seqs"], 40, 3000, seed=31, sub=rate[0], ins=rate[1], dele=rate[2])
        segs = _classify_and_replay(capi, oracle, world, b, o)
        _summary(f"noisy reads at {name}", segs)
        assert len(segs) >= 40
        total += len(segs)
    b, o = util.pack_reads(util.edge_reads(world["seqs"], np.random.default_rng(7)))
    _compare_dp(capi, oracle, world, b, o, min_mapq=0)
    segs = segments.replay(capi, oracle, world, b, o)
    _summary("edge reads", segs)
    assert len(segs) >= 20 and total > 1000


# ---------------------------------------------------------------- (b)
GAP_ADS = (37, 38, 39, 40, 57, 58, 59, 60, 109, 110, 111, 112, 493, 494, 495, 496, 500)
L_SMALL, L_LONG = 260, 1200            # gap fillings of L + (up to ~230, see below) bases: within 511; within 512 .. 2047 with any of the indels


def _gap_reads(oracle, g, rng):
    """-> reads, [(what, value)] per read."""
    reads, what = [], []
    ms = _minimizer_starts(oracle, g)
    ms_set = set(ms.tolist())
    # exact lengths, no indel: 100 matching bases from contig position a (too few for a gap filling of their own), the stretch up
    # to b at 90 % identity without a shared 15-mer, 1 500 matching bases from b on: one gap filling of b - a bases on both sides
    for lo, hi in ((482, 542), (2018, 2078)):
        for v in range(lo, hi):
            for a in ms[(ms > 20_000) & (ms < len(g) - 10_000)][(v * 37) % 97::7]:
                a = int(a)
                if a + v in ms_set and _starts(oracle, g, a) and _starts(oracle, g, a + v):
                    break
            else:
                raise AssertionError(f"no pair of anchoring 15-mers {v} bases apart")
            mid = util.sparse(g[a + 100:a + v], rng)
            mid[-1] = _other(g[a + v - 1])
            if v % 16 == 5:
                mid[len(mid) // 3] = ord("N")
            reads.append(np.concatenate([g[a:a + 100], mid, g[a + v:a + v + 1500]]))
            what.append(("len", v))
    # one indel of `ad` bases in the middle of a stretch of L such bases between flanks of 1 500: |tlen - qlen| = ad exactly; the
    # call reaches from the last seed at which mm_align1 filled (up to 200 bases and a seed before the stretch) to the first seed behind it
    for L, a in ((L_SMALL, 60_000), (L_LONG, 90_000)):
        for ad in GAP_ADS:
            if ad >= L:
                continue
            for sign in (-1, 1):
                mid = util.sparse(g[a + 1500:a + 1500 + L], rng)
                c = L // 2
                if sign < 0:
                    mid = np.concatenate([mid[:c - ad // 2], mid[c - ad // 2 + ad:]])
                else:
                    mid = np.concatenate([mid[:c], util.ACGT[rng.integers(0, 4, ad)], mid[c:]])
                if ad in (38, 494):
                    mid[7] = ord("N")
                reads.append(np.concatenate([g[a:a + 1500], mid, g[a + 1500 + L:a + 3000 + L]]))
                what.append(("ad", sign * ad))
    reads = [util.revcomp(r) if i % 4 == 3 else r for i, r in enumerate(reads)]
    return reads, what


@pytest.mark.gpu
def test_gap_fillings_on_both_sides_of_every_class_limit(capi, oracle, world):
    g = world["seqs"][0]
    reads, what = _gap_reads(oracle, g, np.random.default_rng(511))
    bases, offsets = util.pack_reads(reads)
    eng = world["eng"]
    cache, tables, ctr, classes = {}, [], [], set()
    routes = (0, 20 << 8 | 20 << 24, 48 << 8 | 48 << 24, 0x80000000, 0x40000, 0x80000)
    try:
        for route in routes:
            eng.set_debug(route)
            segs, words = _classify_and_replay(capi, oracle, world, bases, offsets, cache=cache, with_cigars=True)
            _summary(f"gap fillings, route {route:#x}", segs)
            tables.append(segments.results_table(segs, words))
            ctr.append(eng.counters())
            fill = segs[segs["kind"] == 1]
            classes |= set(fill["big"].tolist())
            if route == 0:
                default = fill
    finally:
        eng.set_debug(0)
    # ---- the shapes, from the dump
    mx, mn = np.maximum(default["tlen"], default["qlen"]), np.minimum(default["tlen"], default["qlen"])
    ad = np.abs(default["tlen"] - default["qlen"])
    print("gap fillings: longest side", sorted(set(mx.tolist()))[-8:], " |tlen - qlen|:", sorted(set(ad[ad > 30].tolist())))
    for v in (511, 512, 2047, 2048):
        assert (mx == v).any(), f"no gap filling of {v} bases"
    for i, (kind, v) in enumerate(what):                       # the exact-length reads: one gap filling of exactly that length
        if kind == "len":
            mine = default[(default["read"] == i) & (default["tlen"] == v) & (default["qlen"] == v)]
            # (one in each region of the read: a stretch that two contigs share gives two regions)
            assert len(mine) >= 1 and len(mine) == len(set(mine["reg"].tolist())), \
                f"read {i}: no single gap filling of {v} x {v} bases: {default[default['read'] == i][['reg', 'tlen', 'qlen']].tolist()}"
    for a_ in GAP_ADS:
        if a_ < L_SMALL:
            assert ((ad == a_) & (mx <= 511)).any(), f"no gap filling with |tlen - qlen| = {a_} within 511 bases"
        assert ((ad == a_) & (mx >= 512) & (mx <= 2047)).any(), f"no gap filling with |tlen - qlen| = {a_} and a side of 512 .. 2047 bases"
    # ---- the classes: as planned by default the four banded tiers, the long-gap kernel and the literal kernel's large workspace
    # (2 048 bases); with the packed kernels taken out the literal kernel's small classes.  (3 and 0 of segments.GAP_CLASSES: calls
    # of more than 8 MB of direction bytes / more than 1e8 cells, tens of thousands of bases)
    assert {4, 21, 5, 9, 22, 1} <= set(default["big"].tolist()), sorted(set(default["big"].tolist()))
    assert set(segments.GAP_CLASSES) - {3, 0} <= classes, sorted(classes)
    # ---- the same results from every route, call for call
    for route, t in zip(routes[1:], tables[1:]):
        assert len(t) == len(tables[0]), f"route {route:#x}: {len(t)} calls, {len(tables[0])} by default"
        for x, y in zip(tables[0], t):
            assert x == y, f"route {route:#x}: call {x[0]}: {y[1]} != {x[1]} by default"
    for k in ("dp_fill_tier1", "dp_fill_tier_mid", "dp_fill_tier2", "dp_fill_tier3", "dp_long_gaps"):
        assert any(c[k] > 0 for c in ctr), k


# ---------------------------------------------------------------- (c)
EXT_FLANKS = (list(range(0, 71)) + list(range(119, 124)) + list(range(247, 252)) + list(range(366, 373)) + list(range(500, 525))
              + list(range(740, 765)) + list(range(1525, 1546)) + [2000, 3000])
# (119 .. 123, 247 .. 251, 366 .. 372: qlen 128 | 129 and 256 | 257, the packed extension kernel's last two shapes, and tlen =
# 2 qlen - 2 on both sides of the band, 751: the calls of the 256-cell shapes and of the long-extension kernel)


def _ext_reads(oracle, g, rng):
    a = next(p for p in range(100_000, 130_000) if _starts(oracle, g, p) and _ends(oracle, g, p + 2000 - K))
    core = g[a:a + 2000]
    reads, kinds = [], []
    for F in EXT_FLANKS:
        for left_sparse in (True, False):
            junk = lambda: util.ACGT[rng.integers(0, 4, F)]
            left = util.sparse(g[a - F:a], rng) if left_sparse else junk()
            right = junk() if left_sparse else util.sparse(g[a + 2000:a + 2000 + F], rng)
            if F:
                left[-1], right[0] = _other(g[a - 1]), _other(g[a + 2000])
            r = np.concatenate([left, core, right])
            rc = (len(reads) % 4) in (1, 2)
            reads.append(util.revcomp(r) if rc else r)
            # flank kind of the call of kind 0 / 2 (on a reverse-strand read the left extension is the read's right flank)
            lk, rk = ("sparse", "random") if left_sparse else ("random", "sparse")
            kinds.append({0: lk, 2: rk, "F": F})
    return reads, kinds


@pytest.mark.gpu
def test_extensions_on_both_sides_of_every_class_limit(capi, oracle, world):
    g = world["seqs"][0]
    reads, kinds = _ext_reads(oracle, g, np.random.default_rng(751))
    bases, offsets = util.pack_reads(reads)
    eng = world["eng"]
    cache, classes, tables = {}, set(), []
    routes = (0, 0x20000, 0x100000, 0x8, 0x1)
    try:
        for route in routes:
            eng.set_debug(route)
            segs, words = _classify_and_replay(capi, oracle, world, bases, offsets, cache=cache, with_cigars=True)
            _summary(f"extensions, route {route:#x}", segs)
            tables.append(segments.results_table(segs, words))
            ext = segs[segs["kind"] != 1]
            classes |= set(ext["big"].tolist())
            if route == 0:
                default = ext
    finally:
        eng.set_debug(0)
    ql = set(default["qlen"].tolist())
    print("extensions: qlen", sorted(ql))
    # (mm_align1 starts at seed mid-points: a left extension has at least 7, a right one at least 8 query bases)
    missing = [v for v in list(range(7, 65)) + [512, 513, 751, 752] if v not in ql]
    assert not missing, f"no extension with qlen {missing}"
    span = default["tlen"] + default["qlen"] - 1
    assert (span <= 3070).any() and (span > 3070).any() and ((default["tlen"] <= default["w"]) & (default["qlen"] > 256)).any()
    # reach_end: ksw_extd2 sets it when mqe + end_bonus > max, and mqe <= max -- with minimap2's end bonus for these reads (-1,
    # oidx.opt) the oracle never gives it, so neither may a kernel; with a positive one both values must show.  What tells the
    # flank kinds apart either way: a flank at 90 % identity is aligned to the read's end, a random one stops within a few bases
    seen = {"sparse": set(), "random": set()}
    for s in default:
        k = kinds[int(s["read"])]
        if k["F"] >= 100:
            seen[k[int(s["kind"])]].add("end" if int(s["max_q"]) >= int(s["qlen"]) - 12 else "start" if int(s["max_q"]) < 50 else "between")
    reach = set(default["reach_end"].tolist())
    print("extensions: best cell by flank kind", seen, " reach_end", reach, " Z-dropped:", int((default["zdropped"] != 0).sum()))
    assert seen == {"sparse": {"end"}, "random": {"start"}}, seen      # (a base changed every ten: the best cell within ten bases of the end)
    assert reach == ({0} if world["oidx"].opt.end_bonus <= 0 else {0, 1}), reach
    assert (default["zdropped"] != 0).any()
    # (8: nothing as small as the literal kernel's first pass takes is left by the extension kernels; 3, 0: as for the gap fillings)
    assert set(segments.EXT_CLASSES) - {8, 3, 0} <= classes, sorted(classes)
    for route, t in zip(routes[1:], tables[1:]):
        assert t == tables[0], f"route {route:#x}: the compared fields differ from the default run's"


# ---------------------------------------------------------------- (d)
def test_replay_names_the_call(oracle):
    rng = np.random.default_rng(3)
    t = rng.integers(0, 4, 120).astype(np.uint8)
    q = np.concatenate([t[:20], (t[20:21] + 1) % 4, t[21:40], rng.integers(0, 4, 20).astype(np.uint8)])
    opt = oracle.default_opt()
    mat = oracle.simple_mat(opt.a, opt.b, opt.sc_ambi)
    flag = oracle.EZ_EXTZ_ONLY
    want = segments.expected(oracle, opt, mat, 2, q, t, 751, opt.zdrop, flag)
    assert want["n_cigar"] > 0 and want["max_t"] >= 39 and want["reach_end"] == 0
    row = dict(read=17, reg=0, kind=2, rid=1, rev=0, ts=1000, tlen=len(t), qs=2000, qlen=len(q), w=751, zdrop=opt.zdrop, flag=flag, ai=0, big=14,
               cig_off=0, zdrop_code=0, **{k: want[k] for k in ("n_cigar", "zdropped", "max", "max_t", "max_q", "score", "reach_end", "mqe_t")})
    segments.compare_call(row, want["cigar"], want)                      # the call as the oracle has it passes
    row["score"] = 12345                                                 # a field no later step reads on an extension
    segments.compare_call(row, want["cigar"], want)
    row["max_t"] += 1
    with pytest.raises(AssertionError) as e:
        segments.compare_call(row, want["cigar"], want)
    msg = str(e.value)
    assert "big=14" in msg and "packed extension, 64 cells" in msg and "right extension" in msg and "read 17" in msg
    assert f"(tlen, qlen, w, zdrop, flag)=(120, 60, 751, {opt.zdrop}, 0x40)" in msg
    assert f"field max_t: kernel {want['max_t'] + 1} != ksw_extd2 {want['max_t']}" in msg
    row["max_t"] -= 1
    with pytest.raises(AssertionError, match="field cigar"):
        segments.compare_call(row, want["cigar"][:-1] + [want["cigar"][-1] + 16], want)
    # the table covers every result field of every outcome, compared or excluded with a reason
    for key, fields in segments.COMPARED.items():
        assert set(fields) - {"cigar"} | set(segments.EXCLUDED[key]) == set(segments.RESULT_FIELDS), key
