"""Replay of the alignment stage's kernel calls against ksw2's literal form, call by call.

The engine files one `Seg` per ksw_extd2 call of mm_align1 (MNC_DUMP_SEGS: inputs, planned kernel class `big`, results) and
keeps the calls' CIGARs in a pool of their own (MNC_DUMP_SEG_CIGARS).  `replay` rebuilds every call's two sequences from the
contigs and the reads, runs `pyoracle.ksw_extd2` -- the oracle's literal simulation of the SSE kernel -- with exactly the
call's band, Z-drop and flags, and compares the result fields the stitch kernel (mnc_dp_stitch, csrc/k_align.hip) reads for a
call of that kind and outcome, on EVERY such call, whichever kernel ran it and whether or not a later step happened to consume
the field.  A mismatch names the kernel class, the call's shape and the field.

A gap filling is mm_align1's pair of calls: the first pass with the segment's flag (KSW_EZ_APPROX_MAX), mm_test_zdrop on its
CIGAR, and -- when that answers 1 or 2 -- the exact pass with flag 0 and zdrop / zdrop_inv (oracle/mm_align.c: align1); the Seg
holds the result of the last pass run and the test's answer (`zdrop_code`).  mm_test_zdrop is restated here (`zdrop_test`).

Inversions: the extension mm_align1_inv makes from the start its local alignment found IS filed as a Seg (kind 2, on the other
strand, band (int)(bw * 1.5)) and is replayed like any other; the local alignment itself (ksw_ll_i16, mnc_dp_inv) is no
ksw_extd2 call, is not in the dump and is out of scope here.
"""
import numpy as np

KIND_NAMES = ("left extension", "gap filling", "right extension")
SEG_NEEDS_BIG_WS, SEG_SKIPPED = 0x10000, 0x20000          # Seg.flag bits of the engine's own (csrc/device.h), above ksw2's EZ_* bits
EZ_MASK = 0xffff
NEG_INF = -0x40000000

# Seg.big as plan_seg_class (csrc/k_align.hip) sets it: the kernel a call is planned for
CLASS_NAMES = {0: "not aligned (beyond max_sw_mat / every workspace)", 1: "literal kernel, large workspace", 3: "literal kernel, largest workspace",
               4: "banded gap filling, 32 cells", 21: "banded gap filling, 42 cells", 5: "banded gap filling, 64 cells", 9: "banded gap filling, 128 cells",
               22: "long gap filling, int32 band", 8: "literal kernel, first pass (LDS)", 20: "literal kernel, small workspace",
               6: "step-by-step extension, 32", 7: "step-by-step extension, 64", 10: "step-by-step extension, 128", 11: "step-by-step extension, 256",
               12: "packed extension, 32 cells", 13: "packed extension, 32 cells, gaps right-aligned", 14: "packed extension, 64 cells", 15: "packed extension, 64 cells, gaps right-aligned",
               16: "packed extension, 128 cells", 17: "packed extension, 128 cells, gaps right-aligned", 18: "packed extension, 256 cells", 19: "packed extension, 256 cells, gaps right-aligned",
               23: "long extension"}
# the classes plan_seg_class can give a gap filling / an extension.  (0 and 3 need tlen x qlen > max_sw_mat = 1e8 or more than
# 8 MB of direction bytes: calls of tens of thousands of bases, which no quick test makes.)
GAP_CLASSES = (4, 21, 5, 9, 22, 8, 20, 1, 3, 0)
EXT_CLASSES = (12, 13, 14, 15, 16, 17, 18, 19, 6, 7, 10, 11, 23, 8, 20, 1, 3, 0)

# ---------------------------------------------------------------- what is compared
# Per (call, zdropped, reach_end) of the ORACLE's result: the fields mnc_dp_stitch reads for such a call in any branch.  "cigar"
# stands for the n_cigar words at cig_off of the per-call pool, compared word for word.
COMPARED = {
    ("gap", 0, 0): ("zdropped", "score", "n_cigar", "cigar"),
    ("gap", 1, 0): ("zdropped", "max", "max_t", "max_q", "zdrop_code", "n_cigar", "cigar"),
    ("ext", 0, 0): ("zdropped", "reach_end", "max", "max_t", "max_q", "n_cigar", "cigar"),
    ("ext", 1, 0): ("zdropped", "reach_end", "max", "max_t", "max_q", "n_cigar", "cigar"),
    ("ext", 0, 1): ("zdropped", "reach_end", "max", "max_t", "max_q", "mqe_t", "n_cigar", "cigar"),
}
# ... and every field left out, with the place in mnc_dp_stitch that shows nothing reads it on such a call (the banded gap-filling
# kernels of k_fill.hip leave max / max_t / max_q as planned on a gap filling they accept; the packed extension kernels leave score)
EXCLUDED = {
    ("gap", 0, 0): {
        "max": "the region's score takes `sg[k].zdropped ? sg[k].max : sg[k].score`: score when not dropped",
        "max_t": "read only under `if (dropped)` (`re1 = prs + (g.max_t + 1)`, the seed search before it)",
        "max_q": "read only under `if (dropped)` (`qe1 = pqs + (g.max_q + 1)`)",
        "zdrop_code": "read only under `if (dropped)` (`split_inv = g.zdrop_code == 2`)",
        "reach_end": "read of sg[0] under `d.has_left` and of sg[n_seg - 1] under `d.has_right` only: extensions",
        "mqe_t": "as reach_end",
    },
    ("gap", 1, 0): {
        "score": "the region's score takes `sg[k].zdropped ? sg[k].max : sg[k].score`: max when dropped",
        "reach_end": "read of sg[0] under `d.has_left` and of sg[n_seg - 1] under `d.has_right` only: extensions",
        "mqe_t": "as reach_end",
    },
    ("ext", 0, 0): {
        "score": "`if (!is_fill) term = nk > 0 ? sg[k].max : 0`: an extension adds its max, never its score",
        "zdrop_code": "`split_inv = g.zdrop_code == 2` reads the gap filling that dropped (sg[stop - 1]) only",
        "mqe_t": "`g.reach_end ? g.mqe_t + 1 : g.max_t + 1`: read only when reach_end is set",
    },
}
EXCLUDED[("ext", 1, 0)] = EXCLUDED[("ext", 0, 0)]
EXCLUDED[("ext", 0, 1)] = {k: v for k, v in EXCLUDED[("ext", 0, 0)].items() if k != "mqe_t"}
RESULT_FIELDS = ("n_cigar", "zdropped", "zdrop_code", "max", "max_t", "max_q", "score", "reach_end", "mqe_t")
# a call the stage does not run (SEG_SKIPPED, tlen x qlen > max_sw_mat): ksw_reset_extz + zdropped, as dp_align_queue writes it
NOT_RUN = dict(n_cigar=0, zdropped=1, zdrop_code=0, max=0, max_t=-1, max_q=-1, score=NEG_INF, reach_end=0, mqe_t=-1)

_NT4 = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate((b"Aa", b"Cc", b"Gg", b"TtUu")):
    for _b in _c:
        _NT4[_b] = _i


def codes(ascii_bases):
    """ASCII -> 0..4 (anything but ACGTU / acgtu is 4)."""
    return _NT4[np.asarray(ascii_bases, dtype=np.uint8)]


def revcomp_codes(c):
    c = c[::-1]
    return np.where(c < 4, 3 - c, 4).astype(np.uint8)


def cigar_words(cig):
    """pyoracle's [(len, 'M' | 'I' | 'D'), ...] -> uint32 len << 4 | op."""
    return [ln << 4 | "MID".index(op) for ln, op in cig]


def zdrop_test(oracle, opt, mat, q, t, words):
    """mm_test_zdrop on a finished CIGAR (oracle/mm_align.c: test_zdrop), the walk as array operations.
    0: fine; 1: the score drops by more than zdrop; 2: and the dropped stretch aligns to its own reverse complement."""
    if not words:
        return 0
    sc, ii, jj = [], [], []
    i = j = 0
    for wd in words:
        op, ln = wd & 0xf, wd >> 4
        if op == 0:
            sc.append(mat[t[i:i + ln].astype(np.int64) * 5 + q[j:j + ln]].astype(np.int64))
            ii.append(np.arange(i, i + ln)), jj.append(np.arange(j, j + ln))
            i, j = i + ln, j + ln
        else:
            if op == 1:
                j += ln
            else:
                i += ln
            sc.append(np.array([-(opt.q + opt.e * ln)], dtype=np.int64))      # (the reference scores a gap after moving past it)
            ii.append(np.array([i])), jj.append(np.array([j]))
    score, I, J = np.cumsum(np.concatenate(sc)), np.concatenate(ii), np.concatenate(jj)
    n = len(score)
    prev_max = np.concatenate([[-(1 << 40)], np.maximum.accumulate(score)[:-1]])         # (INT32_MIN there: below any score)
    below = score < prev_max
    at = np.maximum.accumulate(np.where(below, -1, np.arange(n)))         # the event that holds the running maximum (ties move it on)
    z = np.where(below, prev_max - score - np.abs((I - I[at]) - (J - J[at])) * opt.e, 0)
    k = int(np.argmax(z))                                                  # the first event with the largest drop
    max_zdrop = int(z[k])
    if max_zdrop > 0:
        t0, t1, q0, q1 = int(I[at[k]]), int(I[k]) + 1, int(J[at[k]]), int(J[k]) + 1
    else:
        t0 = t1 = q0 = q1 = -1
    q_len, t_len = q1 - q0, t1 - t0
    if max_zdrop > opt.zdrop_inv and q_len < opt.max_gap and t_len < opt.max_gap:
        q2 = np.ascontiguousarray(revcomp_codes(q[q1 - q_len:q1])) if q_len > 0 else np.zeros(1, dtype=np.uint8)
        tt = np.zeros(max(t_len, 1), dtype=np.uint8)                       # (a gap at the very end: the reference's window is one base longer than the call's target)
        tt[:max(0, min(t_len, len(t) - t0))] = t[t0:t0 + t_len]
        s = oracle.lib().orc_local_score(q_len, q2.ctypes.data, t_len, tt.ctypes.data, mat.ctypes.data, opt.q, opt.e)
        if s >= opt.min_chain_score * opt.a and s >= opt.min_dp_max:
            return 2
    return 1 if max_zdrop > opt.zdrop else 0


def expected(oracle, opt, mat, kind, q, t, w, zdrop, flag):
    """What mm_align1 gets from its call(s) of ksw_extd2 for one Seg: dict of the result fields + "cigar" (words)."""
    sc = dict(q=opt.q, e=opt.e, q2=opt.q2, e2=opt.e2, mat=mat)
    if opt.max_sw_mat > 0 and len(t) * len(q) > opt.max_sw_mat:            # mm_align_pair: not run
        return dict(NOT_RUN, cigar=[])
    zdrop_code = 0
    if kind == 1:
        ez = oracle.ksw_extd2(q, t, w=w, zdrop=zdrop, end_bonus=-1, flag=flag, **sc)
        zdrop_code = zdrop_test(oracle, opt, mat, q, t, cigar_words(ez["cigar"]))
        if zdrop_code != 0:
            ez = oracle.ksw_extd2(q, t, w=w, zdrop=opt.zdrop_inv if zdrop_code == 2 else opt.zdrop, end_bonus=-1, flag=0, **sc)
    else:
        ez = oracle.ksw_extd2(q, t, w=w, zdrop=zdrop, end_bonus=opt.end_bonus, flag=flag, **sc)
    words = cigar_words(ez["cigar"])
    return dict(n_cigar=len(words), zdropped=ez["zdropped"], zdrop_code=zdrop_code, max=ez["max"], max_t=ez["max_t"], max_q=ez["max_q"],
                score=ez["score"], reach_end=ez["reach_end"], mqe_t=ez["mqe_t"], cigar=words)


def describe(seg):
    big = int(seg["big"])
    return (f"kernel class big={big} ({CLASS_NAMES.get(big, '?')}), kind={int(seg['kind'])} ({KIND_NAMES[int(seg['kind'])]}), read {int(seg['read'])}, "
            f"(tlen, qlen, w, zdrop, flag)=({int(seg['tlen'])}, {int(seg['qlen'])}, {int(seg['w'])}, {int(seg['zdrop'])}, {int(seg['flag']):#x}), "
            f"rid {int(seg['rid'])} rev {int(seg['rev'])} ts {int(seg['ts'])} qs {int(seg['qs'])}")


def outcome(kind, want):
    return ("gap" if kind == 1 else "ext", int(want["zdropped"]), int(want["reach_end"]))


def compare_call(seg, seg_words, want, not_run=False):
    """One dumped call (a row of SEG_DTYPE, or a dict with its fields) and its CIGAR words against `want` (`expected`'s
    dict).  Raises AssertionError naming the kernel class, the call and the field."""
    if not_run:
        fields = RESULT_FIELDS
    else:
        fields = COMPARED[outcome(int(seg["kind"]), want)]
    for f in fields:
        if f == "cigar":
            got, exp = [int(x) for x in seg_words], [int(x) for x in want["cigar"]]
            show = lambda ws: " ".join(f"{x >> 4}{'MID'[x & 0xf] if (x & 0xf) < 3 else '?'}" for x in ws)
            if got != exp:
                raise AssertionError(f"{describe(seg)}: field cigar: kernel [{show(got)}] != ksw_extd2 [{show(exp)}]")
        elif int(seg[f]) != int(want[f]):
            raise AssertionError(f"{describe(seg)}: field {f}: kernel {int(seg[f])} != ksw_extd2 {int(want[f])}")


def call_key(seg):
    """A call's inputs: what makes two dumps' rows the same call (their order in the pool is the order the waves came)."""
    return tuple(int(seg[k]) for k in ("read", "kind", "rid", "rev", "ts", "tlen", "qs", "qlen", "w", "zdrop")) + (int(seg["flag"]) & EZ_MASK,)


def results_table(segs, words):
    """The compared fields of every call of a dump, keyed and sorted by the call's inputs: equal between two runs of a batch
    whichever kernels ran the calls."""
    out = []
    for s in segs:
        not_run = bool(int(s["flag"]) & SEG_SKIPPED)
        fields = RESULT_FIELDS if not_run else COMPARED[("gap" if int(s["kind"]) == 1 else "ext", int(s["zdropped"]), int(s["reach_end"]) if int(s["kind"]) != 1 else 0)]
        vals = []
        for f in fields:
            if f == "cigar":
                vals.append(tuple(int(x) for x in words[int(s["cig_off"]):int(s["cig_off"]) + int(s["n_cigar"])]))
            else:
                vals.append(int(s[f]))
        out.append((call_key(s), tuple(vals)))
    out.sort()
    return out


def replay(capi, oracle, world, bases, offsets, cache=None, with_cigars=False):
    """After a `classify` of (bases, offsets) on world["eng"] under CONTRACT_DP: every kernel call of the batch against
    ksw_extd2 with the call's own inputs (scoring and end bonus from world["oidx"].opt).  Returns the segment table
    (SEG_DTYPE rows; with `with_cigars` also the per-call CIGAR pool).  `cache`: a dict that keeps the oracle's answers by
    call inputs between runs of the SAME batch on the SAME world (the six routes of one batch make the same calls)."""
    eng, opt, seqs = world["eng"], world["oidx"].opt, world["seqs"]
    segs = eng.dump(capi.DUMP_SEGS, capi.SEG_DTYPE)
    words = eng.dump(capi.DUMP_SEG_CIGARS, np.uint32)
    mat = oracle.simple_mat(opt.a, opt.b, opt.sc_ambi)
    tcodes, qcodes = {}, {}
    cache = {} if cache is None else cache
    for s in segs:
        kind, rid, rev, rd = int(s["kind"]), int(s["rid"]), int(s["rev"]), int(s["read"])
        ts, tlen, qs, qlen, flag = int(s["ts"]), int(s["tlen"]), int(s["qs"]), int(s["qlen"]), int(s["flag"])
        assert kind in (0, 1, 2) and 0 <= rid < len(seqs) and 0 <= rd < len(offsets) - 1, describe(s)
        assert int(s["n_cigar"]) >= 0 and int(s["cig_off"]) >= 0 and int(s["cig_off"]) + int(s["n_cigar"]) <= len(words), f"{describe(s)}: CIGAR outside the pool"
        got_words = words[int(s["cig_off"]):int(s["cig_off"]) + int(s["n_cigar"])]
        if (flag & SEG_SKIPPED) or tlen * qlen > opt.max_sw_mat:
            compare_call(s, got_words, dict(NOT_RUN, cigar=[]), not_run=True)
            continue
        key = call_key(s)
        want = cache.get(key)
        if want is None:
            if rid not in tcodes:
                tcodes[rid] = codes(seqs[rid])
            if (rd, rev) not in qcodes:
                fwd = codes(bases[offsets[rd]:offsets[rd + 1]])
                qcodes[(rd, rev)] = revcomp_codes(fwd) if rev else fwd
            assert 0 <= ts and ts + tlen <= len(tcodes[rid]) and 0 <= qs and qs + qlen <= len(qcodes[(rd, rev)]), f"{describe(s)}: interval outside its sequence"
            t, q = tcodes[rid][ts:ts + tlen], qcodes[(rd, rev)][qs:qs + qlen]
            if kind == 0:                                                  # mm_align1: seq_rev on both for the left extension
                t, q = t[::-1], q[::-1]
            want = expected(oracle, opt, mat, kind, np.ascontiguousarray(q), np.ascontiguousarray(t), int(s["w"]), int(s["zdrop"]), flag & EZ_MASK)
            cache[key] = want
        compare_call(s, got_words, want)
    return (segs, words) if with_cigars else segs
