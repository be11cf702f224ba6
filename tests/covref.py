"""The coverage contract of include/monica_amd.h ("coverage") restated in plain numpy -- the reference of
test_coverage_host.py and test_gpu_coverage.py.  Written from the contract, not from csrc/k_coverage.hip: depth is
counted base by base (no difference array, no scan), bins and summaries are sums over slices of it.

A record is (rid, rs, re, cigar, selected): cigar a list of (length, "M" | "I" | "D") running left to right on the contig
from rs, or None where there is none (the chain contract)."""
import numpy as np

GATED, PRIMARY, ALL, ASSIGNED, SPAN = 1, 2, 4, 8, 16
SUMMARY_DTYPE = np.dtype([("covered", "<i8"), ("depth_sum", "<i8"), ("max_depth", "<i4"), ("n_aln", "<i8")])


def m_columns(rs, cigar):
    """[start, end) on the contig of every M operation: what a record covers by default.  Bases under a D are not
    covered; an I consumes no reference."""
    out, at = [], int(rs)
    for length, op in cigar:
        if op == "M":
            out.append((at, at + length))
        if op != "I":
            at += length
    return out


def covered_runs(rs, cigar):
    """Maximal stretches of M columns not interrupted by a D: M operations that are neighbours or separated only by
    insertions merge."""
    runs = []
    for s, e in m_columns(rs, cigar):
        if e == s:
            continue
        if runs and runs[-1][1] == s:
            runs[-1] = (runs[-1][0], e)
        else:
            runs.append((s, e))
    return runs


def depth(records, contig_lens, span=False):
    """Per-base depth of every contig (a list of int64 arrays) after adding the selected records."""
    tracks = [np.zeros(int(n), dtype=np.int64) for n in contig_lens]
    for rid, rs, re, cigar, selected in records:
        if not selected:
            continue
        if span:
            tracks[rid][rs:re] += 1
        else:
            for s, e in m_columns(rs, cigar):
                tracks[rid][s:e] += 1
    return tracks


def bins(track, bin_bases):
    """(covered bases, depth sum) per bin of one contig; the last bin is short."""
    n = (len(track) + bin_bases - 1) // bin_bases
    cov = np.array([(track[b * bin_bases:(b + 1) * bin_bases] > 0).sum() for b in range(n)], dtype=np.int32)
    dsum = np.array([track[b * bin_bases:(b + 1) * bin_bases].sum() for b in range(n)], dtype=np.int64)
    return cov, dsum


def summary(records, tracks):
    out = np.zeros(len(tracks), dtype=SUMMARY_DTYPE)
    for c, t in enumerate(tracks):
        out[c]["covered"], out[c]["depth_sum"] = int((t > 0).sum()), int(t.sum())
        out[c]["max_depth"] = int(t.max()) if len(t) else 0
    for rid, _, _, _, selected in records:
        if selected:
            out[rid]["n_aln"] += 1
    return out


def best_hit(hits):
    """aligner.py:328-339 over (nm, mlen) pairs in exact integers: the index of the hit with the smallest nm / mlen, or
    None when the last update of the running minimum was a tie (ambiguous) or there is no hit."""
    if not hits:
        return None
    best, ties = 0, 1
    for i in range(1, len(hits)):
        left, right = hits[i][0] * hits[best][1], hits[best][0] * hits[i][1]
        if left < right:
            best, ties = i, 1
        elif left == right:
            best, ties = i, ties + 1
    return best if len(hits) == 1 or ties == 1 else None


def select(regs, what, min_mapq, skipped=False):
    """Which records of ONE read a call adds: `regs` holds id, parent, mapq, blen, mlen, n_ambi per record, in the order
    the read's hits are yielded."""
    primary = [int(r["id"]) == int(r["parent"]) for r in regs]
    gated = [p and int(r["mapq"]) >= min_mapq for p, r in zip(primary, regs)]
    what &= ~SPAN
    if what == ALL:
        return [True] * len(regs)
    if what == PRIMARY:
        return primary
    if what == GATED:
        return gated
    assert what == ASSIGNED
    out = [False] * len(regs)
    at = [i for i, g in enumerate(gated) if g]
    pick = None if skipped else best_hit([(int(regs[i]["blen"]) - int(regs[i]["mlen"]) + int(regs[i]["n_ambi"]), int(regs[i]["mlen"])) for i in at])
    if pick is not None:
        out[at[pick]] = True
    return out


def records_of(per_read, what, min_mapq):
    """The record list of a batch: `per_read` = [(regs, cigars | None), ...] as the oracle gives them."""
    out = []
    for regs, cigs in per_read:
        sel = select(regs, what, min_mapq)
        for i, r in enumerate(regs):
            out.append((int(r["rid"]), int(r["rs"]), int(r["re"]), cigs[i] if cigs is not None else None, sel[i]))
    return out
