"""The strand store's contract (include/monica_amd.h, "pileup": strands and base qualities) restated in plain numpy -- the
reference of test_gpu_strands.py.  Written from the contract, not from csrc/k_pile_strand.hip: every column is tallied into
18 dense arrays per contig, per strand and under a mask array; no difference track, no subtraction of masked columns."""
import numpy as np

import covref
import pileref

FWD, LOWQ, LOWQ_FWD, N_PLANES = 8, 16, 17, 18
VARIANT_STRAND_DTYPE = np.dtype(pileref.VARIANT_DTYPE.descr + [("count_fwd", "<i4"), ("span_fwd", "<i4")])
PLANE_OF = {b"A": pileref.A, b"C": pileref.C, b"G": pileref.G, b"T": pileref.T, b"-": pileref.DEL, b"+": pileref.INS}


def tally(per_read, reads, quals, what, min_mapq, seqs, min_qual):
    """The 18 planes of every contig: `per_read` = [(regs, cigars), ...] as the oracle gives them, `quals` per read."""
    planes = [np.zeros((N_PLANES, len(s)), dtype=np.int64) for s in seqs]
    for (regs, cigs), read, qual in zip(per_read, reads, quals):
        for r, cigar, selected in zip(regs, cigs, covref.select(regs, what, min_mapq)):
            if not selected:
                continue
            rev, qs, qe = int(r["rev"]), int(r["qs"]), int(r["qe"])
            P = planes[int(r["rid"])]
            query = pileref.query_columns(bytes(read), rev, qs, qe)
            phred = np.maximum(np.asarray(qual, dtype=np.int64)[qs:qe] - 33, 0)
            phred = phred[::-1] if rev else phred              # column p: the quality of the read base it is taken from
            rows = (0,) if rev else (0, FWD)                   # both strands; forward records once more
            t, q, ref_seen = int(r["rs"]), 0, False
            for length, op in cigar:
                if op == "M":
                    at, good = np.arange(t, t + length), phred[q:q + length] >= min_qual
                    for o in rows:
                        P[o + pileref.DEPTH, at[good]] += 1
                        P[o + pileref.A + query[q:q + length][good], at[good]] += 1
                        P[LOWQ + o // FWD, at[~good]] += 1
                    t, q, ref_seen = t + length, q + length, ref_seen or length > 0
                elif op == "D":
                    for o in rows:
                        P[o + pileref.DEL, t:t + length] += 1
                    t, ref_seen = t + length, ref_seen or length > 0
                else:
                    if length > 0 and ref_seen:
                        for o in rows:
                            P[o + pileref.INS, t - 1] += 1
                    q += length
    return planes


def variants(planes, seqs, rid, thr, strand_thr):
    """pileref.variants on the planes of both strands, then per strand s: count_s >= min_count, count_s * 1000 >= min_permille * span_s."""
    min_count, min_permille = strand_thr
    out = []
    for v in pileref.variants([p[:8] for p in planes], seqs, rid, *thr):
        P, p, k = planes[int(v["rid"])], int(v["pos"]), PLANE_OF[bytes(v["alt"])]
        cf, sf = int(P[FWD + k, p]), int(P[FWD + pileref.DEPTH, p] + P[FWD + pileref.DEL, p])
        cr, sr = int(v["count"]) - cf, int(v["span"]) - sf
        if all(c >= min_count and c * 1000 >= min_permille * s for c, s in ((cf, sf), (cr, sr))):
            out.append(tuple(v) + (cf, sf))
    return np.array(out, dtype=VARIANT_STRAND_DTYPE)
