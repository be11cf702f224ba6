"""The pileup contract of include/monica_amd.h ("pileup") restated in plain numpy -- the reference of test_pileup_host.py
and test_gpu_pileup.py.  Written from the contract, not from csrc/k_pileup.hip: every column is tallied into eight dense
arrays per contig (no difference track, no "only where it differs from the reference", no reconstruction), variants and
consensus are loops over those arrays.

A record is (rid, rs, cigar, rev, qs, qe, read, selected): cigar a list of (length, "M" | "I" | "D") running left to right
on the contig from rs, `read` the read's bytes as they were classified (forward strand), qs / qe forward-strand read
coordinates."""
import numpy as np

import covref

PLANES = ("depth", "A", "C", "G", "T", "N", "DEL", "INS")
DEPTH, A, C, G, T, N, DEL, INS = range(8)
VARIANT_DTYPE = np.dtype([("rid", "<i4"), ("pos", "<i4"), ("span", "<i4"), ("count", "<i4"), ("ref", "S1"), ("alt", "S1"), ("pad", "<u2")])
ALLELES = ((A, b"A"), (C, b"C"), (G, b"G"), (T, b"T"), (DEL, b"-"), (INS, b"+"))      # the order of a position's variants

CODE = np.full(256, 4, dtype=np.int64)                      # A C G T (U as T) in either case: 0 .. 3; anything else: 4 = N
for _i, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"TtUu")):
    for _b in _pair:
        CODE[_b] = _i


def query_columns(read, rev, qs, qe):
    """The query side of a record on the hit's strand, as codes: column p is read base qs + p for rev = 0 and the
    complement of read base qe - 1 - p for rev = 1."""
    codes = CODE[np.frombuffer(bytes(read), dtype=np.uint8)[qs:qe]]
    if rev:
        codes = codes[::-1]
        codes = np.where(codes < 4, 3 - codes, 4)
    return codes


def tally(records, seqs):
    """The eight planes of every contig (a list of int64 arrays [8, length]) after adding the selected records."""
    planes = [np.zeros((len(PLANES), len(s)), dtype=np.int64) for s in seqs]
    for rid, rs, cigar, rev, qs, qe, read, selected in records:
        if not selected:
            continue
        P = planes[rid]
        query = query_columns(read, rev, qs, qe)
        t, q, ref_seen = int(rs), 0, False
        for length, op in cigar:
            if op == "M":
                at = np.arange(t, t + length)               # every column of the operation: one more of depth and of its base
                P[DEPTH, at] += 1
                P[A + query[q:q + length], at] += 1         # (A C G T N follow one another; no place occurs twice)
                t, q, ref_seen = t + length, q + length, ref_seen or length > 0
            elif op == "D":
                for j in range(length):
                    P[DEL, t + j] += 1
                t, ref_seen = t + length, ref_seen or length > 0
            else:
                assert op == "I"
                if length > 0 and ref_seen:                 # once, at the last reference-consuming column before it
                    P[INS, t - 1] += 1
                q += length
        assert q == qe - qs, "the CIGAR's query length is not the record's"
    return planes


def ref_codes(seq):
    return CODE[np.asarray(seq, dtype=np.uint8)]


def variants(planes, seqs, rid, min_depth, min_count, min_permille):
    """The called variants of contig `rid` (-1: of every contig) in (rid, pos, allele) order."""
    out = []
    for c in (range(len(seqs)) if rid < 0 else [rid]):
        P, ref = planes[c], ref_codes(seqs[c])
        for p in range(P.shape[1]):
            span = int(P[DEPTH, p] + P[DEL, p])
            if ref[p] == 4 or span < min_depth:
                continue
            for plane, letter in ALLELES:
                count = int(P[plane, p])
                if plane == A + ref[p]:
                    continue
                if count >= min_count and count * 1000 >= min_permille * span:
                    out.append((c, p, span, count, b"ACGT"[ref[p]:ref[p] + 1], letter, 0))
    return np.array(out, dtype=VARIANT_DTYPE)


def consensus(planes, seqs, rid, start, end, min_depth):
    """One byte per base of [start, end) of contig `rid`."""
    P, ref = planes[rid], ref_codes(seqs[rid])
    out = bytearray()
    for p in range(start, end):
        if int(P[DEPTH, p] + P[DEL, p]) < min_depth:
            out += b"N"
            continue
        cand = [(int(P[A, p]), b"A"), (int(P[C, p]), b"C"), (int(P[G, p]), b"G"), (int(P[T, p]), b"T"), (int(P[DEL, p]), b"-")]
        top = max(n for n, _ in cand)
        tied = [letter for n, letter in cand if n == top]
        r = b"ACGTN"[ref[p]:ref[p] + 1]
        out += r if r in tied else tied[0]
    return bytes(out)


def records_of(per_read, reads, what, min_mapq):
    """The record list of a batch: `per_read` = [(regs, cigars), ...] as the oracle gives them, `reads` the reads."""
    out = []
    for (regs, cigs), read in zip(per_read, reads):
        sel = covref.select(regs, what, min_mapq)
        for i, r in enumerate(regs):
            out.append((int(r["rid"]), int(r["rs"]), cigs[i], int(r["rev"]), int(r["qs"]), int(r["qe"]), read, sel[i]))
    return out


def variants_tsv(variants, genome_of_contig, contig_names):
    """What aligner.write_variants_tsv leaves for a new file, restated."""
    lines = ["genome\tcontig\tpos\tref\talt\tcount\tspan\tpermille"]
    for v in variants:
        rid, count, span = int(v["rid"]), int(v["count"]), int(v["span"])
        lines.append("\t".join(str(x) for x in (genome_of_contig[rid], contig_names[rid], int(v["pos"]), v["ref"].decode(), v["alt"].decode(),
                                                 count, span, count * 1000 // span if span else 0)))
    return "\n".join(lines) + "\n"
