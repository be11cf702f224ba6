"""The insertion alleles of include/monica_amd.h ("pileup": insertion alleles) restated in plain Python on pileref's
record tuples -- the reference of test_insertions_host.py and test_gpu_insertions.py.  Written from the header: a Counter
keyed by (rid, pos, bases on the hit's strand as codes), the call rule per allele, the consensus with insertions."""
from collections import Counter

import numpy as np

import pileref

LETTERS = b"ACGTN"
DTYPE = np.dtype([("rid", "<i4"), ("pos", "<i4"), ("span", "<i4"), ("count", "<i4"), ("len", "<i4"), ("pad", "<i4"), ("base_off", "<i8")])


def codes(text):
    return tuple(int(c) for c in pileref.CODE[np.frombuffer(bytes(text), dtype=np.uint8)])


def tally(records, seqs):
    """Counter {(rid, pos, codes): events} over the selected records: every I that the INS plane counts."""
    out = Counter()
    for rid, rs, cigar, rev, qs, qe, read, selected in records:
        if not selected:
            continue
        query = pileref.query_columns(read, rev, qs, qe)
        t, q, ref_seen = int(rs), 0, False
        for length, op in cigar:
            if op == "I":
                if length > 0 and ref_seen and 0 <= t - 1 < len(seqs[rid]):
                    out[(rid, t - 1, tuple(int(c) for c in query[q:q + length]))] += 1
                q += length
            else:
                t, ref_seen = t + length, ref_seen or length > 0
                q += length if op == "M" else 0
    return out


def span(planes, rid, pos):
    return int(planes[rid][pileref.DEPTH, pos] + planes[rid][pileref.DEL, pos])


def call(alleles, planes, seqs, rid, min_depth, min_count, min_permille):
    """(records, [bases]) in (rid, pos, len, codes) order, by the rule of the variants applied per allele."""
    rows, bases, off = [], [], 0
    for (c, pos, a), count in sorted(alleles.items(), key=lambda kv: (kv[0][0], kv[0][1], len(kv[0][2]), kv[0][2])):
        s = span(planes, c, pos)
        if (rid >= 0 and c != rid) or pileref.ref_codes(seqs[c][pos:pos + 1])[0] == 4 or s < min_depth:
            continue
        if count >= min_count and count * 1000 >= min_permille * s:
            rows.append((c, pos, s, count, len(a), 0, off))
            bases.append(bytes(LETTERS[x] for x in a))
            off += len(a)
    return np.array(rows, dtype=DTYPE), bases


def consensus(alleles, planes, seqs, rid, start, end, min_depth):
    plain = pileref.consensus(planes, seqs, rid, start, end, min_depth)
    at = {}
    for (c, pos, a), n in alleles.items():
        if c == rid:
            at.setdefault(pos, []).append((a, n))
    out = bytearray()
    for p in range(start, end):
        out += plain[p - start:p - start + 1]
        here = sorted(at.get(p, []), key=lambda an: (len(an[0]), an[0]))
        if here:
            a, n = max(here, key=lambda an: an[1])              # (max keeps the first of a tie)
            if span(planes, rid, p) >= min_depth and 2 * n > span(planes, rid, p):
                out += bytes(LETTERS[x] for x in a).lower()
    return bytes(out)


def variants_tsv(variants, called, genome_of_contig, contig_names):
    """pileref.variants_tsv with every '+' row replaced by the rows of that position's called alleles, alt = '+' + bases."""
    lines = pileref.variants_tsv(variants, genome_of_contig, contig_names).splitlines()
    out = lines[:1]
    for v, line in zip(variants, lines[1:]):
        if v["alt"] != b"+":
            out.append(line)
            continue
        f = line.split("\t")
        for r, b in zip(*called):
            if (r["rid"], r["pos"]) == (v["rid"], v["pos"]):
                out.append("\t".join(f[:4] + ["+" + b.decode(), str(r["count"]), str(r["span"]), str(int(r["count"]) * 1000 // int(r["span"]) if r["span"] else 0)]))
    return "\n".join(out) + "\n"
