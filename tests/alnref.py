"""Plain-Python reference for the cs (short form) and MD strings of an alignment: a restatement of the contract in
include/monica_amd.h ("alignment records"), i.e. of minimap2 2.17's write_cs_core / write_MD_core, applied to a CIGAR and
the two sequences.  Test infrastructure: the GPU strings are compared with these, never the other way round.

Codes: nt4 0-3 = acgt (u as t), anything else = 4 = n.  Two bases match iff their codes are equal (n against n matches).
"""
import numpy as np

NT4 = np.full(256, 4, dtype=np.uint8)
for _c, _v in zip(b"ACGTUacgtu", (0, 1, 2, 3, 3, 0, 1, 2, 3, 3)):
    NT4[_c] = _v
LOWER, UPPER = "acgtn", "ACGTN"


def codes(seq):
    """bytes / str / uint8 array -> nt4 codes"""
    if isinstance(seq, str):
        seq = seq.encode()
    return NT4[np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)]


def query_codes(read, qs, qe, rev):
    """The query side of a hit: read[qs:qe] (forward-strand coordinates) on the hit's strand -- for rev its reverse
    complement, so that column 0 faces read base qe - 1."""
    q = codes(read)[qs:qe]
    if rev:
        q = q[::-1]
        q = np.where(q < 4, 3 - q, 4).astype(np.uint8)
    return q


def _ops(cigar):
    for l, op in cigar:
        yield int(l), ("MID".index(op) if isinstance(op, str) else int(op))


def cs_md(cigar, tseq, qseq):
    """cigar: [(len, op)] with op 'M' 'I' 'D' or 0 1 2; tseq / qseq: nt4 codes of the target interval [rs, re) and of the
    query on the hit's strand.  Returns (cs, MD)."""
    t_span = sum(l for l, op in _ops(cigar) if op != 1)
    q_span = sum(l for l, op in _ops(cigar) if op != 2)
    if t_span != len(tseq) or q_span != len(qseq):
        raise ValueError("the CIGAR spans %d target / %d query bases, the sequences have %d / %d" % (t_span, q_span, len(tseq), len(qseq)))
    cs, md = [], []
    t = q = 0
    l_md = 0
    for ln, op in _ops(cigar):
        if op == 0:
            run = 0
            for j in range(ln):
                tc, qc = int(tseq[t + j]), int(qseq[q + j])
                if tc != qc:
                    if run > 0:
                        cs.append(":%d" % run)
                        run = 0
                    cs.append("*" + LOWER[tc] + LOWER[qc])
                    md.append("%d%s" % (l_md, UPPER[tc]))
                    l_md = 0
                else:
                    run += 1
                    l_md += 1
            if run > 0:
                cs.append(":%d" % run)
            t += ln
            q += ln
        elif op == 1:
            cs.append("+" + "".join(LOWER[int(c)] for c in qseq[q:q + ln]))
            q += ln
        elif op == 2:
            cs.append("-" + "".join(LOWER[int(c)] for c in tseq[t:t + ln]))
            md.append("%d^%s" % (l_md, "".join(UPPER[int(c)] for c in tseq[t:t + ln])))
            l_md = 0
            t += ln
        else:
            raise ValueError("CIGAR operation %r" % (op,))
    if l_md > 0:
        md.append("%d" % l_md)
    return "".join(cs), "".join(md)


def cs_md_of_hit(reg, cigar, contig, read):
    """For one region (fields rs re qs qe rev) of `read` against `contig` (both uint8 / bytes)."""
    return cs_md(cigar, codes(contig)[int(reg["rs"]):int(reg["re"])], query_codes(read, int(reg["qs"]), int(reg["qe"]), int(reg["rev"])))
