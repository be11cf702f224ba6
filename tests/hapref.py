"""The haplotag contract (include/monica_amd.h, "haplotag") restated in plain Python -- the reference of
test_gpu_haplotag.py.  Written from the contract, not from csrc/k_haplotag.hip: a serial loop over records, sites and blocks
with linkref's columns and statement; no masks, no segments, nothing carried from one 64 sites to the next."""
import numpy as np

import covref
import linkref
import pileref


def statements(per_read, reads, what, min_mapq, seqs, sites):
    """Per read, per selected record with a site under it: (index of its first site, [(site, REF or ALT), ...])."""
    refs = [pileref.ref_codes(s) for s in seqs]
    rid, pos, alt = sites["rid"].astype(int), sites["pos"].astype(int), [bytes(a) for a in sites["alt"]]
    out = []
    for (regs, cigs), read in zip(per_read, reads):
        out.append([])
        for r, cigar, selected in zip(regs, cigs, covref.select(regs, what, min_mapq)):
            under = np.flatnonzero((rid == int(r["rid"])) & (pos >= int(r["rs"])) & (pos < int(r["re"])))
            if not selected or not len(under):
                continue
            cols = linkref.columns(r, cigar, read)
            said = [(int(i), linkref.statement(cols.get(pos[i]), alt[i], int(refs[rid[i]][pos[i]]))) for i in under]
            out[-1].append((int(under[0]), [(i, a) for i, a in said if a is not None]))
    return out


def decide(n0, n1, min_votes, min_permille):
    """0 or 1: the haplotype a (record, block) pair is decided for; None: undecided."""
    tot = n0 + n1
    return int(n1 > n0) if tot >= min_votes and n0 != n1 and abs(n0 - n1) * 1000 >= min_permille * tot else None


def tally(stmts, block, phase, min_votes, min_permille):
    """(blk[n_blocks, 4], tag[n_reads], votes[n_reads, 2], pairs) of one add of the reads whose `statements` are `stmts`;
    pairs: (read, its record, the record's first site, block, n0, n1, the sites that voted) per (record, block) with a vote."""
    blk = np.zeros((int(block[-1]) + 1 if len(block) else 0, 4), dtype=np.int32)
    tag, votes, pairs = np.full(len(stmts), -1, dtype=np.int32), np.zeros((len(stmts), 2), dtype=np.int32), []
    for k, records in enumerate(stmts):
        best = 0
        for j, (first, said) in enumerate(records):
            for b in sorted({int(block[i]) for i, _ in said}):
                voted = [(i, a ^ int(phase[i])) for i, a in said if block[i] == b]
                n1 = sum(h for _, h in voted)
                n0 = len(voted) - n1
                hap = decide(n0, n1, min_votes, min_permille)
                blk[b, 2 if hap is None else hap] += 1
                blk[b, 3] += min(n0, n1)
                pairs.append((k, j, first, b, n0, n1, [i for i, _ in voted]))
                if hap is not None and abs(n0 - n1) > best:
                    best, tag[k], votes[k] = abs(n0 - n1), 2 * b + hap, (max(n0, n1), min(n0, n1))
    return blk, tag, votes, pairs
