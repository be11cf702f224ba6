"""The phased-pileup contract (include/monica_amd.h, "phased pileup") restated in plain Python -- the reference of
test_phased_host.py and test_gpu_phased.py.  Written from the contract, not from csrc/k_pile_phase.hip: hapref's statements
and decision per (record, block), then a serial loop over each selected record's CIGAR that tallies every column into one of
three dense [8, length] arrays per contig; no windows, no masks, no runs."""
import numpy as np

import covref
import hapref
import pileref

HAP0, HAP1, REST = range(3)


def block_of(sites, block, rid, p):
    """The block of position p of contig rid, or None."""
    lo, hi = np.searchsorted(sites["rid"], (rid, rid + 1))     # the contig's sites (the list ascends)
    i = int(lo + np.searchsorted(sites["pos"][lo:hi], p))       # the first of them at or behind p
    if i < hi and (sites["pos"][i] == p or (i - 1 >= lo and block[i - 1] == block[i])):
        return int(block[i])
    return None


def tally(per_read, reads, what, min_mapq, seqs, sites, block, phase, min_votes, min_permille):
    """(planes[3][contig] = int64 [8, length], notes): the planes of hap0, hap1 and the rest after adding the selected records;
    notes: per selected record with a site under it (the block of its first site, {block: haplotype} of its decided blocks)
    under "decided", and how often an M run changed between the haplotypes, a D run crossed an extent's border and an I was anchored on an extent's last base."""
    planes = [[np.zeros((len(pileref.PLANES), len(s)), dtype=np.int64) for s in seqs] for _ in range(3)]
    notes = {"decided": [], "M changes haplotype": 0, "D over a border": 0, "I on a last base": 0}
    stmts = hapref.statements(per_read, reads, what, min_mapq, seqs, sites)
    for (regs, cigs), read, said_of in zip(per_read, reads, stmts):
        said_of = iter(said_of)
        for r, cigar, selected in zip(regs, cigs, covref.select(regs, what, min_mapq)):
            if not selected:
                continue
            rid, decided = int(r["rid"]), {}
            if ((sites["rid"] == rid) & (sites["pos"] >= r["rs"]) & (sites["pos"] < r["re"])).any():
                first, said = next(said_of)
                for b in {int(block[i]) for i, _ in said}:
                    n1 = sum(a ^ int(phase[i]) for i, a in said if block[i] == b)
                    hap = hapref.decide(sum(block[i] == b for i, _ in said) - n1, n1, min_votes, min_permille)
                    if hap is not None:
                        decided[b] = hap
                notes["decided"].append((int(block[first]), decided))
            where = {}                                          # position -> (its block, its destination)

            def at(p):
                b = where[p] = where[p] if p in where else block_of(sites, block, rid, p)
                return b, decided.get(b, REST)
            query = pileref.query_columns(read, int(r["rev"]), int(r["qs"]), int(r["qe"]))
            t, q, ref_seen = int(r["rs"]), 0, False
            for length, op in cigar:
                for j in range(length if op != "I" else 0):
                    P = planes[at(t + j)[1]][rid]
                    P[pileref.DEPTH if op == "M" else pileref.DEL, t + j] += 1
                    if op == "M":
                        P[pileref.A + query[q + j], t + j] += 1
                    if j:
                        notes["M changes haplotype"] += op == "M" and at(t + j)[1] + at(t + j - 1)[1] == HAP0 + HAP1
                        notes["D over a border"] += op == "D" and at(t + j)[0] != at(t + j - 1)[0]
                if op == "I" and length > 0 and ref_seen:
                    planes[at(t - 1)[1]][rid][pileref.INS, t - 1] += 1
                    notes["I on a last base"] += at(t - 1)[0] is not None and at(t - 1)[0] != block_of(sites, block, rid, t)
                t, q, ref_seen = t + (length if op != "I" else 0), q + (length if op != "D" else 0), ref_seen or (op != "I" and length > 0)
    return planes, notes
