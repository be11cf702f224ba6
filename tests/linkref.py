"""The linkage contract (include/monica_amd.h, "linkage") restated in plain Python -- the reference of test_gpu_linkage.py.
Written from the contract, not from csrc/k_linkage.hip: a record is expanded to {reference position: its column}, every
site gets its statement from that, the pair cells are a loop over pairs of sites; no masks, no difference track, no
derived cell.  The phase rule is a serial loop."""
import numpy as np

import covref
import pileref

REF, ALT = 0, 1


def columns(r, cigar, read):
    """{position: query code 0 .. 4 of an M column, or "D"} of one record."""
    query = pileref.query_columns(bytes(read), int(r["rev"]), int(r["qs"]), int(r["qe"]))
    cols, t, q = {}, int(r["rs"]), 0
    for length, op in cigar:
        if op != "I":
            cols.update((t + k, int(query[q + k]) if op == "M" else "D") for k in range(length))
        t, q = t + (length if op != "I" else 0), q + (length if op != "D" else 0)
    return cols


def statement(col, alt, ref_code):
    """REF, ALT or None: what a record whose column over a site is `col` (None: not covered) says there."""
    if col == ("D" if alt == b"-" else b"ACGT".index(alt)):
        return ALT
    return REF if col not in (None, "D") and ref_code < 4 and col == ref_code else None


def tally(per_read, reads, what, min_mapq, seqs, sites, window):
    """(site[n, 2], pair[n, window, 4]) after adding the selected records; `per_read` = [(regs, cigars), ...] of the oracle."""
    site, pair = np.zeros((len(sites), 2), dtype=np.int32), np.zeros((len(sites), window, 4), dtype=np.int32)
    refs = [pileref.ref_codes(s) for s in seqs]
    for (regs, cigs), read in zip(per_read, reads):
        for r, cigar, selected in zip(regs, cigs, covref.select(regs, what, min_mapq)):
            if not selected:
                continue
            cols = columns(r, cigar, read)
            said = []                                           # (site, statement) of this record, in list order
            for i, s in enumerate(sites):
                if int(s["rid"]) == int(r["rid"]) and int(r["rs"]) <= int(s["pos"]) < int(r["re"]):
                    a = statement(cols.get(int(s["pos"])), bytes(s["alt"]), int(refs[int(s["rid"])][int(s["pos"])]))
                    if a is not None:
                        site[i, a] += 1
                        said.append((i, a))
            for x, (i, a_i) in enumerate(said):
                for j, a_j in said[x + 1:]:
                    if j - i - 1 < window:                      # (one record: one contig)
                        pair[i, j - i - 1, 2 * a_i + a_j] += 1
    return site, pair


def phase(pair, sites, min_pairs, min_permille):
    """(block, phase) per site from the adjacent pairs."""
    block, ph = np.zeros(len(sites), dtype=np.int32), np.zeros(len(sites), dtype=np.uint8)
    for i in range(1, len(sites)):
        n00, n01, n10, n11 = (int(x) for x in pair[i - 1, 0])
        cis, trans = n00 + n11, n01 + n10
        linked = (sites[i]["rid"] == sites[i - 1]["rid"] and cis + trans >= min_pairs and cis != trans
                  and abs(cis - trans) * 1000 >= min_permille * (cis + trans))
        block[i], ph[i] = block[i - 1] + (not linked), ph[i - 1] ^ (trans > cis) if linked else 0
    return block, ph
