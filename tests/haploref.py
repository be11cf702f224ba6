"""The haplos contract (include/monica_amd.h, "haplos") in plain Python, written from the contract and not from the kernel: a
record's statement at every site comes from linkref, a window is a loop over its k sites; no masks, no track, no derived cell."""
import numpy as np

import covref
import linkref
import pileref

HAPLO_DTYPE = np.dtype([("window", "<i4"), ("pattern", "<i4"), ("count", "<i4"), ("total", "<i4")])


def said(r, cigar, read, sites, refs):
    """REF, ALT or None per site of `sites`: what record `r` says there; `refs`: the contigs as pileref.ref_codes gives them."""
    cols = linkref.columns(r, cigar, read)
    return [linkref.statement(cols.get(int(s["pos"])), bytes(s["alt"]), int(refs[int(s["rid"])][int(s["pos"])]))
            if int(s["rid"]) == int(r["rid"]) else None for s in sites]


def tally(per_read, reads, what, min_mapq, seqs, sites, k):
    """hap[n, 2^k] after adding the selected records; `per_read` = [(regs, cigars), ...] of the oracle."""
    hap = np.zeros((len(sites), 1 << k), dtype=np.int32)
    refs = [pileref.ref_codes(s) for s in seqs]
    for (regs, cigs), read in zip(per_read, reads):
        for r, cigar, selected in zip(regs, cigs, covref.select(regs, what, min_mapq)):
            if not selected:
                continue
            a = said(r, cigar, read, sites, refs)
            for i in range(len(sites) - k + 1):                 # (the list ascends: first and last on one contig, so all k)
                if sites[i]["rid"] == sites[i + k - 1]["rid"] and None not in a[i:i + k]:
                    hap[i, sum(x << (k - 1 - t) for t, x in enumerate(a[i:i + k]))] += 1
    return hap


def call(hap, sites, thresholds, n_contigs=None):
    """(n_haps, total, hist, records) of mnc_haplos_call; `n_contigs`: of the index (by default the last site's contig + 1)."""
    min_total, min_count, min_permille = thresholds
    n_haps, total = np.zeros(len(hap), dtype=np.uint8), hap.sum(axis=1).astype(np.int32)
    hist, records = np.zeros((int(sites["rid"].max()) + 1 if n_contigs is None else n_contigs, 8), dtype=np.int64), []
    for i, row in enumerate(hap):
        tot = int(total[i])
        if tot < min_total or tot <= 0:
            continue
        called = [p for p, c in enumerate(row) if int(c) >= min_count and int(c) * 1000 >= min_permille * tot]
        n_haps[i] = len(called)
        hist[int(sites[i]["rid"]), min(len(called), 7)] += 1
        records += [(i, p, int(row[p]), tot) for p in called]
    return n_haps, total, hist, np.array(records, dtype=HAPLO_DTYPE)
