"""mnc_linkage_phase_window (include/monica_amd.h, "linkage") restated as a plain sequential function over a fetched
pair[n][W][4] and the sites' rid -- the reference of test_gpu_linkwin.py.  Written from the definition: link, parent, interval
start, kept; no tiles, no pointer jumping."""
import numpy as np


def phase_window(pair, rid, reach, min_pairs, min_permille):
    """(keep bool[n], block int32[n], phase uint8[n])."""
    n = len(rid)
    parent, orient = np.arange(n), np.zeros(n, dtype=np.uint8)
    for i in range(n):
        best = 0
        for d in range(min(reach, i)):                          # ascending d: a tie stays with the nearest
            j = i - d - 1
            if rid[j] != rid[i]:
                break
            n00, n01, n10, n11 = (int(x) for x in pair[j, d])
            cis, trans = n00 + n11, n01 + n10
            diff = abs(cis - trans)
            if cis + trans >= min_pairs and cis != trans and diff * 1000 >= min_permille * (cis + trans) and diff > best:
                best, parent[i], orient[i] = diff, j, trans > cis
    start = np.array([all(parent[i] >= k for i in range(k, min(k + reach, n))) for k in range(n)], dtype=bool)
    root, par = np.arange(n), np.zeros(n, dtype=np.uint8)
    for i in range(n):                                          # a parent lies in front of its site
        if parent[i] != i:
            root[i], par[i] = root[parent[i]], par[parent[i]] ^ orient[i]
    keep = start[root] if n else start
    return keep, np.where(keep, np.cumsum(start) - 1, -1).astype(np.int32), np.where(keep, par, 0).astype(np.uint8)


def haplotag_accepts(rid, block, phase):
    """mnc_haplotag_create's rules for block[] / phase[] over a (compacted) list."""
    head = np.r_[True, block[1:] != block[:-1]]
    return bool((len(block) == 0 or block[0] == 0) and np.isin(np.diff(block), (0, 1)).all() and head[np.r_[True, rid[1:] != rid[:-1]]].all()
                and not phase[head].any() and (phase <= 1).all())
