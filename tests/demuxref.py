"""The demux contract (include/monica_amd.h, "demux") in plain Python and numpy: the textbook edit-distance table with a free
start and end in the text, the verdict per end, the rule per read -- no bit vectors.  `search` is the table cell by cell;
`search_all` the same recurrence for many texts and patterns at once (the column's insertion chain as a running minimum)."""
import numpy as np

CODE = np.full(256, 4, dtype=np.int16)
for _c, _letters in enumerate((b"Aa", b"Cc", b"Gg", b"TtUu")):
    CODE[list(_letters)] = _c
TAG_DTYPE = np.dtype([("barcode", "<i2"), ("d_front", "u1"), ("d_rear", "u1"), ("cut_front", "<u2"), ("cut_rear", "<u2")])
FRONT, BOTH, EITHER = 0, 1, 2


def codes(seq):
    return CODE[np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8)]


def texts(read, window):
    """(front, rear) codes of one read: its first and its last min(window, L) bases, the rear backwards and complemented."""
    c = codes(read)
    n = min(window, len(c))
    rear = c[len(c) - n:][::-1]
    return c[:n], np.where(rear < 4, 3 - rear, 4)


def search(p, t):
    """(d, e) of pattern codes p in text codes t: D[0][j] = 0, D[i][0] = i, unit costs; d = the smallest D[m][j], e = the
    first such j, minus one (-1: column 0, the empty substring)."""
    m, n = len(p), len(t)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        D[i][0] = i
        for j in range(1, n + 1):
            D[i][j] = min(D[i - 1][j - 1] + (p[i - 1] != t[j - 1] or t[j - 1] > 3), D[i - 1][j] + 1, D[i][j - 1] + 1)
    d = min(D[m])
    return d, D[m].index(d) - 1


def search_all(pats, txts):
    """d[T, B], e[T, B] of every pattern in every text, as `search` gives them."""
    B, T = len(pats), len(txts)
    plen = np.array([len(p) for p in pats])
    M, n = int(plen.max()), max([len(t) for t in txts] + [0])
    P = np.full((B, M), 5, dtype=np.int16)
    for b, p in enumerate(pats):
        P[b, :len(p)] = p
    X, tl = np.full((T, n), 4, dtype=np.int16), np.array([len(t) for t in txts])
    for k, t in enumerate(txts):
        X[k, :len(t)] = t
    ar = np.arange(M + 1, dtype=np.int16)
    col = np.broadcast_to(ar, (T, B, M + 1)).copy()
    last = lambda c: np.take_along_axis(c, np.broadcast_to(plen[None, :, None], (T, B, 1)), axis=2)[..., 0]
    d, e = last(col).copy(), np.full((T, B), -1)
    for j in range(n):
        sub = col[..., :-1] + (P[None] != X[:, j, None, None])
        new = np.concatenate([np.zeros((T, B, 1), dtype=np.int16), np.minimum(sub, col[..., 1:] + 1)], axis=2)
        new = ar + np.minimum.accumulate(new - ar, axis=2)
        live = j < tl
        col = np.where(live[:, None, None], new, col)
        better = live[:, None] & (last(new) < d)
        d, e = np.where(better, last(new), d), np.where(better, j, e)
    return d, e


def end(d, max_dist, min_margin):
    best = int(np.argmin(d))                                    # (hit, best barcode) of one end; the first of equals
    others = np.delete(d, best)
    return bool(d[best] <= max_dist and (len(others) == 0 or others.min() - d[best] >= min_margin)), best


def tags(barcodes, reads, window, max_dist, min_margin, ends):
    """The tags of `reads` (a list of bytes / uint8 arrays) for `barcodes` (a list of str / bytes)."""
    pats = [codes(b) for b in barcodes]
    tx = [texts(bytes(r), window) for r in reads]
    out = np.zeros(len(reads), dtype=TAG_DTYPE)
    if not len(reads):
        return out
    dF, eF = search_all(pats, [t[0] for t in tx])
    dR, eR = search_all(pats, [t[1] for t in tx]) if ends != FRONT else (None, None)
    for r in range(len(reads)):
        hf, bf = end(dF[r], max_dist, min_margin)
        hr, br = end(dR[r], max_dist, min_margin) if ends != FRONT else (False, -1)
        if ends == FRONT:
            bc = bf if hf else -1
        elif ends == BOTH:
            bc = bf if hf and hr and bf == br else -1
        else:
            bc = (bf if bf == br else -2) if hf and hr else bf if hf else br if hr else -1
        out[r] = (bc, dF[r, bf], dR[r, br] if ends != FRONT else 255,
                  eF[r, bf] + 1 if bc >= 0 and hf and bf == bc else 0, eR[r, br] + 1 if bc >= 0 and hr and br == bc else 0)
    return out


def read_counts(tag, n_barcodes):                               # reads[n + 2]: per barcode, then none, then conflict
    bc = tag["barcode"].astype(np.int64)
    return np.bincount(np.where(bc >= 0, bc, n_barcodes - 1 - bc), minlength=n_barcodes + 2)
