"""The abundance contract (include/monica_amd.h, "abundance") in plain numpy: the reference of test_abundance_host.py and
test_gpu_abundance.py.  Written from the header, not from csrc/k_abundance.hip: candidates by a dict per read, the EM row
by row in float64 and uint64 scalars."""
import numpy as np

MAX_DELTA, SCALE_Q = 80, 3                       # the Python layer's defaults
MAX_PRODUCT = 4000
Q32 = 4294967296.0
# 2^(-f/4), f = 0 .. 3: the header's exact doubles
T = np.array([float.fromhex(h) for h in ("0x1.0000000000000p+0", "0x1.ae89f995ad3adp-1", "0x1.6a09e667f3bcdp-1", "0x1.306fe0a31b715p-1")],
             dtype=np.float64)


def candidates(records_of_read, contig_genome, max_delta=MAX_DELTA):
    """The (genome, delta) pairs of one read in ascending genome id: `records_of_read` is a structured array with "rid",
    "dp_max" and "n_cigar" (the oracle's regions); every record with a CIGAR counts.  [] for a read with no record."""
    best_of = {}
    for r in records_of_read:
        if int(r["n_cigar"]) <= 0:
            continue
        g, s = int(contig_genome[int(r["rid"])]), int(r["dp_max"])
        best_of[g] = max(best_of.get(g, s), s)
    if not best_of:
        return []
    best = max(best_of.values())
    return [(g, best - s) for g, s in sorted(best_of.items()) if best - s <= max_delta]


def collect(per_read, contig_genome, n_genomes, max_delta=MAX_DELTA):
    """What an accumulator holds after these reads: (unique int64[G], rows sorted as fetch_lists sorts them, n_reads)."""
    unique = np.zeros(n_genomes, dtype=np.int64)
    rows, n_reads = [], 0
    for recs in per_read:
        c = candidates(recs, contig_genome, max_delta)
        if not c:
            continue
        n_reads += 1
        if len(c) == 1:
            unique[c[0][0]] += 1
        else:
            rows.append(c)
    return unique, sort_rows(rows), n_reads


def sort_rows(rows):
    """Lexicographic by the row's sequence genome[0], delta[0], genome[1], ...; a prefix comes first (Python's tuple order)."""
    return sorted([[(int(g), int(d)) for g, d in row] for row in rows], key=lambda row: tuple(x for pair in row for x in pair))


def rows_to_csr(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    for i, row in enumerate(rows):
        off[i + 1] = off[i] + len(row)
    gen = np.array([g for row in rows for g, _ in row], dtype=np.int32)
    dlt = np.array([d for row in rows for _, d in row], dtype=np.int32)
    return off, gen, dlt


def csr_to_rows(off, gen, dlt):
    return [[(int(gen[j]), int(dlt[j])) for j in range(int(off[i]), int(off[i + 1]))] for i in range(len(off) - 1)]


def weights(delta, scale_q=SCALE_Q):
    """w = ldexp(T[x & 3], -(x >> 2)), x = delta * scale_q."""
    x = np.asarray(delta, dtype=np.int64) * int(scale_q)
    return np.ldexp(T[x & 3], -(x >> 2).astype(np.int32)).astype(np.float64)


def solve(unique, rows, G, scale_q=SCALE_Q, max_iter=200, tol_q32=1 << 22, n_reads=None, trace=None):
    """(theta float64[G], expected float64[G], iters).  `n_reads` = reads added (default: what unique and rows hold)."""
    unique = np.asarray(unique, dtype=np.int64)
    theta, expected = np.zeros(G, dtype=np.float64), np.zeros(G, dtype=np.float64)
    if n_reads is None:
        n_reads = int(unique.sum()) + len(rows)
    if n_reads == 0 or G == 0:
        return theta, expected, 0
    theta[:] = np.float64(1.0) / np.float64(G)
    prepared = [(np.array([g for g, _ in row], dtype=np.int64), weights([d for _, d in row], scale_q)) for row in rows]
    prev = [0] * G
    iters = 0
    for _ in range(int(max_iter)):
        acc = [int(u) << 32 for u in unique]                       # Python ints: checked to stay below 2^64 at the end
        for gs, ws in prepared:
            t = [np.float64(w) * theta[g] for g, w in zip(gs, ws)]
            z = np.float64(0.0)
            for x in t:
                z = z + x
            if z > 0:
                for g, x in zip(gs, t):
                    acc[int(g)] += int(np.floor((x / z) * np.float64(Q32)))
        total = sum(acc)
        assert total < 1 << 64
        for g in range(G):
            theta[g] = np.float64(np.uint64(acc[g])) / np.float64(np.uint64(total)) if total else 0.0
        iters += 1
        diff = max(abs(a - b) for a, b in zip(acc, prev))
        prev = acc
        if trace is not None:
            trace.append((theta.copy(), list(acc)))
        if diff <= int(tol_q32):
            break
    expected[:] = [np.float64(np.uint64(a)) / np.float64(Q32) for a in prev]
    return theta, expected, iters
