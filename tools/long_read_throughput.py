"""Throughput of a batch of very long reads: N reads of L genome bases at a given error rate from one synthetic contig,
classified through mnc_classify_batch (host arrays in, host arrays out).  Prints one JSON line with Gbases/s.

  python tools/long_read_throughput.py --reads 8 --length 900000                  # within the usual pass' limit
  python tools/long_read_throughput.py --reads 8 --length 1500000 --long-reads    # the wide pass (2^20 bases or more)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monica_amd import _capi, synth  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def noisy(rng, seg, rate):
    """`rate` errors per base: 40 % substitutions, 30 % deletions, 30 % one-base insertions."""
    r = rng.random(len(seg))
    seg = seg.copy()
    sub = r < rate * 0.4
    seg[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
    reps = np.ones(len(seg), dtype=np.int64)
    reps[(r >= rate * 0.4) & (r < rate * 0.7)] = 0
    ins = (r >= rate * 0.7) & (r < rate)
    reps[ins] = 2
    out = np.repeat(seg, reps)
    first = np.cumsum(reps)[ins] - 2                                # the first of the two copies becomes the inserted base
    out[first] = ACGT[rng.integers(0, 4, len(first))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8)
    ap.add_argument("--length", type=int, default=900_000)
    ap.add_argument("--error", type=float, default=0.08)
    ap.add_argument("--long-reads", action="store_true", help="Engine.set_long_reads(True): reads of 2^20 bases or more are classified")
    ap.add_argument("--genome", type=int, default=2_300_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    g = synth.genome(0x2C2C, a.genome)
    idx = _capi.Index.from_seqs([synth.contig_name(0), synth.contig_name(1)], [g, synth.genome(0x2C2D, 300_000)])
    eng = _capi.Engine(idx, 0)
    if a.long_reads:
        eng.set_long_reads(True)
    rng = np.random.default_rng(1)
    starts = rng.integers(0, a.genome - a.length + 1, a.reads)
    reads = [noisy(rng, g[s:s + a.length], a.error) for s in starts]
    offsets = np.zeros(a.reads + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(r) for r in reads])
    bases = _capi.pinned_array(np.concatenate(reads))
    times = []
    for step in range(a.warmup + a.steps):
        t = time.perf_counter()
        assign, best, nhits = eng.classify(bases, offsets, 60)
        times.append(time.perf_counter() - t)
    times = sorted(times[a.warmup:])
    med = times[len(times) // 2]
    print(json.dumps({"reads": a.reads, "genome_bases_per_read": a.length, "read_bases": int(offsets[-1]), "error": a.error,
                      "long_reads": bool(a.long_reads), "classified": int((assign >= 0).sum()), "skipped": int((assign == _capi.SKIPPED).sum()),
                      "mlen_over_len": round(float(best["mlen"].sum()) / float(offsets[-1]), 4),
                      "ms_per_batch_median": round(med * 1e3, 2), "ms_min": round(times[0] * 1e3, 2), "ms_max": round(times[-1] * 1e3, 2),
                      "gbases_per_s": round(float(offsets[-1]) / med / 1e9, 4), "steps": a.steps}))


if __name__ == "__main__":
    main()
