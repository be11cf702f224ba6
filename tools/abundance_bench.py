#!/usr/bin/env python3
"""What the abundance EM costs (mnc_engine_add_abundance / mnc_abundance_solve, csrc/k_abundance.hip), warm, median of --reps,
in one run on one device:

  add            mnc_engine_add_abundance on bench.py's default shape -- 100 000 reads of 5 kb against 20 genomes, classified
                 once (host buffers): HIP events around the call on the engine's stream (torch.cuda.Event on
                 torch.cuda.ExternalStream(engine.stream)), the accumulator reset before every call
  iterate        ms per EM iteration over --rows stored rows of 3 candidates made with add_lists, for G = 20 and G = 500:
                 the wall clock of solve(max_iter = N, tol_q32 = 0) -- N iterations queued, one wait at the end -- for two
                 values of N; their difference over the difference in N is one iteration without the call's fixed costs.
                 The rows' three candidates tie (delta 0): the slowest EM to settle, so every iteration asked for runs.
                 Beside it the bytes a pass must read -- 8 per candidate and 8 per row offset; theta (8 G bytes) stays on
                 chip -- and that as a fraction of the HBM rate a float4 copy reaches on this chip (6.29 TB/s).

One JSON object on stdout; --out writes it to a file as well (profiles/abundance_cost.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12          # a float4 copy, measured on the MI355X (8 TB/s by the data sheet)


def triples(rng, G, n):
    """n rows of three ascending genome ids, spread over 0 .. G - 1, all three tied (delta 0): the slowest EM to settle, so
    that every iteration asked for is run."""
    step = max(G // 3, 1)
    a = rng.integers(0, G - 2 * step, n)
    b = a + rng.integers(1, step + 1, n)
    c = b + rng.integers(1, step + 1, n)
    genome = np.stack([a, b, c], axis=1).astype(np.int32).reshape(-1)
    delta = np.zeros(3 * n, dtype=np.int32)
    return np.arange(0, 3 * n + 1, 3, dtype=np.int64), genome, delta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=5000)
    ap.add_argument("--genomes", type=int, default=20)
    ap.add_argument("--min-len", type=int, default=2_000_000)
    ap.add_argument("--max-len", type=int, default=7_000_000)
    ap.add_argument("--rows", type=int, nargs="*", default=[1_000_000, 10_000_000])
    ap.add_argument("--G", type=int, nargs="*", default=[20, 500])
    ap.add_argument("--iters", type=int, nargs=2, default=[10, 50])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-add", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from monica_amd import _capi, synth

    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes, "reps": args.reps}}
    if not args.skip_add:
        names, seqs = synth.genome_set(args.genomes, min_len=args.min_len, max_len=args.max_len)
        index = _capi.Index.from_seqs(names, seqs)
        bases, offsets, _ = synth.reads(seqs, args.reads, args.read_len, seed=synth.SEED_READS + 2)
        eng = _capi.Engine(index, 0)
        eng.classify(bases, offsets, 60)
        ab = _capi.Abundance(index, 0, cap_cands=8 * args.reads)
        stream = torch.cuda.ExternalStream(eng.stream)
        ms = []
        for k in range(args.warmup + args.reps):
            ab.reset()
            ab.info()                                               # the reset is over before the timed span
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            eng.add_abundance(ab)
            b.record(stream)
            b.synchronize()
            if k >= args.warmup:
                ms.append(a.elapsed_time(b))
        res["add"] = {"device_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), **ab.info(),
                      "hbm_held_bytes": ab.device_bytes()}
        ab.close(), eng.close()
        del index
    res["iterate"] = []
    rng = np.random.default_rng(1)
    lo, hi = args.iters
    for G in args.G:
        index = _capi.Index.from_seqs([f"t{g}:acc{g}" for g in range(G)], [synth.genome(100 + g, 80) for g in range(G)])
        for rows in args.rows:
            ab = _capi.Abundance(index, 0, cap_cands=3 * rows)
            ab.add_lists(*triples(rng, G, rows))
            uniq = np.repeat(np.arange(G, dtype=np.int32), (np.arange(G) % 7 + 1) * max(rows // (10 * G), 1))        # unequal unique reads, a tenth of the rows
            ab.add_lists(np.arange(len(uniq) + 1, dtype=np.int64), uniq, np.zeros(len(uniq), dtype=np.int32))
            wall = {lo: [], hi: []}
            for k in range(args.warmup + args.reps):
                for n in (lo, hi):
                    t0 = time.perf_counter()
                    _, _, iters = ab.solve(max_iter=n, tol_q32=0)
                    if k >= args.warmup:
                        wall[n].append((time.perf_counter() - t0) * 1e3)
                    if iters != n:
                        raise RuntimeError(f"the EM settled after {iters} of {n} iterations: the timing would count launches that do nothing")
            per_iter = (float(np.median(wall[hi])) - float(np.median(wall[lo]))) / (hi - lo)
            must_read = rows * (3 * 8 + 8)
            res["iterate"].append({"G": G, "rows": rows, "candidates": 3 * rows, "ms_per_iteration": round(per_iter, 5),
                                   "solve_wall_ms": {str(n): round(float(np.median(wall[n])), 3) for n in (lo, hi)},
                                   "bytes_per_pass": must_read,
                                   "fraction_of_hbm_copy_rate": round(must_read / (per_iter * 1e-3) / HBM_COPY_BYTES_PER_S, 4) if per_iter > 0 else None,
                                   "note": "wall clock of solve at two iteration counts, differenced; both kernels of an iteration and their launch gap"})
            ab.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
