#!/usr/bin/env python3
"""What the candidate carry costs (mnc_engine_carry_candidates / mnc_abundance_add_carry, csrc/k_carry.hip, csrc/k_abundance.hip),
warm, median of --reps, in one run on one device:

  carry          mnc_engine_carry_candidates on bench.py's default shape -- 100 000 reads of 5 kb against 20 genomes, classified
                 once (host buffers) -- into a carry of --width pairs per read: HIP events around the call on the engine's
                 stream (torch.cuda.Event on torch.cuda.ExternalStream(engine.stream)).  Twice: into an empty carry (reset
                 before every call: what the first index part pays) and into the rows the call before left (every later part:
                 each pair meets its own genome).  Beside it mnc_engine_add_abundance on the same batch, measured the same way.
  add_carry      mnc_abundance_add_carry of --rows rows of three pairs (made with add_lists) into a global accumulator: the
                 wall clock of the call and of the wait for it (Abundance.info), the accumulator reset before.  The call
                 reads the carry's largest genome id back first (one pass over the carry, one wait), which is in the figure.

One JSON object on stdout; --out writes it to a file as well (profiles/carry_cost.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=5000)
    ap.add_argument("--genomes", type=int, default=20)
    ap.add_argument("--min-len", type=int, default=2_000_000)
    ap.add_argument("--max-len", type=int, default=7_000_000)
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-carry", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from monica_amd import _capi, synth

    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes, "width": args.width, "reps": args.reps}}
    if not args.skip_carry:
        names, seqs = synth.genome_set(args.genomes, min_len=args.min_len, max_len=args.max_len)
        index = _capi.Index.from_seqs(names, seqs)
        bases, offsets, _ = synth.reads(seqs, args.reads, args.read_len, seed=synth.SEED_READS + 2)
        eng = _capi.Engine(index, 0)
        eng.classify(bases, offsets, 60)
        carry = _capi.Carry(0, args.reads, width=args.width)
        ab = _capi.Abundance(index, 0, cap_cands=8 * args.reads)
        stream = torch.cuda.ExternalStream(eng.stream)

        def timed(call, before):
            ms = []
            for k in range(args.warmup + args.reps):
                before()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call()
                b.record(stream)
                b.synchronize()
                if k >= args.warmup:
                    ms.append(a.elapsed_time(b))
            return {"device_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4)}

        def emptied():
            carry.reset()
            carry.info()                                            # the reset is over before the timed span

        def cleared():
            ab.reset()
            ab.info()

        res["carry_into_empty_rows"] = timed(lambda: eng.carry_candidates(carry, 0, 0), emptied)
        res["carry_into_filled_rows"] = timed(lambda: eng.carry_candidates(carry, 0, 0), carry.info)
        res["carry_into_filled_rows"].update(carry.info(), hbm_held_bytes=carry.device_bytes())
        res["add_abundance_same_batch"] = timed(lambda: eng.add_abundance(ab), cleared)
        carry.close(), ab.close(), eng.close()
        del index
    # ---- add_carry: rows of three pairs, the middle one the best
    G, rows = 20, args.rows
    rng = np.random.default_rng(1)
    a = rng.integers(0, G - 6, rows)
    genome = np.stack([a, a + rng.integers(1, 4, rows), a + rng.integers(4, 7, rows)], axis=1).astype(np.int32).reshape(-1)
    score = np.stack([rng.integers(900, 1000, rows), np.full(rows, 1000), rng.integers(950, 1000, rows)], axis=1).astype(np.int32).reshape(-1)
    carry = _capi.Carry(0, rows, width=args.width, max_delta=100)
    carry.add_lists(0, np.arange(0, 3 * rows + 1, 3, dtype=np.int64), genome, score)
    ab = _capi.Abundance.global_(0, G, cap_cands=3 * rows, max_delta=100)
    wall = []
    for k in range(args.warmup + args.reps):
        ab.reset()
        ab.info()
        t0 = time.perf_counter()
        ab.add_carry(carry, 0, rows)
        info = ab.info()
        if k >= args.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    if info["n_stored_reads"] != rows or info["n_dropped"]:
        raise RuntimeError(f"{info}: {rows} rows of three candidates were expected")
    res["add_carry"] = {"rows": rows, "wall_ms": round(float(np.median(wall)), 4), "min_ms": round(float(np.min(wall)), 4), **info,
                        "carry_bytes_read": rows * (8 * args.width + 8),
                        "note": "wall clock of add_carry and the wait for it; includes the pass that reads the carry's largest genome id back"}
    carry.close(), ab.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
