#!/usr/bin/env python3
"""What the alignment-record export costs (mnc_engine_export_alignments, csrc/k_export.hip) on bench.py's default shape:
100 000 reads of 5 kb against 20 genomes, classified once (host buffers), then -- after warm-up --

  export(0)        records + CSR + CIGAR pool           HIP events around the export on the engine's stream
  export(CS|MD)    ... and both string pools            (they span the two small read-backs in the middle)
  fetch            the D2H copy of everything exported  (wall clock around mnc_engine_fetch_alignments)
  dump route       what the same information cost before: Engine.dump(DUMP_REGS) + Engine.cigars() (one hipMemcpy per
                   read and per region), on a slice of --slice reads, SCALED to the batch and labelled so

and the bytes each pass moves, from the exported records, against the achievable HBM rate (6.3 TB/s).  One JSON object
on stdout; --out writes it to a file as well (profiles/export_cost.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ROOF = 6.3e12       # bytes/s, float4 copy on an MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=5000)
    ap.add_argument("--genomes", type=int, default=20)
    ap.add_argument("--min-len", type=int, default=2_000_000)
    ap.add_argument("--max-len", type=int, default=7_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slice", type=int, default=2000, help="reads of the dump-route leg (0: skip it)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from monica_amd import _capi, synth

    names, seqs = synth.genome_set(args.genomes, min_len=args.min_len, max_len=args.max_len)
    index = _capi.Index.from_seqs(names, seqs)
    bases, offsets, _ = synth.reads(seqs, args.reads, args.read_len, seed=synth.SEED_READS + 2)
    eng = _capi.Engine(index, 0)
    eng.set_profiling(True)
    eng.classify(bases, offsets, 60)

    def timed_export(cs, md):
        dev, wall, sizes = [], [], None
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            sizes = eng.export_alignments(cs=cs, MD=md)
            ms = eng.export_ms()                                # waits for the write pass
            t1 = time.perf_counter()
            if k >= args.warmup:
                dev.append(ms), wall.append((t1 - t0) * 1e3)
        return sizes, float(np.median(dev)), float(np.median(wall))

    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes}}
    sizes0, dev0, wall0 = timed_export(False, False)
    sizes, dev, wall = timed_export(True, True)
    fetch = []
    for k in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        out = eng.fetch_alignments(sizes)
        if k >= args.warmup:
            fetch.append((time.perf_counter() - t0) * 1e3)
    off, recs, cig, cs, md = out
    n = len(recs)
    q_span = int((recs["qe"] - recs["qs"]).sum())
    t_span = int((recs["re"] - recs["rs"]).sum())
    slots = n * 104
    # bytes per pass (compulsory traffic; the look-ahead base of a match column and re-reads within a line hit the caches)
    rec_pass = {"read": int(args.reads * 4 + n * (104 + 48)), "write": slots}                 # n_reg, a region and its RegDP per record
    count_pass = {"read": slots + 4 * len(cig) + q_span + t_span // 2, "write": 8 * n}
    write_pass = {"read": slots + 4 * len(cig) + q_span + t_span // 2 + 24 * n, "write": 4 * len(cig) + len(cs) + len(md) + 24 * n}
    write_pass0 = {"read": slots + 4 * len(cig) + 8 * n, "write": 4 * len(cig) + 24 * n}
    tot0 = sum(rec_pass.values()) + sum(write_pass0.values())
    tot = sum(rec_pass.values()) + sum(count_pass.values()) + sum(write_pass.values())
    res["records"] = {"n": n, "cigar_words": int(len(cig)), "cs_bytes": int(len(cs)), "md_bytes": int(len(md)), "query_bases": q_span, "target_bases": t_span}
    res["export_0"] = {"device_span_ms": round(dev0, 3), "wall_ms": round(wall0, 3), "bytes": tot0, "passes": {"records": rec_pass, "write": write_pass0},
                       "hbm_roof_frac": round(tot0 / (dev0 * 1e-3) / HBM_ROOF, 4) if dev0 > 0 else None}
    res["export_cs_md"] = {"device_span_ms": round(dev, 3), "wall_ms": round(wall, 3), "bytes": tot,
                           "passes": {"records": rec_pass, "count": count_pass, "write": write_pass},
                           "hbm_roof_frac": round(tot / (dev * 1e-3) / HBM_ROOF, 4) if dev > 0 else None,
                           "columns_per_s": round((q_span + t_span) / 2 / (dev * 1e-3), 1) if dev > 0 else None}
    d2h = off.nbytes + recs.nbytes + cig.nbytes + cs.nbytes + md.nbytes
    res["fetch"] = {"wall_ms": round(float(np.median(fetch)), 3), "bytes": int(d2h), "GB_per_s": round(d2h / (np.median(fetch) * 1e-3) / 1e9, 2)}
    if args.slice:
        m = min(args.slice, args.reads)
        eng.classify(bases[:offsets[m]], offsets[:m + 1], 60)
        t0 = time.perf_counter()
        regs = eng.dump(_capi.DUMP_REGS, _capi.REG_DTYPE)
        eng.cigars()
        t = (time.perf_counter() - t0) * 1e3
        res["dump_route"] = {"slice_reads": m, "slice_regions": int(len(regs)), "slice_wall_ms": round(t, 3),
                             "scaled_to_batch_ms": round(t * args.reads / m, 1), "note": "SCALED from the slice by read count, not measured at full size"}
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
