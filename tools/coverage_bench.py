#!/usr/bin/env python3
"""What coverage costs (mnc_engine_add_coverage / mnc_coverage_summary, csrc/k_coverage.hip) on bench.py's default shape:
100 000 reads of 5 kb against 20 genomes, classified once (host buffers), then -- warm, median of --reps --

  add            mnc_engine_add_coverage for COV_ASSIGNED and COV_ALL, each without and with COV_SPAN: HIP events around
                 the call on the engine's stream (torch.cuda.Event on torch.cuda.ExternalStream(engine.stream))
  summary        mnc_coverage_summary: wall clock around the call (it runs on the accumulator's own stream and waits
                 for the host, so the wall clock IS what a caller sees; labelled so)
  bins / depth   the profile and the per-base depth of the longest contig, wall clock likewise
  HBM held       mnc_coverage_device_bytes

beside the route available without it: export(0) + fetch of every record (tools/export_bench.py; walking the CIGARs on
the host comes on top).  One JSON object on stdout; --out writes it to a file as well (profiles/coverage_cost.json)."""
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
    ap.add_argument("--bin-bases", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from monica_amd import _capi, synth

    names, seqs = synth.genome_set(args.genomes, min_len=args.min_len, max_len=args.max_len)
    index = _capi.Index.from_seqs(names, seqs)
    bases, offsets, _ = synth.reads(seqs, args.reads, args.read_len, seed=synth.SEED_READS + 2)
    eng = _capi.Engine(index, 0)
    eng.classify(bases, offsets, 60)
    cov = _capi.Coverage(index, 0, args.bin_bases)
    stream = torch.cuda.ExternalStream(eng.stream)

    def median_wall(f):
        t = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            f()
            if k >= args.warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(t)), 4)

    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes, "reference_bases": int(sum(len(s) for s in seqs)),
                     "bin_bases": args.bin_bases, "reps": args.reps}}
    res["hbm_held_bytes"] = cov.device_bytes()
    res["add"] = {}
    for label, what in (("assigned", _capi.COV_ASSIGNED), ("assigned_span", _capi.COV_ASSIGNED | _capi.COV_SPAN),
                        ("all", _capi.COV_ALL), ("all_span", _capi.COV_ALL | _capi.COV_SPAN)):
        ms = []
        for k in range(args.warmup + args.reps):
            cov.reset()
            cov.summary()                                       # the reset is over before the timed span
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            eng.add_coverage(cov, what)
            b.record(stream)
            b.synchronize()
            if k >= args.warmup:
                ms.append(a.elapsed_time(b))
        s = cov.summary()
        res["add"][label] = {"device_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "records": int(s["n_aln"].sum()),
                             "depth_sum": int(s["depth_sum"].sum()), "covered": int(s["covered"].sum())}
    # the last state (ALL | SPAN) stays in the track for the read-outs
    res["summary"] = {"wall_ms": median_wall(cov.summary), "note": "wall clock: the call waits for its own stream"}
    rid = int(np.argmax(index.contig_lens))
    res["bins_longest_contig"] = {"wall_ms": median_wall(lambda: cov.bins(rid)), "contig_bases": int(index.contig_lens[rid])}
    res["depth_longest_contig"] = {"wall_ms": median_wall(lambda: cov.depth(rid)), "contig_bases": int(index.contig_lens[rid])}
    # the route available without the accumulator: every record to the host
    t_exp, t_fetch = [], []
    for k in range(args.warmup + 5):
        t0 = time.perf_counter()
        sizes = eng.export_alignments()
        eng.sync()
        t1 = time.perf_counter()
        eng.fetch_alignments(sizes)
        t2 = time.perf_counter()
        if k >= args.warmup:
            t_exp.append((t1 - t0) * 1e3), t_fetch.append((t2 - t1) * 1e3)
    res["export_route"] = {"export_0_wall_ms": round(float(np.median(t_exp)), 3), "fetch_wall_ms": round(float(np.median(t_fetch)), 3),
                           "note": "before any CIGAR is walked on the host, per batch"}
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
