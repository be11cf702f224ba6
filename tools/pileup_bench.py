#!/usr/bin/env python3
"""What the per-base pileup costs (mnc_engine_add_pileup / mnc_pileup_call_variants, csrc/k_pileup.hip) on bench.py's
default shape: 100 000 reads of 5 kb against 20 genomes, classified once (host buffers), then -- warm, median of --reps,
in one run on one device --

  add_pileup     mnc_engine_add_pileup(GATED): HIP events around the call on the engine's stream
                 (torch.cuda.Event on torch.cuda.ExternalStream(engine.stream))
  add_coverage   mnc_engine_add_coverage(GATED), the same way: the depth track alone
  cs export      mnc_engine_export_alignments(cs): the same way -- the route a caller without the pileup has to take
                 before tallying on the host (the fetch of the strings comes on top: tools/export_bench.py)
  call_variants  mnc_pileup_call_variants over the whole index: wall clock around the call (it runs on the accumulator's
                 own stream and waits for the host, so the wall clock IS what a caller sees; labelled so)

and the atomics of one add, taken from the counts: the alt planes' atomics exactly -- the sum of the seven planes as they
stand in HBM after one add (mnc_pileup_device) -- beside the M columns, deleted bases and insertions, which is what one
atomic per column would have issued; the depth track adds two per run of M columns (the records are reported).  One JSON object on stdout; --out writes it to a file as well (profiles/pileup_cost.json)."""
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
    pu = _capi.Pileup(index, 0)
    cov = _capi.Coverage(index, 0, 1024)
    stream = torch.cuda.ExternalStream(eng.stream)

    def device_ms(before, call):
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

    def settle_pileup():
        pu.reset()
        pu.counts(0, 0, 1)                                      # the reset is over before the timed span

    def settle_coverage():
        cov.reset()
        cov.summary()

    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes, "reference_bases": int(sum(len(s) for s in seqs)),
                     "reps": args.reps}}
    res["hbm_held_bytes"] = pu.device_bytes()
    res["add_pileup_gated"] = device_ms(settle_pileup, lambda: eng.add_pileup(pu, _capi.COV_GATED))
    res["add_coverage_gated"] = device_ms(settle_coverage, lambda: eng.add_coverage(cov, _capi.COV_GATED))
    res["export_cs"] = device_ms(lambda: None, lambda: eng.export_alignments(cs=True))
    # ---- the atomics of one add, from the planes as they stand (one add since the last reset)
    summary = cov.summary()
    pu.counts(0, 0, 1)                                          # the add is over
    _, d_alt, words = pu.device()

    class AltPlanes:                                            # the seven planes in place, as a tensor
        __cuda_array_interface__ = {"shape": (7, words), "typestr": "<i4", "data": (d_alt, False), "version": 2}

    per_plane = torch.as_tensor(AltPlanes(), device="cuda:0").sum(dim=1, dtype=torch.int64).tolist()
    n_alt = int(sum(per_plane))
    m_columns = int(summary["depth_sum"].sum())
    records = int(summary["n_aln"].sum())
    res["atomics_per_batch"] = {"records": records, "m_columns": m_columns, "alt_plane_atomics": n_alt,
                                "alt_planes": dict(zip(_capi.PILE_PLANES[1:], per_plane)),
                                "one_per_column": m_columns + per_plane[5] + per_plane[6],
                                "note": "alt planes: exact (their sum after one add; DEL counts deleted bases, INS insertions); the depth track "
                                        "adds two per run of M columns, i.e. 2 * (1 + D operations) per record"}
    # ---- variants over the whole index
    t = []
    n_var = 0
    for k in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        n_var = len(pu.variants(-1, 5, 3, 500))
        if k >= args.warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    res["call_variants_whole_index"] = {"wall_ms": round(float(np.median(t)), 4), "variants": n_var, "thresholds": [5, 3, 500],
                                        "note": "wall clock: count pass, scan, write pass, two waits for the host"}
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
