#!/usr/bin/env python3
"""What the local haplotypes cost (mnc_engine_add_haplos, mnc_haplos_call; csrc/k_haplos.hip) on tools/linkage_bench.py's
batch and site lists: 100 000 reads of 5 kb against 20 genomes, classified once (host buffers), then one add of the batch --
warm, median of --reps, the variants ALTERNATING within every repetition of one run on one device, HIP events around the
call on the engine's stream (torch.cuda.Event on torch.cuda.ExternalStream(engine.stream)):

  linkage w<W>    mnc_engine_add_linkage(GATED) at --window (16): the yardstick
  haplos k<K>     mnc_engine_add_haplos(GATED) at each of --ks

per site list ("called": what mnc_pileup_call_variants gives for the batch at (5, 3, 500), '+' rows left out; "grid": a site
every --grid bases of every contig).  Per list as well the wall clock of one call() at (5, 3, 200) beside one phase(3, 500)
of the linkage accumulator (each with its copies and its wait, alternating), the HBM held, the histogram of the call summed
over the contigs, and the atomics of one add counted from the words as they stand (mnc_haplos_device).  One JSON object on
stdout; --out writes it to a file as well."""
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
    ap.add_argument("--ks", type=int, nargs="+", default=(2, 4, 6))
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--grid", type=int, default=200)
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
    stream = torch.cuda.ExternalStream(eng.stream)
    what = _capi.COV_GATED
    pu = _capi.Pileup(index, 0)
    eng.add_pileup(pu, what)
    called = pu.variants(-1, 5, 3, 500)
    called = called[called["alt"] != b"+"]
    pu.close()
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    grid = np.zeros(sum(len(range(0, len(s), args.grid)) for s in seqs), dtype=_capi.VARIANT_DTYPE)
    k = 0
    for rid, s in enumerate(seqs):
        at = np.arange(0, len(s), args.grid)
        grid["rid"][k:k + len(at)], grid["pos"][k:k + len(at)] = rid, at
        grid["alt"][k:k + len(at)] = acgt[(np.searchsorted(acgt, s[at]) + 1) % 4].view("S1")
        k += len(at)
    lists = {"called": called, "grid": grid}
    accs = {f"{name} linkage w{args.window}": _capi.Linkage(index, sites, args.window) for name, sites in lists.items()}
    accs.update({f"{name} haplos k{k}": _capi.Haplos(index, sites, k) for name, sites in lists.items() for k in args.ks})
    calls = {key: ((lambda a=a: eng.add_linkage(a, what)) if isinstance(a, _capi.Linkage) else (lambda a=a: eng.add_haplos(a, what))) for key, a in accs.items()}
    ms = {key: [] for key in calls}
    for rep in range(args.warmup + args.reps):
        for key, call in calls.items():
            acc = accs[key]
            acc.reset()
            n1 = min(1, len(acc.sites))
            acc.site_counts(0, n1) if isinstance(acc, _capi.Linkage) else acc.table(0, n1)   # the reset is over before the timed span
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            if rep >= args.warmup:
                ms[key].append(a.elapsed_time(b))
    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes, "reference_bases": int(sum(len(s) for s in seqs)),
                     "reps": args.reps, "selector": "GATED", "grid": args.grid},
           "sites": {name: len(sites) for name, sites in lists.items()},
           "hbm_held_bytes": {key: a.device_bytes() for key, a in accs.items()}}
    res["add_ms"] = {}
    for key, v in ms.items():
        base = float(np.median(ms[f"{key.split()[0]} linkage w{args.window}"]))
        res["add_ms"][key] = {"device_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4),
                              "over_linkage": round(float(np.median(v)) / base, 3)}
    # ---- the atomics of one add, from the words as they stand after the last repetition's one add; call() beside phase()
    res["atomics_per_batch"], res["readout_wall_ms"], res["hist"] = {}, {}, {}
    for key, hp in accs.items():
        n = len(hp.sites)
        if not n or isinstance(hp, _capi.Linkage):
            continue
        table = hp.table()
        cells = n << hp.k

        class Words:
            __cuda_array_interface__ = {"shape": (cells + n,), "typestr": "<i4", "data": (hp.device(), False), "version": 2}

        words = torch.as_tensor(Words(), device="cuda:0")
        res["atomics_per_batch"][key] = {"row_words_issued": int(words[:cells].sum(dtype=torch.int64)),
                                         "track_words_issued_at_least": int(words[cells:].abs().sum(dtype=torch.int64)),
                                         "one_per_spelled_window": int(table.sum(dtype=np.int64))}
        lk = accs[f"{key.split()[0]} linkage w{args.window}"]
        t = {"call": [], "phase": []}
        for _ in range(args.warmup + args.reps):
            for name, fn in (("call", lambda: hp.call(5, 3, 200)), ("phase", lambda: lk.phase(3, 500))):
                t0 = time.perf_counter()
                fn()
                t[name].append((time.perf_counter() - t0) * 1e3)
        res["readout_wall_ms"][key] = {name: {"wall_ms": round(float(np.median(v[args.warmup:])), 4), "min_ms": round(float(np.min(v[args.warmup:])), 4),
                                              "max_ms": round(float(np.max(v[args.warmup:])), 4)} for name, v in t.items()}
        n_haps, _, hist, rec = hp.call(5, 3, 200)
        res["hist"][key] = {"judged_windows_by_n_haps": hist.sum(axis=0).tolist(), "records": len(rec)}
    res["note"] = ("track_words_issued_at_least: the absolute sum of the difference track (+1 and -1 at one word cancel there, so the true count "
                   "is a little higher); call's wall clock is one mnc_haplos_call with room for the records the call before found: a scan of the track, the count pass, a scan of the tiles, "
                   "the place pass, four copies to the host and two waits")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
