#!/usr/bin/env python3
"""What linkage costs (mnc_engine_add_linkage, mnc_linkage_phase; csrc/k_linkage.hip) on bench.py's default shape: 100 000
reads of 5 kb against 20 genomes, classified once (host buffers), then one add of the batch -- warm, median of --reps, the
variants ALTERNATING within every repetition of one run on one device, HIP events around the call on the engine's stream
(torch.cuda.Event on torch.cuda.ExternalStream(engine.stream)):

  pileup          mnc_engine_add_pileup(GATED): the yardstick
  called w<W>     mnc_engine_add_linkage(GATED) at each of --windows, the sites those mnc_pileup_call_variants gives for that
                  batch at tools/pileup_bench.py's thresholds (5, 3, 500), '+' rows left out: the two-pass recipe as it is run
  grid w<W>       the same over a site every --grid bases of every contig (an allele that is not the reference's): the load
                  of a sample with that many true variant positions, which the synthetic reads' chance calls do not give

and per site list the wall clock of one phase() over it and of one phase_window() at reach 1, 8 and 64 (where the window
holds it; with its allocation, its copies and its wait, alternating with phase()), the HBM held, and the atomics of one add counted from the words
as they stand (mnc_linkage_device) beside what one atomic per pair with both statements would have issued.  One JSON
object on stdout; --out writes it to a file as well."""
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
    ap.add_argument("--windows", type=int, nargs="+", default=(1, 16, 64))
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
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    grid = np.zeros(sum(len(range(0, len(s), args.grid)) for s in seqs), dtype=_capi.VARIANT_DTYPE)
    k = 0
    for rid, s in enumerate(seqs):
        at = np.arange(0, len(s), args.grid)
        grid["rid"][k:k + len(at)], grid["pos"][k:k + len(at)] = rid, at
        grid["alt"][k:k + len(at)] = acgt[(np.searchsorted(acgt, s[at]) + 1) % 4].view("S1")
        k += len(at)
    lists = {"called": called, "grid": grid}
    links = {f"{name} w{w}": _capi.Linkage(index, sites, w) for name, sites in lists.items() for w in args.windows}
    calls = {"pileup": lambda: eng.add_pileup(pu, what)}
    calls.update({key: (lambda lk=lk: eng.add_linkage(lk, what)) for key, lk in links.items()})
    ms = {key: [] for key in calls}
    for rep in range(args.warmup + args.reps):
        for key, call in calls.items():
            acc = links.get(key, pu)
            acc.reset()
            acc.site_counts(0, min(1, len(acc.sites))) if key in links else acc.counts(0, 0, 1)   # the reset is over before the timed span
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
           "hbm_held_bytes": {"pileup": pu.device_bytes(), **{key: lk.device_bytes() for key, lk in links.items()}}}
    base = float(np.median(ms["pileup"]))
    res["add_ms"] = {key: {"device_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4),
                           "over_pileup": round(float(np.median(v)) / base, 3)} for key, v in ms.items()}
    # ---- the atomics of one add, from the words as they stand after the last repetition's one add
    res["atomics_per_batch"], res["phase_wall_ms"], res["phase_window_wall_ms"] = {}, {}, {}
    for key, lk in links.items():
        n, w = len(lk.sites), lk.window
        if not n:
            continue
        site, pair = lk.site_counts(), lk.pairs()
        _, d_pair = lk.device()

        class Words:
            __cuda_array_interface__ = {"shape": (5 * n * w,), "typestr": "<i4", "data": (d_pair, False), "version": 2}

        words = torch.as_tensor(Words(), device="cuda:0")
        issued = int(words[:4 * n * w].sum(dtype=torch.int64)) + int(words[4 * n * w:].abs().sum(dtype=torch.int64))
        res["atomics_per_batch"][key] = {"site_statements": int(site.sum(dtype=np.int64)), "pair_words_issued_at_least": issued,
                                         "one_per_pair_with_both_statements": int(pair.sum(dtype=np.int64))}
        t = []
        for _ in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            lk.phase(3, 500)
            t.append((time.perf_counter() - t0) * 1e3)
        res["phase_wall_ms"][key] = round(float(np.median(t[args.warmup:])), 4)
        # ---- phase_window at every reach the window holds, alternating with phase() within every repetition
        reaches = [r for r in (1, 8, 64) if r <= w]
        tw = {r: [] for r in [0] + reaches}                       # 0: phase() itself
        for _ in range(args.warmup + args.reps):
            for r in tw:
                t0 = time.perf_counter()
                lk.phase_window(r, 3, 500) if r else lk.phase(3, 500)
                tw[r].append((time.perf_counter() - t0) * 1e3)
        res["phase_window_wall_ms"][key] = {("phase" if r == 0 else f"reach {r}"): {
            "wall_ms": round(float(np.median(v[args.warmup:])), 4), "min_ms": round(float(np.min(v[args.warmup:])), 4), "max_ms": round(float(np.max(v[args.warmup:])), 4),
            "cell_bytes_per_site": 16 * r, "kept": int(lk.phase_window(r, 3, 500)[0].sum()) if r else n} for r, v in tw.items()}
    res["note"] = ("pair_words_issued_at_least: the sum of the missing / n01 / n10 / n11 words plus the absolute sum of the difference track "
                   "(+1 and -1 at one word cancel there, so the true count is a little higher)")
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
