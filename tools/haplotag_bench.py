#!/usr/bin/env python3
"""What haplotagging costs (mnc_engine_add_haplotag; csrc/k_haplotag.hip) on bench.py's default shape: 100 000 reads of 5 kb
against 20 genomes, classified once (host buffers), then one add of the batch -- warm, median of --reps, the variants
ALTERNATING within every repetition of one run on one device, HIP events around the call on the engine's stream
(torch.cuda.Event on torch.cuda.ExternalStream(engine.stream)), as tools/linkage_bench.py times its own:

  <list> linkage w1   mnc_engine_add_linkage(GATED) at window 1: the yardstick -- the same walk, more atomics
  <list> haplotag     mnc_engine_add_haplotag(GATED) over the same sites, block[] and phase[] from that linkage's
                      phase(3, 500), min_votes 2, min_permille 600

for tools/linkage_bench.py's two site lists: `called` (what mnc_pileup_call_variants gives for the batch at (5, 3, 500), '+'
rows left out) and `grid` (a site every --grid bases of every contig).  Per list also the blocks, the four block words'
sums and the tagged reads.  One JSON object on stdout; --out writes it to a file as well.  --yardstick FILE: the JSON that
tools/linkage_bench.py --windows 1 wrote with another build of the library on the same device; its "<list> w1" times are
copied in beside this run's."""
import argparse
import json
import os
import sys

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
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--yardstick", default=None)
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
    accs, blocks = {}, {}
    for name, sites in lists.items():
        lk = accs[f"{name} linkage w1"] = _capi.Linkage(index, sites, 1)
        eng.add_linkage(lk, what)
        block, phase = lk.phase(3, 500)
        accs[f"{name} haplotag"] = _capi.Haplotag(index, sites, block, phase, args.reads, 2, 600)
        blocks[name] = int(block[-1]) + 1 if len(block) else 0
    ms = {key: [] for key in accs}
    for rep in range(args.warmup + args.reps):
        for key, acc in accs.items():
            acc.reset()
            # a one-row read-out: the reset is over before the timed span
            acc.blocks(0, min(1, acc.n_blocks)) if key.endswith("haplotag") else acc.site_counts(0, min(1, len(acc.sites)))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            eng.add_haplotag(acc, what) if key.endswith("haplotag") else eng.add_linkage(acc, what)
            b.record(stream)
            b.synchronize()
            if rep >= args.warmup:
                ms[key].append(a.elapsed_time(b))
    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes, "reference_bases": int(sum(len(s) for s in seqs)),
                     "reps": args.reps, "warmup": args.warmup, "selector": "GATED", "grid": args.grid, "phase": [3, 500], "min_votes": 2, "min_permille": 600},
           "sites": {name: len(sites) for name, sites in lists.items()}, "blocks": blocks,
           "hbm_held_bytes": {key: acc.device_bytes() for key, acc in accs.items()}}
    res["add_ms"] = {key: {"device_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)} for key, v in ms.items()}
    for name in lists:
        res["add_ms"][f"{name} haplotag"]["over_linkage_w1"] = round(float(np.median(ms[f"{name} haplotag"]) / np.median(ms[f"{name} linkage w1"])), 3)
    res["tables"] = {}
    for name in lists:                                           # as the last repetition's one add left them
        ht = accs[f"{name} haplotag"]
        tag, _ = ht.tags()
        res["tables"][name] = {"block_word_sums": [int(x) for x in ht.blocks().sum(axis=0, dtype=np.int64)], "tagged_reads": int((tag >= 0).sum())}
    if args.yardstick:
        with open(args.yardstick) as f:
            other = json.load(f)["add_ms"]
        res["yardstick_other_build"] = {f"{name} linkage w1": other[f"{name} w1"] for name in lists if f"{name} w1" in other}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
