#!/usr/bin/env python3
"""What the strand store of the pileup costs (mnc_pileup_store_strands, mnc_engine_add_pileup_quals; csrc/k_pile_strand.hip)
on bench.py's default shape: 100 000 reads of 5 kb against 20 genomes, classified once (host buffers), then one add of the
batch -- warm, median of --reps, the variants ALTERNATING within every repetition of one run on one device, HIP events
around the call on the engine's stream (torch.cuda.Event on torch.cuda.ExternalStream(engine.stream)):

  plain            mnc_engine_add_pileup into a pileup without the store: the yardstick, the kernel of the parent commit
  strands          the same call into a pileup with the store, min_qual 0: the forward records' planes, no qualities read
  strands q<floor> mnc_engine_add_pileup_quals, the qualities already on the device, at each of --floors: the kernel alone
  ... host         the same with a page-locked host array: the copy of one byte per base comes on top

The qualities are seeded random Phred 0 .. 40 per base, so a floor q masks q / 41 of the M columns; the share that was
masked is read back from the planes (MNC_PILE_LOWQ over the M columns).  One JSON object on stdout; --out writes it to a
file as well."""
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
    ap.add_argument("--floors", type=int, nargs=2, default=(10, 20))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from monica_amd import _capi, synth

    names, seqs = synth.genome_set(args.genomes, min_len=args.min_len, max_len=args.max_len)
    index = _capi.Index.from_seqs(names, seqs)
    bases, offsets, _ = synth.reads(seqs, args.reads, args.read_len, seed=synth.SEED_READS + 2)
    quals = torch.from_numpy((33 + np.random.default_rng(0x9A15).integers(0, 41, len(bases))).astype(np.uint8)).pin_memory()
    d_quals = quals.to("cuda:0")
    eng = _capi.Engine(index, 0)
    eng.classify(bases, offsets, 60)
    stream = torch.cuda.ExternalStream(eng.stream)
    what = _capi.COV_GATED
    piles = {"plain": _capi.Pileup(index, 0), "strands": _capi.Pileup(index, 0, strands=0)}
    calls = {"plain": lambda: eng.add_pileup(piles["plain"], what), "strands": lambda: eng.add_pileup(piles["strands"], what)}
    for floor in args.floors:
        key = f"strands q{floor}"
        piles[key] = _capi.Pileup(index, 0, strands=floor)
        calls[key] = lambda p=piles[key]: eng.add_pileup(p, what, quals=d_quals.data_ptr(), quals_on_device=True)
    calls[f"strands q{args.floors[0]} host"] = lambda p=piles[f"strands q{args.floors[0]}"]: eng.add_pileup(p, what, quals=quals.data_ptr())
    ms = {k: [] for k in calls}
    for rep in range(args.warmup + args.reps):
        for key, call in calls.items():
            pu = piles[key.removesuffix(" host")]
            pu.reset()
            pu.counts(0, 0, 1)                                  # the reset is over before the timed span
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            if rep >= args.warmup:
                ms[key].append(a.elapsed_time(b))
    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes, "reference_bases": int(sum(len(s) for s in seqs)),
                     "reps": args.reps, "selector": "GATED"},
           "hbm_held_bytes": {k: p.device_bytes() for k, p in piles.items()}}
    base = float(np.median(ms["plain"]))
    res["add_ms"] = {k: {"device_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4),
                         "over_plain": round(float(np.median(v)) / base, 3)} for k, v in ms.items()}
    # ---- the masked share, from the planes as they stand after the last repetition's one add
    res["masked"] = {}
    for floor in args.floors:
        pu = piles[f"strands q{floor}"]
        pu.counts(0, 0, 1)
        _, _, d_lowq = pu.strands_device()
        words = pu.device()[2]

        class Planes:
            __cuda_array_interface__ = {"shape": (2, words), "typestr": "<i4", "data": (d_lowq, False), "version": 2}

        lowq, lowq_fwd = torch.as_tensor(Planes(), device="cuda:0").sum(dim=1, dtype=torch.int64).tolist()
        m_columns = lowq + sum(int(pu.counts(rid)[0].sum(dtype=np.int64)) for rid in range(len(seqs)))
        res["masked"][f"q{floor}"] = {"m_columns": m_columns, "masked": lowq, "masked_forward": lowq_fwd, "share": round(lowq / max(m_columns, 1), 4)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
