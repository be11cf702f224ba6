#!/usr/bin/env python3
"""What assigning reads to barcodes costs (mnc_engine_add_demux, csrc/k_demux.hip), warm, median of --reps, in one run on one
device, on bench.py's default shape -- 100 000 reads of 5 kb against 20 genomes, classified once (host buffers):

  add            HIP events around the call on the engine's stream (torch.cuda.Event on torch.cuda.ExternalStream(engine.stream)),
                 the accumulator reset before every call:
                   abundance, lca   mnc_engine_add_abundance / mnc_engine_add_lca on the same batch, the yardsticks
                   demux            (barcodes, bases) = (24, 24), (96, 24), (96, 64) random patterns at window 150, for
                                    MNC_DEMUX_FRONT and MNC_DEMUX_BOTH: the search and the taxa kernel.  The search does the
                                    same work whatever the reads hold, so the batch carries no planted barcodes.
                   demux, wide      (96, 24) once more with the 64-bit kernel forced (mnc_demux_set_word_bits): what the
                                    32-bit instantiation gains on the same patterns
                   demux, search    ... and with an accumulator of no index: the search alone, no taxa kernel
  text steps     slots x window per read x reads over the add's time: the rate at which lanes advance one text base

One JSON object on stdout; --out writes it to a file as well (profiles/demux_cost.json)."""
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
    ap.add_argument("--window", type=int, default=150)
    ap.add_argument("--reps", type=int, default=9)
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

    def timed(acc, add):
        ms = []
        for k in range(args.warmup + args.reps):
            acc.reset()
            acc.info()                                              # the reset is over before the timed span
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            add(acc)
            b.record(stream)
            b.synchronize()
            if k >= args.warmup:
                ms.append(a.elapsed_time(b))
        return {"device_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4)}

    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes, "window": args.window, "reps": args.reps}, "add": {}}
    ab = _capi.Abundance(index, 0, cap_cands=8 * args.reads)
    res["add"]["abundance"] = timed(ab, eng.add_abundance)
    ab.close()
    lca = _capi.Lca(index, _capi.taxonomy_from_names(index.genome_names)[0], cap_reads=args.reads)
    res["add"]["lca"] = timed(lca, eng.add_lca)
    lca.close()
    rng = np.random.default_rng(24)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for n, m in ((24, 24), (96, 24), (96, 64)):
        bcs = [acgt[rng.integers(0, 4, m)] for _ in range(n)]
        for ends, label in ((_capi.DEMUX_FRONT, "front"), (_capi.DEMUX_BOTH, "both")):
            for kind in (("", "_wide", "_search") if (n, m, label) == (96, 24, "both") else ("",)):
                dm = _capi.Demux(None if kind == "_search" else index, bcs, window=args.window, ends=ends, cap_reads=args.reads)
                dm.set_word_bits(64 if kind == "_wide" else 0)
                row = {**timed(dm, eng.add_demux), "n_barcodes": n, "bases": m, "ends": label, **dm.info(), "hbm_held_bytes": dm.device_bytes()}
                if row["n_assigned"] + row["n_none"] + row["n_conflict"] != args.reads:
                    raise RuntimeError(f"reads[] sums to {row['n_assigned'] + row['n_none'] + row['n_conflict']}, the batch holds {args.reads}")
                steps = n * (1 if label == "front" else 2) * min(args.window, args.read_len) * args.reads
                row["text_steps_per_ns"] = round(steps / (row["device_ms"] * 1e6), 2)
                res["add"][f"demux_{n}x{m}_{label}" + kind] = row
                dm.close()
    head = res["add"]["demux_96x24_both"]["device_ms"]
    res["headline"] = {"demux_96x24_both_ms": head, "ratio_to_abundance": round(head / res["add"]["abundance"]["device_ms"], 3),
                       "ratio_to_lca": round(head / res["add"]["lca"]["device_ms"], 3),
                       "gain_of_32_bit": round(res["add"]["demux_96x24_both_wide"]["device_ms"] / head, 3)}
    eng.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
