#!/usr/bin/env python3
"""What the phased pileup costs (mnc_engine_add_pileup_phased; csrc/k_pile_phase.hip) on bench.py's default shape: 100 000
reads of 5 kb against 20 genomes, classified once (host buffers), then one add of the batch -- warm, median of --reps, the
variants ALTERNATING within every repetition of one run on one device, HIP events around the call on the engine's stream
(torch.cuda.Event on torch.cuda.ExternalStream(engine.stream)), as tools/haplotag_bench.py times its own:

  pileup            mnc_engine_add_pileup(GATED)            } the work the phased add fuses
  haplotag          mnc_engine_add_haplotag(GATED)          }
  phased            mnc_engine_add_pileup_phased(GATED) into hap0, hap1 and a rest
  phased, no rest   ... with rest = NULL

over the `called` site list of tools/haplotag_bench.py (what mnc_pileup_call_variants gives for the batch at (5, 3, 500), '+'
rows left out), block[] and phase[] from a window-1 linkage's phase(3, 500), min_votes 2, min_permille 600.  Also the sums of
the three accumulators' depth and the plain pileup's, which must agree.  One JSON object on stdout; --out writes it to a file
as well."""
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
    plain = _capi.Pileup(index, 0)
    eng.add_pileup(plain, what)
    sites = plain.variants(-1, 5, 3, 500)
    sites = sites[sites["alt"] != b"+"]
    lk = _capi.Linkage(index, sites, 1)
    eng.add_linkage(lk, what)
    block, phase = lk.phase(3, 500)
    lk.close()
    ht = _capi.Haplotag(index, sites, block, phase, args.reads, 2, 600)
    three, two = [_capi.Pileup(index, 0) for _ in range(3)], [_capi.Pileup(index, 0) for _ in range(2)]
    runs = {"pileup": ([plain], lambda: eng.add_pileup(plain, what)), "haplotag": ([ht], lambda: eng.add_haplotag(ht, what)),
            "phased": (three, lambda: eng.add_pileup_phased(ht, *three, what=what)), "phased, no rest": (two, lambda: eng.add_pileup_phased(ht, *two, what=what))}
    ms = {key: [] for key in runs}
    for rep in range(args.warmup + args.reps):
        for key, (accs, add) in runs.items():
            for acc in accs:
                acc.reset()
                acc.blocks(0, min(1, acc.n_blocks)) if acc is ht else acc.counts(0, 0, 1)   # a one-row read-out: the reset is over before the timed span
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            add()
            b.record(stream)
            b.synchronize()
            if rep >= args.warmup:
                ms[key].append(a.elapsed_time(b))
    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes, "reference_bases": int(sum(len(s) for s in seqs)),
                     "reps": args.reps, "warmup": args.warmup, "selector": "GATED", "phase": [3, 500], "min_votes": 2, "min_permille": 600},
           "sites": len(sites), "blocks": int(block[-1]) + 1 if len(block) else 0}
    res["add_ms"] = {key: {"device_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)} for key, v in ms.items()}
    fused = np.median(ms["pileup"]) + np.median(ms["haplotag"])
    for key in ("phased", "phased, no rest"):
        res["add_ms"][key]["over_pileup_plus_haplotag"] = round(float(np.median(ms[key]) / fused), 3)
    depth = {key: [int(sum(int(acc.counts(rid)[0].sum(dtype=np.int64)) for rid in range(len(seqs)))) for acc in accs] for key, (accs, _) in runs.items() if key != "haplotag"}
    res["depth_sums"] = depth                                    # as the last repetition's one add left them
    res["depth_agrees"] = sum(depth["phased"]) == depth["pileup"][0] and depth["phased"][:2] == depth["phased, no rest"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
