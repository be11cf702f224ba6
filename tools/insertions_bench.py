#!/usr/bin/env python3
"""What storing the inserted bases costs (mnc_pileup_store_insertions; csrc/pile_ins.h, csrc/k_pile_ins.hip) on bench.py's
default shape: 100 000 reads of 5 kb against 20 genomes, classified once (host buffers), then -- warm, median of --reps,
in one run on one device --

  add_pileup          mnc_engine_add_pileup(GATED) into a pileup WITHOUT the store and into one WITH it, the two
                      alternating rep by rep: HIP events around the call on the engine's stream
                      (torch.cuda.Event on torch.cuda.ExternalStream(engine.stream)), each after a reset that is over
  occupancy           mnc_pileup_insertion_info after the first, second, ... --batches-th add of the same batch without a
                      reset in between (the same alleles again: the claims of the first add, the counts of the rest),
                      and of --batches batches of other reads
  call_insertions     mnc_pileup_call_insertions over the whole index, at (0, 1, 0) -- everything -- and at the variants'
  consensus_ins       (5, 3, 500); mnc_pileup_consensus_ins over the longest contig: wall clock around the call (they run
                      on the accumulator's own stream and wait for the host, so the wall clock IS what a caller sees)

One JSON object on stdout; --out writes it to a file as well (profiles/insertions_cost.json)."""
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
    ap.add_argument("--cap-alleles", type=int, default=1 << 26)
    ap.add_argument("--cap-pool-bases", type=int, default=1 << 24)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from monica_amd import _capi, synth

    names, seqs = synth.genome_set(args.genomes, min_len=args.min_len, max_len=args.max_len)
    index = _capi.Index.from_seqs(names, seqs)
    eng = _capi.Engine(index, 0)

    def classify(k):
        bases, offsets, _ = synth.reads(seqs, args.reads, args.read_len, seed=synth.SEED_READS + 2 + k)
        eng.classify(bases, offsets, 60)

    classify(0)
    plain = _capi.Pileup(index, 0)
    store = _capi.Pileup(index, 0, insertions=(args.cap_alleles, args.cap_pool_bases))
    stream = torch.cuda.ExternalStream(eng.stream)
    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes, "reference_bases": int(sum(len(s) for s in seqs)),
                     "cap_alleles": args.cap_alleles, "cap_pool_bases": args.cap_pool_bases, "reps": args.reps},
           "hbm_held_bytes": {"without_store": plain.device_bytes(), "with_store": store.device_bytes()}}
    # ---- the add, with and without the store, alternating
    ms = {"without_store": [], "with_store": []}
    for k in range(args.warmup + args.reps):
        for label, pu in (("without_store", plain), ("with_store", store)):
            pu.reset()
            pu.counts(0, 0, 1)                                  # the reset is over before the timed span
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            eng.add_pileup(pu, _capi.COV_GATED)
            b.record(stream)
            b.synchronize()
            if k >= args.warmup:
                ms[label].append(a.elapsed_time(b))
    res["add_pileup_gated"] = {k: {"device_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4)}
                               for k, v in ms.items()}
    # ---- occupancy: the same batch again (one add is in the table), then other reads
    occupancy = [dict(store.insertion_info(), after="add 1")]
    for k in range(1, args.batches):
        eng.add_pileup(store, _capi.COV_GATED)
        occupancy.append(dict(store.insertion_info(), after=f"add {k + 1} of the same batch"))
    for k in range(1, args.batches):
        classify(k)
        eng.add_pileup(store, _capi.COV_GATED)
        occupancy.append(dict(store.insertion_info(), after=f"batch {k + 1} of other reads"))
    slots = 64
    while slots < 2 * args.cap_alleles:
        slots *= 2
    for o in occupancy:
        o["load"] = round(o["n_alleles"] / slots, 4)
    res["occupancy"] = {"slots": slots, "per_add": occupancy}

    # ---- the read-outs
    def wall_ms(call):
        t, out = [], None
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            out = call()
            if k >= args.warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(t)), 4), out

    def fetch(thr):
        """mnc_pileup_call_insertions as a caller uses it: once for the sizes, once for the records and their bases."""
        import ctypes as C
        L, n, nb = _capi.lib(), C.c_int64(0), C.c_int64(0)
        rc = L.mnc_pileup_call_insertions(store._h, -1, *thr, None, 0, C.byref(n), None, 0, C.byref(nb))
        if n.value == 0:
            _capi.check(rc)
            return 0, 0
        rec, bases = np.empty(n.value, dtype=_capi.INSERTION_DTYPE), np.empty(max(nb.value, 1), dtype=np.uint8)
        _capi.check(L.mnc_pileup_call_insertions(store._h, -1, *thr, rec.ctypes.data, len(rec), C.byref(n), bases.ctypes.data, len(bases), C.byref(nb)))
        return int(n.value), int(nb.value)

    if occupancy[-1]["n_dropped"] or occupancy[-1]["n_pool_dropped"]:
        res["read_outs"] = "not measured: events were dropped (raise --cap-alleles / --cap-pool-bases)"
    else:
        longest = int(np.argmax(index.contig_lens))
        for label, thr in (("call_insertions_everything", (0, 1, 0)), ("call_insertions_5_3_500", (5, 3, 500))):
            t, (n_rec, n_bases) = wall_ms(lambda: fetch(thr))
            res[label] = {"wall_ms": t, "alleles": n_rec, "bases": n_bases, "note": "wall clock of the sizing call and the fetching call together (ctypes, into numpy arrays)"}
        t, cons = wall_ms(lambda: store.consensus(longest, 0, None, 5, insertions=True))
        res["consensus_ins_longest_contig"] = {"wall_ms": t, "bases": int(index.contig_lens[longest]), "characters": len(cons)}
        t, _ = wall_ms(lambda: store.consensus(longest, 0, None, 5))
        res["consensus_longest_contig"] = {"wall_ms": t}
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
