#!/usr/bin/env python3
"""What placing reads on a taxonomy costs (mnc_engine_add_lca / mnc_lca_fetch, csrc/k_lca.hip), warm, median of --reps, in one
run on one device, on bench.py's default shape -- 100 000 reads of 5 kb against 20 genomes, classified once (host buffers):

  add            HIP events around the call on the engine's stream (torch.cuda.Event on torch.cuda.ExternalStream(engine.stream)),
                 the accumulator reset before every call:
                   abundance   mnc_engine_add_abundance on the same batch, the yardstick (tools/abundance_bench.py's number)
                   lca, lds    mnc_engine_add_lca with monica's own two ranks over the 20 genomes (taxonomy_from_names): the
                               tree and a private direct[] in LDS
                   lca, global the same tree padded with unused inner nodes to MNC_LCA_LDS_NODES + 1: the tree through L2, one
                               global atomic per read -- the same answer for the shared nodes
  clade          the wall clock of Lca.counts() (scatter, scan, difference, two copies, one wait) for both trees

One JSON object on stdout; --out writes it to a file as well (profiles/lca_cost.json)."""
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
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
    parent, _ = _capi.taxonomy_from_names(index.genome_names)
    root = int(np.flatnonzero(parent == -1)[0])
    big = np.concatenate([parent, np.full(_capi.LCA_LDS_NODES + 1 - len(parent), root, dtype=np.int32)])

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

    res = {"shape": {"reads": args.reads, "read_len": args.read_len, "genomes": args.genomes, "reps": args.reps}, "add": {}, "clade": {}}
    ab = _capi.Abundance(index, 0, cap_cands=8 * args.reads)
    res["add"]["abundance"] = {**timed(ab, eng.add_abundance), **ab.info()}
    ab.close()
    direct = {}
    for label, tree in (("lca_lds", parent), ("lca_global", big)):
        lca = _capi.Lca(index, tree, cap_reads=args.reads)
        res["add"][label] = {**timed(lca, eng.add_lca), "n_nodes": len(tree), **lca.info(), "hbm_held_bytes": lca.device_bytes()}
        res["add"][label]["ratio_to_abundance"] = round(res["add"][label]["device_ms"] / res["add"]["abundance"]["device_ms"], 3)
        wall = []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            direct[label], clade = lca.counts()
            if k >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
        if int(clade[root]) != lca.info()["n_placed"]:
            raise RuntimeError(f"clade[root] {int(clade[root])} is not the {lca.info()['n_placed']} reads placed")
        res["clade"][label] = {"n_nodes": len(tree), "wall_ms": round(float(np.median(wall)), 4), "nodes_with_reads": int((direct[label] > 0).sum())}
        lca.close()
    if not np.array_equal(direct["lca_lds"], direct["lca_global"][:len(parent)]):
        raise RuntimeError("the two instantiations disagree on the shared nodes")
    eng.close()
    text = json.dumps(res)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
