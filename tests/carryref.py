"""The candidate carry's merge rule (include/monica_amd.h, "candidate carry") in plain Python dicts: the reference of
test_carry_host.py and test_gpu_carry.py.  Written from the header, not from csrc/k_carry.hip.  A part's pairs are offered
WITHOUT the per-part pre-filter the header allows an implementation, so the tests check that claim too.

A row is a dict {"best": int or None, "pairs": {genome: score}, "truncated": bool}; an empty row has best None."""


def empty():
    return {"best": None, "pairs": {}, "truncated": False}


def offered(records_of_read, contig_genome, genome_offset=0):
    """What one part gives a read (rule 1): [(global genome id, s_g)] in ascending id; `records_of_read` as abundref takes
    them (the oracle's regions: "rid", "dp_max", "n_cigar")."""
    best_of = {}
    for r in records_of_read:
        if int(r["n_cigar"]) <= 0:
            continue
        g, s = int(contig_genome[int(r["rid"])]) + genome_offset, int(r["dp_max"])
        best_of[g] = max(best_of.get(g, s), s)
    return sorted(best_of.items())


def rank(pair):
    """Sort key: score descending, ties to the smaller genome id."""
    g, s = pair
    return (-s, g)


def merge(row, pairs, width, max_delta):
    """Rules 2 and 3: `pairs` [(genome, score)] of one delivery merged into `row`, in place; returns the row."""
    if not pairs:
        return row
    incoming = max(s for _, s in pairs)
    row["best"] = incoming if row["best"] is None else max(row["best"], incoming)
    for g, s in pairs:
        row["pairs"][g] = max(row["pairs"].get(g, s), s)
    kept = [(g, s) for g, s in row["pairs"].items() if row["best"] - s <= max_delta]
    if len(kept) > width:
        kept = sorted(kept, key=rank)[:width]
        row["truncated"] = True
    row["pairs"] = dict(kept)
    return row


def merge_rows(dst, src, width, max_delta):
    """mnc_carry_merge for one row: src's pairs by the same rule, and its truncated bit handed on."""
    merge(dst, sorted(src["pairs"].items()), width, max_delta)
    dst["truncated"] = dst["truncated"] or src["truncated"]
    return dst


def closed_form(all_pairs, width, max_delta):
    """Rule 4: the top `width` pairs by rank among all pairs ever offered (per genome its largest score), cut at
    best - max_delta.  {genome: score}."""
    best_of = {}
    for g, s in all_pairs:
        best_of[g] = max(best_of.get(g, s), s)
    if not best_of:
        return {}
    best = max(best_of.values())
    return dict(sorted(((g, s) for g, s in best_of.items() if best - s <= max_delta), key=rank)[:width])


def fetched(row, width):
    """The row as mnc_carry_fetch returns it: (count, best, genome[width], score[width]); ascending genome id, unused -1 / 0."""
    pairs = sorted(row["pairs"].items())
    pad = width - len(pairs)
    return (len(pairs), row["best"] if pairs else 0, [g for g, _ in pairs] + [-1] * pad, [s for _, s in pairs] + [0] * pad)


def candidates(row):
    """The row in abundref's terms: [(genome, delta)] in ascending genome id ([] for an empty row)."""
    return [(g, row["best"] - s) for g, s in sorted(row["pairs"].items())]


def info(rows):
    """n_rows_used, n_cands, n_truncated_reads of mnc_carry_info."""
    used = [r for r in rows if r["pairs"]]
    return len(used), sum(len(r["pairs"]) for r in used), sum(1 for r in rows if r["truncated"])
