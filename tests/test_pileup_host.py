"""Per-base pileup (include/monica_amd.h, "pileup"): what needs no GPU -- the reference model tests/pileref.py on hand-made
records whose answer follows from the contract alone, the binding against the header, the argument / device errors of the
C-ABI and the variants TSV byte for byte."""
import ctypes as C
import os
import re

import numpy as np

import pileref
import util

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "monica_amd.h")
REF = np.frombuffer(b"ACGTACGGTCATTGCA", dtype=np.uint8)          # 16 bases


def rec(rs, cigar, read, rev=0, rid=0, selected=True, qs=0, qe=None):
    return (rid, rs, cigar, rev, qs, len(read) if qe is None else qe, read, selected)


def plane(P, k):
    return P[0][k].tolist()


# ---------------------------------------------------------------- pileref on known answers
def test_both_strands_count_the_same_allele():
    # the reads cover reference bases 2 .. 9 (GTACGGTC) and say T instead of the C at base 5
    fwd = b"GTATGGTC"
    rev = util.revcomp(np.frombuffer(fwd, dtype=np.uint8)).tobytes()        # what a read of the other strand holds
    assert rev == b"GACCATAC"
    P = pileref.tally([rec(2, [(8, "M")], fwd), rec(2, [(8, "M")], rev, rev=1)], [REF])
    assert plane(P, pileref.DEPTH) == [0, 0] + [2] * 8 + [0] * 6
    assert plane(P, pileref.T) == [0, 0, 0, 2, 0, 2, 0, 0, 2, 0] + [0] * 6   # bases 3 and 8 are T in the reference, base 5 is the SNP
    assert plane(P, pileref.C)[5] == 0 and plane(P, pileref.C)[9] == 2
    assert P[0][1:6].sum(axis=0).tolist() == plane(P, pileref.DEPTH)          # every M column is one observation
    v = pileref.variants(P, [REF], -1, 1, 1, 0)
    assert [(int(x["pos"]), x["ref"], x["alt"], int(x["count"]), int(x["span"])) for x in v] == [(5, b"C", b"T", 2, 2)]
    # a clipped reverse read: qs / qe are forward-strand coordinates, column 0 is the complement of read base qe - 1
    P = pileref.tally([rec(2, [(4, "M")], b"NN" + rev, rev=1, qs=6, qe=10)], [REF])       # read bases 6 .. 9 = "ATAC" -> GTAT
    assert plane(P, pileref.DEPTH) == [0, 0, 1, 1, 1, 1] + [0] * 10
    assert plane(P, pileref.T)[5] == 1 and plane(P, pileref.G)[2] == 1


def test_an_insertion_counts_once_at_the_base_on_its_left():
    read = b"GTA" + b"TTTTT" + b"CGG"
    P = pileref.tally([rec(2, [(3, "M"), (5, "I"), (3, "M")], read)], [REF])
    assert plane(P, pileref.INS) == [0, 0, 0, 0, 1] + [0] * 11                # once, at base 4, whatever its length
    assert plane(P, pileref.DEPTH) == [0, 0] + [1] * 6 + [0] * 8
    assert sum(plane(P, k)[p] for k in range(1, 6) for p in range(16)) == 6   # the inserted bases are not observations
    # an insertion with no reference column on its left is not counted; one behind a deletion sits on the deleted base
    P = pileref.tally([rec(2, [(2, "I"), (3, "M"), (2, "D"), (1, "I"), (2, "M")], b"TT" + b"GTA" + b"A" + b"GT")], [REF])
    assert plane(P, pileref.INS) == [0] * 6 + [1] + [0] * 9
    assert plane(P, pileref.DEL) == [0] * 5 + [1, 1] + [0] * 9


def test_a_deletion_counts_every_base_and_no_depth():
    P = pileref.tally([rec(1, [(3, "M"), (4, "D"), (2, "M")], b"CGTTC")], [REF])
    assert plane(P, pileref.DEL) == [0] * 4 + [1] * 4 + [0] * 8
    assert plane(P, pileref.DEPTH) == [0, 1, 1, 1, 0, 0, 0, 0, 1, 1] + [0] * 6
    v = pileref.variants(P, [REF], 0, 1, 1, 1000)
    assert [(int(x["pos"]), x["alt"], int(x["span"])) for x in v] == [(4, b"-", 1), (5, b"-", 1), (6, b"-", 1), (7, b"-", 1)]
    assert pileref.consensus(P, [REF], 0, 0, 11, 1) == b"NCGT----TCN"


def test_n_on_either_side_and_unselected_records():
    ref = REF.copy()
    ref[4] = ord("N")
    P = pileref.tally([rec(2, [(5, "M")], b"GTANG"), rec(2, [(5, "M")], b"GTCCG", selected=False)], [ref])
    assert plane(P, pileref.DEPTH)[2:7] == [1] * 5
    assert plane(P, pileref.A)[4] == 1                                        # over the reference N: its own base
    assert plane(P, pileref.N)[5] == 1 and plane(P, pileref.C)[5] == 0        # a query N is an observation of N
    # a reference N calls nothing; an observation of N is no allele
    assert len(pileref.variants(P, [ref], -1, 1, 1, 0)) == 0
    assert pileref.consensus(P, [ref], 0, 2, 7, 1) == b"GTACG"                # base 5: all counts 0, the reference wins the tie


def test_consensus_tie_rules():
    def planes(a=0, c=0, g=0, t=0, d=0):
        P = np.zeros((8, 1), dtype=np.int64)
        P[pileref.A], P[pileref.C], P[pileref.G], P[pileref.T], P[pileref.DEL] = a, c, g, t, d
        P[pileref.DEPTH] = a + c + g + t
        return [P]
    ref_g = [np.frombuffer(b"G", dtype=np.uint8)]
    assert pileref.consensus(planes(a=3, g=3, t=3), ref_g, 0, 0, 1, 1) == b"G"        # the reference is among the tied
    assert pileref.consensus(planes(c=3, t=3, g=2), ref_g, 0, 0, 1, 1) == b"C"        # it is not: the first in A C G T DEL
    assert pileref.consensus(planes(t=3, d=3), ref_g, 0, 0, 1, 1) == b"T"
    assert pileref.consensus(planes(g=2, d=3), ref_g, 0, 0, 1, 1) == b"-"
    assert pileref.consensus(planes(a=4, g=3), ref_g, 0, 0, 1, 1) == b"A"
    assert pileref.consensus(planes(a=2, d=2), ref_g, 0, 0, 1, 5) == b"N"             # span 4 < 5
    assert pileref.consensus(planes(a=2, d=3), ref_g, 0, 0, 1, 5) == b"-"             # span = depth + del = 5


def test_permille_comparison_at_equality():
    P = np.zeros((8, 1), dtype=np.int64)
    P[pileref.DEPTH], P[pileref.A], P[pileref.G], P[pileref.DEL], P[pileref.INS] = 7, 2, 5, 1, 2        # span 8: A is 250 permille
    ref_g = [np.frombuffer(b"G", dtype=np.uint8)]
    alts = lambda *thr: [x["alt"] for x in pileref.variants([P], ref_g, -1, *thr)]
    assert alts(8, 1, 250) == [b"A", b"+"]                                    # 2 * 1000 >= 250 * 8: equality is a call
    assert alts(8, 1, 251) == []
    assert alts(8, 1, 125) == [b"A", b"-", b"+"]                              # 1 * 1000 >= 125 * 8
    assert alts(8, 2, 125) == [b"A", b"+"]
    assert alts(9, 1, 0) == []                                                # span < min_depth
    assert alts(1, 1, 0) == [b"A", b"-", b"+"]                                # the reference base is never a variant


# ---------------------------------------------------------------- binding against the header
def test_binding_matches_the_header(capi):
    text = open(HEADER).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+MNC_PILE_(\w+)\s+(\d+)", text)}
    assert defs.pop("PLANES") == len(capi.PILE_PLANES) == 8
    assert [k for k, _ in sorted(defs.items(), key=lambda kv: kv[1])] == [p.upper() for p in capi.PILE_PLANES] and sorted(defs.values()) == list(range(8))
    assert capi.PILE_PLANES == pileref.PLANES == ("depth", "A", "C", "G", "T", "N", "DEL", "INS")
    for name in ("create", "free", "reset", "device_bytes", "device", "fetch_counts", "call_variants", "consensus"):
        assert "mnc_pileup_" + name in capi.EXPORTS and hasattr(capi.lib(), "mnc_pileup_" + name)
    assert "mnc_engine_add_pileup" in capi.EXPORTS and hasattr(capi.lib(), "mnc_engine_add_pileup")
    # mnc_variant_t: four int32, ref, alt, two bytes of padding
    body = re.search(r"typedef struct \{([^}]*)\} mnc_variant_t;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["int32_t rid, pos", "int32_t span", "int32_t count", "uint8_t ref", "uint8_t alt", "uint8_t pad[2]"]
    assert capi.VARIANT_DTYPE.itemsize == 20 and capi.VARIANT_DTYPE == pileref.VARIANT_DTYPE
    assert capi.VARIANT_DTYPE.names == ("rid", "pos", "span", "count", "ref", "alt", "pad")
    assert [capi.VARIANT_DTYPE.fields[n][1] for n in capi.VARIANT_DTYPE.names] == [0, 4, 8, 12, 16, 17, 18]
    for name in ("reset", "counts", "variants", "consensus", "device"):
        assert callable(getattr(capi.Pileup, name))
    assert callable(capi.Engine.add_pileup)
    limits = text[text.index("limits, and what happens at each"):text.index("---- classify")]
    assert "mnc_engine_add_pileup: MNC_ERR_UNSUPPORTED" in limits and "mnc_engine_add_pileup: MNC_ERR_ARG" in limits
    assert "inserted bases are not stored" in limits and "every plane of mnc_pileup holds int32" in limits


def test_python_signatures():
    import inspect
    from monica_amd import aligner, mappy_compat
    assert list(inspect.signature(aligner.aligner_coverage).parameters)[-2:] == ["coverage", "pileup"]
    assert list(inspect.signature(aligner.multi_threaded_aligner).parameters)[-2:] == ["coverage", "pileup"]
    assert "pileup" not in inspect.signature(aligner.aligner).parameters
    p = inspect.signature(mappy_compat.Aligner.map_batch).parameters
    assert p["pileup"].default is None and "pileup_what" in p and callable(mappy_compat.Aligner.pileup)


# ---------------------------------------------------------------- errors that need no device
def test_create_without_a_device_and_argument_errors(capi):
    L = capi.lib()
    idx = capi.Index.from_seqs(["a:1"], [np.frombuffer(b"ACGTTGCAAGGCTTAACCGGTATGCATGCAAT" * 40, dtype=np.uint8)])
    h = C.c_void_p()
    n_dev = capi.device_count()                                    # a device that does not exist -- without a GPU that is device 0
    assert L.mnc_pileup_create(idx._h, n_dev, C.byref(h)) == capi.ERR_NODEVICE and not h.value
    try:
        capi.Pileup(idx, n_dev)
        raise AssertionError("no error")
    except capi.MncError as err:
        assert err.code == capi.ERR_NODEVICE
    assert L.mnc_pileup_create(None, n_dev, C.byref(h)) == capi.ERR_ARG
    assert L.mnc_pileup_create(idx._h, n_dev, None) == capi.ERR_ARG
    n = C.c_int64(7)
    assert L.mnc_pileup_reset(None) == capi.ERR_ARG
    assert L.mnc_pileup_device_bytes(None, C.byref(n)) == capi.ERR_ARG
    assert L.mnc_pileup_device(None, None, None, C.byref(n)) == capi.ERR_ARG
    assert L.mnc_pileup_fetch_counts(None, 0, 0, 0, None) == capi.ERR_ARG
    assert L.mnc_pileup_call_variants(None, -1, 1, 1, 0, None, 0, C.byref(n)) == capi.ERR_ARG
    assert L.mnc_pileup_consensus(None, 0, 0, 0, 1, None) == capi.ERR_ARG
    assert L.mnc_engine_add_pileup(None, None, capi.COV_GATED) == capi.ERR_ARG
    assert n.value == 7
    L.mnc_pileup_free(None)                                        # a no-op


# ---------------------------------------------------------------- the TSV
def test_variants_tsv_byte_for_byte(capi, tmp_path):
    from monica_amd import aligner

    class Index:
        genome_names = ["Escherichia coli", "Bacillus subtilis"]
        contig_names = ["NC_1.1", "NC_2.1", "NC_2.2"]
        contig_genome = [0, 1, 1]

    v = np.array([(0, 41, 12, 12, b"A", b"G", 0), (2, 7, 9, 3, b"T", b"-", 0), (2, 7, 9, 2, b"T", b"+", 0)], dtype=capi.VARIANT_DTYPE)
    path = tmp_path / "s.variants.tsv"
    aligner.write_variants_tsv(Index, v, str(path))
    want = ("genome\tcontig\tpos\tref\talt\tcount\tspan\tpermille\n"
            "Escherichia coli\tNC_1.1\t41\tA\tG\t12\t12\t1000\n"
            "Bacillus subtilis\tNC_2.2\t7\tT\t-\t3\t9\t333\n"
            "Bacillus subtilis\tNC_2.2\t7\tT\t+\t2\t9\t222\n")
    assert path.read_bytes() == want.encode()
    assert pileref.variants_tsv(v, ["Escherichia coli", "Bacillus subtilis", "Bacillus subtilis"], Index.contig_names) == want
    aligner.write_variants_tsv(Index, v[:1], str(path))            # a second index part appends its rows, without a header
    assert path.read_bytes() == (want + want.splitlines(True)[1]).encode()
    aligner.write_variants_tsv(Index, v[:0], str(tmp_path / "none.tsv"))
    assert (tmp_path / "none.tsv").read_text() == want.splitlines(True)[0]
