"""Insertion alleles of the pileup (include/monica_amd.h, "pileup": insertion alleles): what needs no GPU -- the argument
and device errors of the new entry points, mnc_insertion_t against the header, and the TSV rows against tests/insref.py."""
import ctypes as C
import os
import re

import numpy as np

import insref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "monica_amd.h")


def test_null_handles_and_a_store_on_a_missing_device(capi):
    L = capi.lib()
    n, m = C.c_int64(7), C.c_int64(7)
    assert L.mnc_pileup_store_insertions(None, 100, 100) == capi.ERR_ARG
    assert L.mnc_pileup_add_insertion_list(None, 0, None, None, None, None, None, None) == capi.ERR_ARG
    assert L.mnc_pileup_insertion_info(None, C.byref(n), None, None, None, None, None) == capi.ERR_ARG
    assert L.mnc_pileup_call_insertions(None, -1, 0, 1, 0, None, 0, C.byref(n), None, 0, C.byref(m)) == capi.ERR_ARG
    assert L.mnc_pileup_consensus_ins(None, 0, 0, 0, 1, None, 0, C.byref(n)) == capi.ERR_ARG
    assert n.value == m.value == 7
    idx = capi.Index.from_seqs(["a:1"], [np.frombuffer(b"ACGTTGCAAGGCTTAACCGGTATGCATGCAAT" * 40, dtype=np.uint8)])
    try:
        capi.Pileup(idx, capi.device_count(), insertions=(100, 100))      # a device that does not exist
        raise AssertionError("no error")
    except capi.MncError as err:
        assert err.code == capi.ERR_NODEVICE


def test_insertion_record_matches_the_header(capi):
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} mnc_insertion_t;", text).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["int32_t rid, pos, span, count, len", "int32_t pad", "int64_t base_off"]
    assert capi.INSERTION_DTYPE == insref.DTYPE and capi.INSERTION_DTYPE.itemsize == 32
    assert [capi.INSERTION_DTYPE.fields[k][1] for k in capi.INSERTION_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24]
    for name in ("store_insertions", "add_insertion_list", "insertion_info", "call_insertions", "consensus_ins"):
        assert "mnc_pileup_" + name in capi.EXPORTS and hasattr(capi.lib(), "mnc_pileup_" + name)


def test_variants_tsv_with_insertion_alleles(capi, tmp_path):
    from monica_amd import aligner

    class Index:
        genome_names = ["Escherichia coli", "Bacillus subtilis"]
        contig_names = ["NC_1.1", "NC_2.1", "NC_2.2"]
        contig_genome = [0, 1, 1]

    v = np.array([(0, 41, 12, 12, b"A", b"G", 0), (0, 41, 12, 7, b"A", b"+", 0), (2, 7, 9, 3, b"T", b"-", 0), (2, 7, 9, 5, b"T", b"+", 0)], dtype=capi.VARIANT_DTYPE)
    called = (np.array([(0, 41, 12, 7, 2, 0, 0), (2, 7, 9, 3, 1, 0, 2), (2, 7, 9, 2, 3, 0, 3)], dtype=capi.INSERTION_DTYPE), [b"GT", b"N", b"ACA"])
    path = tmp_path / "s.variants.tsv"
    aligner.write_variants_tsv(Index, v, str(path), called)
    assert aligner.pileup_options(True) == (aligner.PILEUP_THRESHOLDS, None) and aligner.pileup_options((2, 1, 0)) == ((2, 1, 0), None)
    assert aligner.pileup_options({"insertions": (100, 50)}) == (aligner.PILEUP_THRESHOLDS, (100, 50))
    assert aligner.pileup_options({"thresholds": (4, 2, 300), "insertions": (1, 0)}) == ((4, 2, 300), (1, 0))
    want = ("genome\tcontig\tpos\tref\talt\tcount\tspan\tpermille\n"
            "Escherichia coli\tNC_1.1\t41\tA\tG\t12\t12\t1000\n"
            "Escherichia coli\tNC_1.1\t41\tA\t+GT\t7\t12\t583\n"
            "Bacillus subtilis\tNC_2.2\t7\tT\t-\t3\t9\t333\n"
            "Bacillus subtilis\tNC_2.2\t7\tT\t+N\t3\t9\t333\n"
            "Bacillus subtilis\tNC_2.2\t7\tT\t+ACA\t2\t9\t222\n")
    assert path.read_text() == want == insref.variants_tsv(v, called, ["Escherichia coli", "Bacillus subtilis", "Bacillus subtilis"], Index.contig_names)
