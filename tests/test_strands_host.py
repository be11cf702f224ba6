"""The strand store of the pileup (include/monica_amd.h, "pileup": strands and base qualities): what needs no GPU -- the
option parsing of `pileup=`, the variants TSV with its two more columns byte for byte and the 28-byte record against the header."""
import re

import numpy as np
import pytest

import strandref
import test_pileup_host as host


def test_the_pileup_dict_asks_for_the_strand_store():
    from monica_amd import aligner
    assert aligner.pileup_strand_options(True) is None and aligner.pileup_strand_options((2, 1, 500)) is None
    assert aligner.pileup_strand_options({"strands": True}) == (0, 0, 0)
    assert aligner.pileup_strand_options({"min_qual": 12, "min_strand_permille": 50}) == (12, 0, 50)
    assert aligner.pileup_options({"strands": True, "min_qual": 7}) == (aligner.PILEUP_THRESHOLDS, None)     # its return shape stays
    for bad in ({"min_qual": 94}, {"min_qual": -1}, {"min_strand_count": -1}):
        with pytest.raises(ValueError):
            aligner.pileup_strand_options(bad)


def test_variants_tsv_with_the_strand_columns(capi, tmp_path):
    from monica_amd import aligner

    class Index:
        genome_names = ["Escherichia coli", "Bacillus subtilis"]
        contig_names = ["NC_1.1", "NC_2.1", "NC_2.2"]
        contig_genome = [0, 1, 1]

    v = np.array([(0, 41, 12, 12, b"A", b"G", 0, 5, 5), (2, 7, 9, 3, b"T", b"-", 0, 1, 4)], dtype=capi.VARIANT_STRAND_DTYPE)
    path = tmp_path / "s.variants.tsv"
    aligner.write_variants_tsv(Index, v, str(path))
    assert path.read_bytes() == (b"genome\tcontig\tpos\tref\talt\tcount\tspan\tpermille\tcount_fwd\tspan_fwd\n"
                                 b"Escherichia coli\tNC_1.1\t41\tA\tG\t12\t12\t1000\t5\t5\n"
                                 b"Bacillus subtilis\tNC_2.2\t7\tT\t-\t3\t9\t333\t1\t4\n")


def test_the_record_of_28_bytes_matches_the_header(capi):
    body = re.search(r"typedef struct \{([^}]*)\} mnc_variant_strand_t;", open(host.HEADER).read()).group(1)
    assert re.sub(r"/\*.*?\*/|\s", "", body, flags=re.S) == "int32_trid,pos;int32_tspan;int32_tcount;uint8_tref;uint8_talt;uint8_tpad[2];int32_tcount_fwd,span_fwd;"
    d = capi.VARIANT_STRAND_DTYPE
    assert d.itemsize == 28 and d == strandref.VARIANT_STRAND_DTYPE and d.names[:7] == capi.VARIANT_DTYPE.names
    assert [d.fields[n][1] for n in d.names] == [0, 4, 8, 12, 16, 17, 18, 20, 24]
    assert (capi.PILE_FWD, capi.PILE_LOWQ, capi.PILE_LOWQ_FWD, len(capi.PILE_STRAND_PLANES)) == (strandref.FWD, strandref.LOWQ, strandref.LOWQ_FWD, 18)

