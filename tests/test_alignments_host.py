"""Host side of the alignment records (include/monica_amd.h, "alignment records"): contig bases out of an index
(mnc_index_getseq, Aligner.seq), PAF lines from records (mnc_fastq_write_paf), and the cs / MD reference the GPU
tests compare against (tests/alnref.py) on cases worked out by hand.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import alnref
from monica_amd import synth


# ---------------------------------------------------------------- mnc_index_getseq / Aligner.seq
@pytest.fixture(scope="module")
def seq_index(capi):
    g0 = synth.genome(0x51, 5000).copy()
    g0[1200:1237] = ord("N")                                    # an N run; its ends are not word-aligned in the 4-bit store
    g1 = synth.genome(0x52, 3001).copy()
    g1[0] = ord("n")
    g1[-1] = ord("N")
    names = ["taxA:ctg0", "taxB:ctg1"]
    return names, [g0, g1], capi.Index.from_seqs(names, [g0, g1])


def _upper_n(a):
    s = bytes(a).upper()
    return bytes(c if c in b"ACGT" else ord("N") for c in s)


def test_getseq_slices(capi, seq_index):
    names, seqs, idx = seq_index
    for rid, g in enumerate(seqs):
        want = _upper_n(g)
        assert idx.getseq(rid) == want                          # the whole contig
        assert idx.getseq(rid, 0, len(g)) == want
        for a, b in ((1190, 1250), (1200, 1237), (1, 2), (7, 16), (0, 1), (len(g) - 1, len(g)), (len(g) - 9, len(g)), (0, 9)):
            assert idx.getseq(rid, a, b) == want[a:b], (rid, a, b)
        for p in (0, 1237, len(g)):                             # start == end: nothing, and no error
            assert idx.getseq(rid, p, p) == b""
    assert b"N" * 37 in idx.getseq(0) and idx.getseq(0).count(b"N") == 37
    assert idx.getseq(1)[:1] == b"N" and idx.getseq(1)[-1:] == b"N"


def test_getseq_out_of_range_is_err_arg(capi, seq_index):
    names, seqs, idx = seq_index
    L = capi.lib()
    buf = C.create_string_buffer(64)
    n0 = len(seqs[0])
    for rid, a, b in ((0, -1, 5), (0, 10, 9), (0, 0, n0 + 1), (0, n0 + 1, n0 + 1), (0, n0, n0 + 2), (-1, 0, 5), (2, 0, 5), (1, 0, n0)):
        assert L.mnc_index_getseq(idx._h, rid, a, b, buf) == capi.ERR_ARG, (rid, a, b)
    assert L.mnc_index_getseq(None, 0, 0, 5, buf) == capi.ERR_ARG
    assert L.mnc_index_getseq(idx._h, 0, 0, 5, None) == capi.ERR_ARG
    with pytest.raises(capi.MncError):
        idx.getseq(0, 5, n0 + 1)


def test_aligner_seq(capi, seq_index, tmp_path):
    from monica_amd import mappy_compat
    names, seqs, idx = seq_index
    path = str(tmp_path / "two.idx")
    idx.save(path)
    al = mappy_compat.Aligner(fn_idx_in=path)
    assert al
    want = _upper_n(seqs[0]).decode()
    assert al.seq(names[0]) == want                             # mappy's defaults: the whole contig
    assert al.seq(names[0], 1190, 1250) == want[1190:1250]
    assert al.seq(names[0], 4990) == want[4990:]
    assert al.seq(names[0], 4990, 10 ** 9) == want[4990:]       # end beyond the contig is clipped, as mappy does
    assert al.seq(names[1], 0, 1) == "N"
    assert al.seq("no such contig") is None
    assert al.seq(names[0], 10, 10) is None and al.seq(names[0], 5000) is None and al.seq(names[0], 20, 10) is None


# ---------------------------------------------------------------- mnc_fastq_write_paf
FASTQ = ("@read/1 first extra words\nACGTACGTAC\n+\nIIIIIIIIII\n"
         "@lonely\nACGT\n+\nIIII\n"
         "@r3 x\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n")


def _rec(capi, **kw):
    r = np.zeros(1, dtype=capi.ALN_DTYPE)
    for k, v in kw.items():
        r[k] = v
    return r


@pytest.fixture()
def paf_world(capi, seq_index, tmp_path):
    names, seqs, idx = seq_index
    fq_path = str(tmp_path / "three.fastq")
    with open(fq_path, "w") as f:
        f.write(FASTQ)
    rd = capi.FastqReader(fq_path)
    assert rd.next() == 3
    P = capi.ALN_PRIMARY
    recs = np.concatenate([
        # read 0: a forward primary and a secondary on the other contig
        _rec(capi, read=0, rid=0, rev=0, qs=1, qe=9, rs=100, re=109, mapq=60, mlen=7, blen=9, nm=2, score=55, cnt=4,
             dp_score=10, dp_max=12, n_ambi=0, flags=P | capi.ALN_GATED | 1 << 8, n_cigar=3, cigar_off=0, cs_off=0, cs_len=11, md_off=0, md_len=5),
        _rec(capi, read=0, rid=1, rev=1, qs=0, qe=10, rs=2000, re=2010, mapq=0, mlen=10, blen=10, nm=0, score=40, cnt=3,
             dp_score=20, dp_max=20, n_ambi=0, flags=1 << 8, n_cigar=1, cigar_off=3, cs_off=11, cs_len=3, md_off=5, md_len=2),
        # read 1: nothing; read 2: a reverse-strand primary with an ambiguous base
        _rec(capi, read=2, rid=1, rev=1, qs=2, qe=20, rs=0, re=19, mapq=17, mlen=16, blen=19, nm=4, score=70, cnt=5,
             dp_score=-3, dp_max=25, n_ambi=1, flags=P | 1 << 8, n_cigar=2, cigar_off=4, cs_off=14, cs_len=8, md_off=7, md_len=6)])
    offs = np.array([0, 2, 2, 3], dtype=np.int64)
    cigar = np.array([4 << 4 | 0, 1 << 4 | 2, 4 << 4 | 0, 10 << 4 | 0, 18 << 4 | 0, 1 << 4 | 2], dtype=np.uint32)
    cs = np.frombuffer(b":3*ag-t:4:X" + b":10" + b":17*na-c", dtype=np.uint8)
    md = np.frombuffer(b"3A^T4" + b"10" + b"17N^C0", dtype=np.uint8)
    return dict(idx=idx, rd=rd, recs=recs, offs=offs, cigar=cigar, cs=cs, md=md, tmp=tmp_path)


L0 = "read/1\t10\t1\t9\t+\ttaxA:ctg0\t5000\t100\t109\t7\t9\t60\ttp:A:P\tcm:i:4\ts1:i:55\tNM:i:2\tAS:i:10\tms:i:12\tnn:i:0"
L1 = "read/1\t10\t0\t10\t-\ttaxB:ctg1\t3001\t2000\t2010\t10\t10\t0\ttp:A:S\tcm:i:3\ts1:i:40\tNM:i:0\tAS:i:20\tms:i:20\tnn:i:0"
L2 = "r3\t20\t2\t20\t-\ttaxB:ctg1\t3001\t0\t19\t16\t19\t17\ttp:A:P\tcm:i:5\ts1:i:70\tNM:i:4\tAS:i:-3\tms:i:25\tnn:i:1"


def test_write_paf_exact_lines(capi, paf_world):
    w = paf_world
    out = str(w["tmp"] / "all.paf")
    w["rd"].write_paf(w["idx"], w["offs"], w["recs"], out, cigar=w["cigar"], cs=w["cs"], md=w["md"])
    assert open(out).read() == (L0 + "\tcg:Z:4M1D4M\tcs:Z::3*ag-t:4:X\tMD:Z:3A^T4\n"
                                + L1 + "\tcg:Z:10M\tcs:Z::10\tMD:Z:10\n"
                                + L2 + "\tcg:Z:18M1D\tcs:Z::17*na-c\tMD:Z:17N^C0\n")
    # the file is appended to; primary-only mode drops the secondary
    w["rd"].write_paf(w["idx"], w["offs"], w["recs"], out, cigar=w["cigar"], primary_only=True)
    assert open(out).read().splitlines()[3:] == [L0 + "\tcg:Z:4M1D4M", L2 + "\tcg:Z:18M1D"]


def test_write_paf_each_pool_alone(capi, paf_world):
    w = paf_world
    tails = dict(cigar=["\tcg:Z:4M1D4M", "\tcg:Z:10M", "\tcg:Z:18M1D"], cs=["\tcs:Z::3*ag-t:4:X", "\tcs:Z::10", "\tcs:Z::17*na-c"],
                 md=["\tMD:Z:3A^T4", "\tMD:Z:10", "\tMD:Z:17N^C0"])
    for which in (None, "cigar", "cs", "md"):
        out = str(w["tmp"] / f"only_{which}.paf")
        kw = {which: w[which]} if which else {}
        w["rd"].write_paf(w["idx"], w["offs"], w["recs"], out, **kw)
        t = tails[which] if which else ["", "", ""]
        assert open(out).read() == L0 + t[0] + "\n" + L1 + t[1] + "\n" + L2 + t[2] + "\n", which


def test_write_paf_no_records_and_errors(capi, paf_world):
    w = paf_world
    out = str(w["tmp"] / "none.paf")
    w["rd"].write_paf(w["idx"], np.zeros(4, dtype=np.int64), np.zeros(0, dtype=capi.ALN_DTYPE), out)
    assert open(out).read() == ""
    L = capi.lib()
    bad = str(w["tmp"] / "no_such_dir" / "x.paf")
    rc = L.mnc_fastq_write_paf(w["rd"]._h, w["idx"]._h, w["offs"].ctypes.data, w["recs"].ctypes.data, None, None, None, 0, bad.encode())
    assert rc == capi.ERR_IO and b"no_such_dir" in L.mnc_last_error()
    assert L.mnc_fastq_write_paf(None, w["idx"]._h, w["offs"].ctypes.data, w["recs"].ctypes.data, None, None, None, 0, out.encode()) == capi.ERR_ARG
    assert L.mnc_fastq_write_paf(w["rd"]._h, w["idx"]._h, w["offs"].ctypes.data, None, None, None, None, 0, out.encode()) == capi.ERR_ARG
    wrong = w["recs"].copy()
    wrong["rid"][0] = 7                                         # a contig the index does not have: refused, nothing written
    assert L.mnc_fastq_write_paf(w["rd"]._h, w["idx"]._h, w["offs"].ctypes.data, wrong.ctypes.data, None, None, None, 0, out.encode()) == capi.ERR_ARG
    assert open(out).read() == ""


def test_record_layout(capi):
    d = capi.ALN_DTYPE
    assert d.itemsize == 104 and d.fields["cigar_off"][1] == 72 and d.fields["cs_off"][1] == 80 and d.fields["md_off"][1] == 88
    assert d.fields["cs_len"][1] == 96 and d.fields["md_len"][1] == 100 and d.fields["flags"][1] == 64 and d.fields["n_cigar"][1] == 68


def test_merge_of_two_calls_by_read_ordinal(capi):
    """`Aligner.map_batch_alignments` classifies a mixed long / short batch as two calls; the merge puts the records back
    in read order and rewrites their pool offsets."""
    from monica_amd import mappy_compat
    def part(sel, per_read):
        recs, cig, cs, md, offs = [], [], b"", b"", [0]
        for k, n in enumerate(per_read):
            for j in range(n):
                tag = b"%d.%d" % (sel[k], j)
                recs.append(_rec(capi, read=k, rid=sel[k], n_cigar=j + 1, cigar_off=len(cig), cs_off=len(cs), cs_len=len(tag), md_off=len(md), md_len=len(tag) + 1))
                cig += [sel[k] * 100 + j] * (j + 1)
                cs += tag
                md += tag + b"!"
            offs.append(len(recs))
        return (np.array(sel), np.array(offs, dtype=np.int64), np.concatenate(recs) if recs else np.zeros(0, dtype=capi.ALN_DTYPE),
                np.array(cig, dtype=np.uint32), np.frombuffer(cs, dtype=np.uint8), np.frombuffer(md, dtype=np.uint8))
    offs, recs, cig, cs, md = mappy_compat._merge_alignments(5, [part([0, 2, 3], [2, 0, 1]), part([1, 4], [3, 1])])
    assert offs.tolist() == [0, 2, 5, 5, 6, 7]
    assert recs["read"].tolist() == [0, 0, 1, 1, 1, 3, 4] and recs["rid"].tolist() == [0, 0, 1, 1, 1, 3, 4]
    for a in recs:
        j = int(a["n_cigar"]) - 1
        tag = b"%d.%d" % (a["rid"], j)
        assert cig[a["cigar_off"]:a["cigar_off"] + a["n_cigar"]].tolist() == [int(a["rid"]) * 100 + j] * (j + 1)
        assert bytes(cs[a["cs_off"]:a["cs_off"] + a["cs_len"]]) == tag and bytes(md[a["md_off"]:a["md_off"] + a["md_len"]]) == tag + b"!"
    assert recs["cigar_off"].tolist() == np.concatenate([[0], np.cumsum(recs["n_cigar"])[:-1]]).tolist()


# ---------------------------------------------------------------- tests/alnref.py on cases worked out by hand
def _ref(cigar, t, q):
    return alnref.cs_md(cigar, alnref.codes(t), alnref.codes(q))


def test_alnref_perfect_match():
    assert _ref([(8, "M")], "ACGTACGT", "ACGTACGT") == (":8", "8")
    assert _ref([(12, 0)], "ACGTACGTACGT", "acgtacgtacgu") == (":12", "12")       # case and U do not matter; numeric ops


def test_alnref_mismatch_at_the_first_and_last_column():
    #                  t: A C G T A      q: C C G T A
    assert _ref([(5, "M")], "ACGTA", "CCGTA") == ("*ac:4", "0A4")
    assert _ref([(5, "M")], "ACGTA", "ACGTG") == (":4*ag", "4A")
    assert _ref([(5, "M")], "ACGTA", "TCGTC") == ("*at:3*ac", "0A3A")
    assert _ref([(2, "M")], "AC", "CA") == ("*ac*ca", "0A0C")


def test_alnref_deletion_followed_by_a_mismatch():
    # target ACG AC TTA, query ACG -- GTA: 3M 2D 3M, first column after the deletion T against G
    cs, md = _ref([(3, "M"), (2, "D"), (3, "M")], "ACGACTTA", "ACGGTA")
    assert cs == ":3-ac*tg:2"
    assert md == "3^AC0T2"
    # ... and a match right after it: the counter starts again at the deletion
    assert _ref([(3, "M"), (2, "D"), (3, "M")], "ACGACTTA", "ACGTTA") == (":3-ac:3", "3^AC3")
    # a deletion before any match: MD opens with 0
    assert _ref([(1, "D"), (2, "M")], "GAC", "AC") == ("-g:2", "0^G2")


def test_alnref_insertion_between_two_match_runs():
    # MD's run carries across the insertion (3 + 4 = 7), cs's does not
    assert _ref([(3, "M"), (2, "I"), (4, "M")], "ACGTACG", "ACGGGTACG") == (":3+gg:4", "7")
    # an insertion directly followed by a mismatch; the mismatch closes MD's carried run
    assert _ref([(3, "M"), (1, "I"), (3, "M")], "ACGTAC", "ACGCAAC") == (":3+c*ta:2", "3T2")
    # two M operations in a row: cs ends a run with its operation
    assert _ref([(2, "M"), (3, "M")], "ACGTA", "ACGTA") == (":2:3", "5")


def test_alnref_n_against_n_and_n_against_a_base():
    assert _ref([(5, "M")], "ACNTA", "ACNTA") == (":5", "5")                      # n against n: a match
    assert _ref([(5, "M")], "ACNTA", "ACXTA") == (":5", "5")                      # any non-ACGTU byte is n
    assert _ref([(5, "M")], "ACNTA", "ACGTA") == (":2*ng:2", "2N2")
    assert _ref([(5, "M")], "ACGTA", "ACNTA") == (":2*gn:2", "2G2")
    assert _ref([(2, "M"), (2, "D"), (1, "M"), (1, "I"), (1, "M")], "ACNNGT", "ACGNT") == (":2-nn:1+n:1", "2^NN2")


def test_alnref_strand_and_span_checks():
    read = b"AACCGGTTAN"
    assert alnref.query_codes(read, 2, 8, 0).tolist() == [1, 1, 2, 2, 3, 3]
    # reverse strand: column 0 is the complement of read base qe - 1
    assert alnref.query_codes(read, 2, 10, 1).tolist() == [4, 3, 0, 0, 1, 1, 2, 2]
    reg = dict(rs=1, re=7, qs=2, qe=8, rev=1)
    # read[2:8] = CCGGTT, reverse complement AACCGG; contig[1:7] = AACCGG
    assert alnref.cs_md_of_hit(reg, [(6, "M")], b"TAACCGGT", read) == (":6", "6")
    with pytest.raises(ValueError):
        alnref.cs_md([(5, "M")], alnref.codes("ACGT"), alnref.codes("ACGT"))
