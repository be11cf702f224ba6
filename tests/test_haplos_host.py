"""Haplos (include/monica_amd.h, "haplos"): what needs no GPU -- the symbols, the argument errors of mnc_haplos_create, which
are all answered before a device is looked at, and tests/haploref.py on a corpus worked out by hand."""
import ctypes as C

import numpy as np
import pytest

import covref
import haploref
import util
from test_linkage_host import SEQ


def create(capi, rows, k):
    idx = capi.Index.from_seqs(["a:1", "b:1"], [SEQ, SEQ[::-1].copy()])
    s, h = np.array([(rid, pos, 0, 0, b"A", alt, 0) for rid, pos, alt in rows], dtype=capi.VARIANT_DTYPE), C.c_void_p()
    return capi.lib().mnc_haplos_create(idx._h, capi.device_count(), s.ctypes.data, len(s), k, C.byref(h)), h.value   # a device that does not exist


def test_the_symbols_exist(capi):
    for sym in ["mnc_haplos_" + n for n in ("create", "free", "reset", "device_bytes", "device", "fetch", "call")] + ["mnc_engine_add_haplos"]:
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym), sym
    assert capi.HAPLOS_MAX_K == 6 and capi.HAPLO_DTYPE.itemsize == 16 and callable(capi.Haplos.call) and callable(capi.Engine.add_haplos)
    from monica_amd import mappy_compat
    assert callable(mappy_compat.Aligner.haplos) and "haplos" in mappy_compat.Aligner.map_batch.__code__.co_varnames


@pytest.mark.parametrize("rows,k,word", (
    (((0, 5, b"C"), (0, 9, b"C")), 1, b"k 1 outside 2 .. 6"),
    (((0, 5, b"C"), (0, 9, b"C")), 7, b"k 7 outside 2 .. 6"),
    (((0, 5, b"C"), (0, 7, b"+")), 4, b"site 1 is an insertion allele"),
    (((0, 9, b"C"), (0, 5, b"C")), 4, b"site 1 does not ascend"),
    (((0, 5, b"C"), (1, 1280, b"C")), 4, b"site 1: position 1280 of contig 1 is outside the index"),
))
def test_create_argument_errors(capi, rows, k, word):
    rc, h = create(capi, rows, k)
    assert rc == capi.ERR_ARG and not h and word in capi.lib().mnc_last_error(), capi.lib().mnc_last_error()
    assert create(capi, ((0, 5, b"C"), (0, 5, b"-"), (1, 0, b"T")), 6) == (capi.ERR_NODEVICE, None)
    assert capi.lib().mnc_engine_add_haplos(None, None, capi.COV_GATED) == capi.ERR_ARG


def test_reference_on_six_records_by_hand():
    """Contig 0, bases [0, 50); sites at 10 (G>A), 20 (T>C), 30 (deleted), 40 (A>C) and one on contig 1, so window 3 does not
    exist.  The statements per record at the four sites (R, A, . = nothing):
      1 clean, forward                RRRR      2 A at 10, C at 20        AARR      3 base 30 deleted         RRAR
      4 C at 40, reverse strand       RRRA      5 G at 20, mapq 10        R.RR      6 bases [15, 35) of read 1  .RR."""
    t = [SEQ[:50].copy() for _ in range(5)]
    t[1][10], t[1][20], t[3][40], t[4][20] = b"ACCG"
    reads = [t[0], t[1], np.delete(t[2], 30), util.revcomp(t[3]), t[4]]
    reg = lambda **kw: dict(dict(id=0, parent=0, mapq=60, rid=0, rs=0, re=50, rev=0, qs=0, qe=50), **kw)
    per_read = [([reg(), reg(id=1, parent=1, rs=15, re=35, qs=15, qe=35)], [[(50, "M")], [(20, "M")]]), ([reg()], [[(50, "M")]]),
                ([reg(qe=49)], [[(30, "M"), (1, "D"), (19, "M")]]), ([reg(rev=1)], [[(50, "M")]]), ([reg(mapq=10)], [[(50, "M")]])]
    sites = np.array([(0, 10, 0, 0, b"G", b"A", 0), (0, 20, 0, 0, b"T", b"C", 0), (0, 30, 0, 0, b"A", b"-", 0), (0, 40, 0, 0, b"A", b"C", 0),
                      (1, 5, 0, 0, b"A", b"C", 0)], dtype=haploref.pileref.VARIANT_DTYPE)
    seqs = [SEQ, SEQ[::-1].copy()]
    hap = lambda what, k: haploref.tally(per_read, reads, what, 60, seqs, sites, k).tolist()
    assert hap(covref.ALL, 2) == [[3, 0, 0, 1], [3, 1, 1, 0], [3, 1, 1, 0], [0] * 4, [0] * 4]
    assert hap(covref.GATED, 2) == [[3, 0, 0, 1], [3, 1, 1, 0], [2, 1, 1, 0], [0] * 4, [0] * 4]
    h3 = haploref.tally(per_read, reads, covref.ALL, 60, seqs, sites, 3)
    assert h3.tolist() == [[2, 1, 0, 0, 0, 0, 1, 0], [1, 1, 1, 0, 1, 0, 0, 0]] + [[0] * 8] * 3
    n_haps, total, hist, rec = haploref.call(h3, sites, (1, 1, 0))
    assert n_haps.tolist() == [3, 4, 0, 0, 0] and total.tolist() == [4, 4, 0, 0, 0] and hist.tolist() == [[0, 0, 0, 1, 1, 0, 0, 0], [0] * 8]
    assert rec.tolist() == [(0, 0, 2, 4), (0, 1, 1, 4), (0, 6, 1, 4), (1, 0, 1, 4), (1, 1, 1, 4), (1, 2, 1, 4), (1, 4, 1, 4)]
    n_haps, total, hist, rec = haploref.call(h3, sites, (1, 2, 500))
    assert n_haps.tolist() == [1, 0, 0, 0, 0] and hist[0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and rec.tolist() == [(0, 0, 2, 4)]
    assert not haploref.call(h3, sites, (5, 1, 0))[2].any()
