"""Demux (include/monica_amd.h, "demux"): what needs no GPU -- the symbols, the argument errors of mnc_demux_create, which
are all answered before a device is looked at, and tests/demuxref.py on cases worked by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import demuxref
from demuxref import BOTH, EITHER, FRONT

BC = "ACGTTGCAAC"                                                            # 10 bases, no period
RC = "GTTGCAACGT"                                                            # its reverse complement


def create(capi, barcodes, window=150, max_dist=6, min_margin=2, ends=EITHER, cap_reads=16, n=None):
    pats = [np.frombuffer(b.encode(), dtype=np.uint8) for b in barcodes]
    off = np.zeros(len(pats) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in pats])
    bases, h = np.concatenate(pats + [np.zeros(1, dtype=np.uint8)]), C.c_void_p()
    rc = capi.lib().mnc_demux_create(None, capi.device_count(), bases.ctypes.data, off.ctypes.data, len(pats) if n is None else n,
                                     window, max_dist, min_margin, ends, cap_reads, C.byref(h))
    return rc, h.value                                                       # (a device that does not exist)


def test_the_symbols_exist(capi):
    for sym in ["mnc_demux_" + n for n in ("create", "free", "reset", "device_bytes", "info", "set_word_bits", "add", "fetch_tags", "fetch_counts",
                                           "device")] + ["mnc_engine_add_demux"]:
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym), sym
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "monica_amd.h")).read()
    for name, value in (("MNC_DEMUX_MAX_BARCODES", capi.DEMUX_MAX_BARCODES), ("MNC_DEMUX_MAX_LEN", capi.DEMUX_MAX_LEN),
                        ("MNC_DEMUX_MAX_WINDOW", capi.DEMUX_MAX_WINDOW), ("MNC_DEMUX_FRONT", FRONT), ("MNC_DEMUX_BOTH", BOTH), ("MNC_DEMUX_EITHER", EITHER)):
        assert int(re.search(rf"#define {name} +(\d+)", header).group(1)) == value
    assert capi.DEMUX_TAG_DTYPE == demuxref.TAG_DTYPE and capi.DEMUX_TAG_DTYPE.itemsize == 8
    assert callable(capi.Demux.tags) and callable(capi.Engine.add_demux)
    from monica_amd import mappy_compat
    assert callable(mappy_compat.Aligner.demux) and mappy_compat.Aligner.map_batch.__code__.co_varnames[:mappy_compat.Aligner.map_batch.__code__.co_argcount][-1] == "demux"


@pytest.mark.parametrize("barcodes,word,kw", (
    (["ACGT", "ACNT"], b"barcode 1, position 2: character 0x4e", {}),
    (["ACGT", "", "AC"], b"barcode 1: length 0 outside 1 .. 64", {}),
    (["A" * 65], b"barcode 0: length 65 outside 1 .. 64", {}),
    ([BC], b"window 0 outside 1 .. 1024", dict(window=0)),
    ([BC], b"window 1025 outside 1 .. 1024", dict(window=1025)),
    ([BC], b"n_barcodes 0 outside 1 .. 256", dict(n=0)),
    (["ACGT"] * 257, b"n_barcodes 257 outside 1 .. 256", {}),
    ([BC], b"max_dist -1", dict(max_dist=-1)),
    ([BC], b"min_margin -1", dict(min_margin=-1)),
    ([BC], b"ends 3", dict(ends=3)),
    ([BC], b"cap_reads 0", dict(cap_reads=0)),
))
def test_create_argument_errors(capi, barcodes, word, kw):
    rc, h = create(capi, barcodes, **kw)
    assert rc == capi.ERR_ARG and not h and word in capi.lib().mnc_last_error(), capi.lib().mnc_last_error()


def test_a_valid_call_gets_as_far_as_the_device(capi):
    assert create(capi, ["acgu", "A" * 64, "T"] + ["ACGT"] * 253, window=1024, max_dist=0, min_margin=0, ends=FRONT) == (capi.ERR_NODEVICE, None)
    assert capi.lib().mnc_engine_add_demux(None, None) == capi.ERR_ARG and capi.lib().mnc_demux_add(None, None, None, 0, 0) == capi.ERR_ARG


@pytest.mark.parametrize("text,want", (
    (BC + "GGGG", (0, 9)),                                                   # exact at index 0: e = |p| - 1
    ("GG" + "ACGTAGCAAC" + "GG", (1, 11)),                                   # one substitution
    ("GG" + "ACGTTAGCAAC" + "GG", (1, 12)),                                  # one base inserted into the read
    ("GG" + "ACGTGCAAC" + "GG", (1, 10)),                                    # one base deleted from it
    ("ACGTT", (5, 4)),                                                       # the pattern is longer than the text: its head, five deleted
    ("GGGG" + BC[:7], (3, 10)),                                              # cut by the window's end
    ("GG" + "ACGTNGCAAC", (1, 11)),                                          # an N costs one, as any mismatch
    ("ggacguugcaac", (0, 11)),                                               # lower case, U
    ("", (10, -1)),
))
def test_reference_search_by_hand(text, want):
    p, t = demuxref.codes(BC), demuxref.codes(text)
    assert demuxref.search(p, t) == want
    d, e = demuxref.search_all([p, p[:3]], [t, t[:5]])                       # the batched form is the same table
    assert (int(d[0, 0]), int(e[0, 0])) == want and (int(d[1, 1]), int(e[1, 1])) == demuxref.search(p[:3], t[:5])


def test_reference_tags_by_hand():
    other = "TTGGCCAATT"                                                     # 6 or more from BC anywhere below
    assert "".join("ACGTN"[c] for c in demuxref.texts(b"AAC" + b"G" * 20 + RC.encode() + b"TT", 14)[1]) == "AA" + BC + "CC"     # the rear text
    tag = lambda reads, bcs=(BC, other), window=14, max_dist=2, min_margin=2, ends=EITHER: \
        [tuple(int(v) for v in t) for t in demuxref.tags(list(bcs), reads, window, max_dist, min_margin, ends)]
    mid = b"G" * 20
    both = b"AA" + BC.encode() + mid + RC.encode() + b"TT"                   # barcode 0 at both ends
    split = b"AA" + BC.encode() + mid + b"AATTGGCCAA" + b"TT"                # barcode 0 in front, barcode 1 (reverse complement) behind
    rear = b"GGGGGGGGGGGGGG" + mid + RC.encode() + b"TT"
    assert tag([both]) == [(0, 0, 0, 12, 12)]
    assert tag([split], ends=FRONT) == [(0, 0, 255, 12, 0)] and tag([split], ends=BOTH) == [(-1, 0, 0, 0, 0)] and tag([split]) == [(-2, 0, 0, 0, 0)]
    assert tag([rear]) == [(0, 8, 0, 0, 12)] and tag([rear], ends=BOTH) == [(-1, 8, 0, 0, 0)]
    # a tie between two barcodes: the lower index is the best, and only min_margin 0 lets it hit
    assert tag([b"AA" + BC.encode()], bcs=(BC, BC), ends=FRONT) == [(-1, 0, 255, 0, 0)]
    assert tag([b"AA" + BC.encode()], bcs=(BC, BC), ends=FRONT, min_margin=0) == [(0, 0, 255, 12, 0)]
    assert tag([b"AA" + BC.encode()], bcs=(BC,), ends=FRONT) == [(0, 0, 255, 12, 0)]             # one barcode passes the margin
    assert tag([b""], bcs=(BC,), max_dist=10) == [(0, 10, 10, 0, 0)] and tag([b""], bcs=(BC,)) == [(-1, 10, 10, 0, 0)]
    assert demuxref.read_counts(demuxref.tags([BC, other], [both, split, rear, mid], 14, 2, 2, EITHER), 2).tolist() == [2, 0, 1, 1]
