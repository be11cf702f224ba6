"""Linkage (include/monica_amd.h, "linkage"): what needs no GPU -- the binding against the header and the argument errors of
mnc_linkage_create, which are all answered before a device is looked at."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import test_pileup_host as host

SEQ = np.frombuffer(b"ACGTTGCAAGGCTTAACCGGTATGCATGCAAT" * 40, dtype=np.uint8)          # 1 280 bases


def create(capi, rows, window, device):
    idx = capi.Index.from_seqs(["a:1", "b:1"], [SEQ, SEQ[::-1].copy()])
    s, h = np.array([(rid, pos, 0, 0, b"A", alt, 0) for rid, pos, alt in rows], dtype=capi.VARIANT_DTYPE), C.c_void_p()
    return capi.lib().mnc_linkage_create(idx._h, device, s.ctypes.data, len(s), window, C.byref(h)), h.value


def test_binding_matches_the_header(capi):
    text = open(host.HEADER).read()
    for sym in ["mnc_linkage_" + n for n in ("create", "free", "reset", "device_bytes", "fetch_sites", "fetch_pairs", "phase", "device")] + ["mnc_engine_add_linkage"]:
        assert re.search(r"\b%s\(" % sym, text) and sym in capi.EXPORTS and hasattr(capi.lib(), sym), sym
    assert int(re.search(r"#define\s+MNC_LINKAGE_MAX_WINDOW\s+(\d+)", text).group(1)) == capi.LINKAGE_MAX_WINDOW == 64
    assert all(callable(getattr(capi.Linkage, name)) for name in ("reset", "device_bytes", "site_counts", "pairs", "phase")) and callable(capi.Engine.add_linkage)
    limits = text[text.index("limits, and what happens at each"):text.index("---- classify")]
    assert "mnc_engine_add_linkage: MNC_ERR_UNSUPPORTED" in limits and "mnc_linkage_create: MNC_ERR_ARG" in limits
    from monica_amd import mappy_compat
    p = inspect.signature(mappy_compat.Aligner.map_batch).parameters
    assert p["linkage"].default is None and "linkage_what" in p and callable(mappy_compat.Aligner.linkage)


@pytest.mark.parametrize("rows,window,word", (
    (((0, 9, b"C"), (0, 5, b"C")), 16, b"site 1 does not ascend"),                 # positions
    (((1, 5, b"C"), (0, 9, b"C")), 16, b"site 1 does not ascend"),                 # contigs
    (((0, 5, b"C"), (0, 5, b"C")), 16, b"site 1 does not ascend"),                 # the same site twice
    (((0, 5, b"-"), (0, 5, b"T")), 16, b"site 1 does not ascend"),                 # alleles out of order
    (((0, 5, b"C"), (0, 7, b"+")), 16, b"site 1 is an insertion allele"),
    (((0, 5, b"N"),), 16, b"site 0"),
    (((0, 5, b"C"), (1, 1280, b"C")), 16, b"site 1"),                              # one past the contig's last base
    (((0, 5, b"C"),), 0, b"window 0"),
    (((0, 5, b"C"),), 65, b"window 65"),
))
def test_create_argument_errors(capi, rows, window, word):
    rc, h = create(capi, rows, window, capi.device_count())      # a device that does not exist: the answer comes before it
    assert rc == capi.ERR_ARG and not h and word in capi.lib().mnc_last_error(), capi.lib().mnc_last_error()


def test_null_pointers_and_a_good_list_without_a_device(capi):
    L, n_dev, h, n = capi.lib(), capi.device_count(), C.c_void_p(), C.c_int64(7)
    good = ((0, 5, b"C"), (0, 5, b"-"), (0, 1279, b"A"), (1, 0, b"T"))
    assert create(capi, good, 64, n_dev) == (capi.ERR_NODEVICE, None)
    idx = capi.Index.from_seqs(["a:1"], [SEQ])
    s = np.zeros(1, dtype=capi.VARIANT_DTYPE)
    assert L.mnc_linkage_create(None, n_dev, s.ctypes.data, 1, 16, C.byref(h)) == capi.ERR_ARG
    assert L.mnc_linkage_create(idx._h, n_dev, s.ctypes.data, 1, 16, None) == capi.ERR_ARG
    assert L.mnc_linkage_create(idx._h, n_dev, None, 1, 16, C.byref(h)) == capi.ERR_ARG
    assert L.mnc_linkage_create(idx._h, n_dev, s.ctypes.data, -1, 16, C.byref(h)) == capi.ERR_ARG
    assert L.mnc_linkage_reset(None) == capi.ERR_ARG and L.mnc_linkage_device_bytes(None, C.byref(n)) == capi.ERR_ARG
    assert L.mnc_linkage_fetch_sites(None, 0, 0, None) == capi.ERR_ARG and L.mnc_linkage_fetch_pairs(None, 0, 0, None) == capi.ERR_ARG
    assert L.mnc_linkage_phase(None, 1, 0, None, None) == capi.ERR_ARG and L.mnc_linkage_device(None, None, None) == capi.ERR_ARG
    assert L.mnc_engine_add_linkage(None, None, capi.COV_GATED) == capi.ERR_ARG and n.value == 7
    L.mnc_linkage_free(None)                                       # a no-op
