"""Haplotag (include/monica_amd.h, "haplotag"): what needs no GPU -- the argument errors of mnc_haplotag_create, which are
all answered before a device is looked at."""
import ctypes as C

import numpy as np
import pytest

from test_linkage_host import SEQ

GOOD = ((0, 5, b"C"), (0, 9, b"C"), (0, 30, b"-"), (1, 2, b"T"), (1, 8, b"G"))      # (rid, pos, allele)


def create(capi, rows, block, phase, cap_reads=100, min_votes=2, min_permille=600):
    idx = capi.Index.from_seqs(["a:1", "b:1"], [SEQ, SEQ[::-1].copy()])
    s, h = np.array([(rid, pos, 0, 0, b"A", alt, 0) for rid, pos, alt in rows], dtype=capi.VARIANT_DTYPE), C.c_void_p()
    b, p = np.array(block, dtype=np.int32), np.array(phase, dtype=np.uint8)
    rc = capi.lib().mnc_haplotag_create(idx._h, capi.device_count(), s.ctypes.data, len(s), b.ctypes.data, p.ctypes.data,   # a device that does not exist
                                        cap_reads, min_votes, min_permille, C.byref(h))
    return rc, h.value


@pytest.mark.parametrize("word,kw", (
    (b"site 0: block 1", dict(block=(1, 1, 1, 2, 2))),
    (b"site 2: block 2 after block 0", dict(block=(0, 0, 2, 3, 3))),
    (b"site 2: block 0 after block 1", dict(block=(0, 1, 0), rows=GOOD[:3])),
    (b"site 3: the first site of contig 1 continues block 1", dict(block=(0, 1, 1, 1, 2))),
    (b"site 4: phase 2", dict(phase=(0, 1, 0, 0, 2))),
    (b"site 2: phase 1 at the first site of block 1", dict(phase=(0, 1, 1, 0, 0))),
    (b"site 0: phase 1 at the first site of block 0", dict(phase=(1, 0, 0, 0, 0))),
    (b"min_votes 0", dict(min_votes=0)),
    (b"min_permille -1", dict(min_permille=-1)),
    (b"min_permille 1001", dict(min_permille=1001)),
    (b"cap_reads 0", dict(cap_reads=0)),
    (b"site 1 is an insertion allele", dict(rows=((0, 5, b"C"), (0, 7, b"+")))),
    (b"site 1 does not ascend", dict(rows=((0, 9, b"C"), (0, 5, b"C")))),
))
def test_create_argument_errors(capi, word, kw):
    rows = kw.pop("rows", GOOD)
    args = dict(block=(0, 0, 1, 2, 2)[:len(rows)], phase=((0, 1, 0, 0, 0) if "block" not in kw else (0,) * 5)[:len(rows)])
    args.update((k, v[:len(rows)] if k in ("block", "phase") else v) for k, v in kw.items())
    rc, h = create(capi, rows, **args)
    assert rc == capi.ERR_ARG and not h and word in capi.lib().mnc_last_error(), capi.lib().mnc_last_error()


def test_good_arguments_without_a_device(capi):
    assert create(capi, GOOD, (0, 0, 1, 2, 2), (0, 1, 0, 0, 1)) == (capi.ERR_NODEVICE, None)
    assert create(capi, (), (), ()) == (capi.ERR_NODEVICE, None)
    assert capi.lib().mnc_engine_add_haplotag(None, None, capi.COV_GATED) == capi.ERR_ARG
