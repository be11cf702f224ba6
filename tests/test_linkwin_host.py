"""mnc_linkage_phase_window / mnc_linkage_add_tables: what needs no GPU -- tests/linkwinref.py against tests/linkref.py and
against the haplotag's rules, the binding against the header, the refusals answered before a device is looked at."""
import ctypes as C
import re

import numpy as np
import pytest

import linkref
import linkwinref
import test_pileup_host as host


def random_tables(seed, sizes=(40, 1, 2, 57), window=8, density=0.3):
    """(pair[n, window, 4], rid[n]): seeded counts 0 .. 11 in a share of the cells, none past a contig's last site."""
    rng = np.random.default_rng(seed)
    rid = np.repeat(np.arange(len(sizes)), sizes)
    pair = rng.integers(0, 12, (len(rid), window, 4)) * (rng.random((len(rid), window, 1)) < density)
    j = np.arange(len(rid))[:, None] + np.arange(window)[None, :] + 1
    inside = (j < len(rid)) & (rid[np.minimum(j, len(rid) - 1)] == rid[:, None])
    return (pair * inside[:, :, None]).astype(np.int32), rid


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("thresholds", ((1, 0), (4, 600)))
def test_reach_one_is_the_adjacent_phase(seed, thresholds):
    pair, rid = random_tables(seed)
    sites = np.zeros(len(rid), dtype=[("rid", np.int32)])
    sites["rid"] = rid
    keep, block, phase = linkwinref.phase_window(pair, rid, 1, *thresholds)
    want_block, want_phase = linkref.phase(pair, sites, *thresholds)
    assert keep.all() and np.array_equal(block, want_block) and np.array_equal(phase, want_phase) and phase.any() and np.bincount(block).max() > 1


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("reach,density", ((8, 0.3), (8, 0.04), (3, 0.1)))
def test_kept_sites_are_what_the_haplotag_takes(seed, reach, density):
    pair, rid = random_tables(seed, density=density)
    keep, block, phase = linkwinref.phase_window(pair, rid, reach, 2, 300)
    assert keep[np.r_[True, rid[1:] != rid[:-1]]].all() and (block[~keep] == -1).all() and not phase[~keep].any()
    assert linkwinref.haplotag_accepts(rid[keep], block[keep], phase[keep])
    if density < 0.3:
        assert not keep.all(), "no dropped site: the inputs are wrong"


def test_binding_and_refusals_without_a_device(capi):
    L, text = capi.lib(), open(host.HEADER).read()
    for sym in ("mnc_linkage_phase_window", "mnc_linkage_add_tables"):
        assert re.search(r"\b%s\(" % sym, text) and sym in capi.EXPORTS and hasattr(L, sym), sym
    assert callable(capi.Linkage.phase_window) and callable(capi.Linkage.add_tables)
    n, out = C.c_int64(7), np.zeros(4, dtype=np.int32)
    assert L.mnc_linkage_phase_window(None, 1, 1, 0, out.ctypes.data, out.ctypes.data, C.byref(n)) == capi.ERR_ARG and n.value == 7
    assert L.mnc_linkage_add_tables(None, out.ctypes.data, out.ctypes.data) == capi.ERR_ARG
