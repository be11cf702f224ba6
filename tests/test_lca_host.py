"""Lca (include/monica_amd.h, "lca"): what needs no GPU -- the symbols, the argument errors of mnc_lca_create, which are all
answered before a device is looked at, the taxonomy made from genome names, and tests/lcaref.py on a tree worked out by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lcaref

CHAIN = lambda n: list(range(1, n)) + [-1]                                   # node 0 at the bottom of n levels


def create(capi, parent, n_genomes, max_delta=80, cap_reads=16, idx=None):
    p, h = np.asarray(parent, dtype=np.int32), C.c_void_p()
    rc = capi.lib().mnc_lca_create(idx._h if idx else None, capi.device_count(), n_genomes, p.ctypes.data, len(p), max_delta, cap_reads, C.byref(h))
    return rc, h.value                                                       # (a device that does not exist)


def test_the_symbols_exist(capi):
    for sym in ["mnc_lca_" + n for n in ("create", "free", "reset", "device_bytes", "info", "add_carry", "fetch", "fetch_nodes", "device")] + ["mnc_engine_add_lca"]:
        assert sym in capi.EXPORTS and hasattr(capi.lib(), sym), sym
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "monica_amd.h")).read()
    for name, value in (("MNC_LCA_MAX_DEPTH", capi.LCA_MAX_DEPTH), ("MNC_LCA_LDS_NODES", capi.LCA_LDS_NODES)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    assert callable(capi.Lca.counts) and callable(capi.Engine.add_lca)
    from monica_amd import mappy_compat
    assert callable(mappy_compat.Aligner.lca) and "lca" in mappy_compat.Aligner.map_batch.__code__.co_varnames


@pytest.mark.parametrize("parent,n_genomes,word,kw", (
    ([2, 2, -1], 4, b"n_nodes 3 below n_genomes 4", {}),
    ([2, 3, -1], 2, b"node 1: parent 3 outside -1 .. 2", {}),
    ([2, -2, -1], 2, b"node 1: parent -2 outside -1 .. 2", {}),
    ([9] * 7 + [8, 7, -1], 4, b"node 7 is its own ancestor", {}),
    ([1, 1, -1], 1, b"node 1 is its own ancestor", {}),
    ([1, 0], 1, b"no node is the root", {}),
    ([9, 9, 9, -1, 3, 3, 3, 3, 3, -1], 3, b"nodes 3 and 9 are both roots", {}),
    (CHAIN(65), 1, b"node 0 lies 65 levels deep", {}),
    ([2, 2, -1], 2, b"max_delta -1", dict(max_delta=-1)),
    ([2, 2, -1], 2, b"cap_reads 0", dict(cap_reads=0)),
))
def test_create_argument_errors(capi, parent, n_genomes, word, kw):
    rc, h = create(capi, parent, n_genomes, **kw)
    assert rc == capi.ERR_ARG and not h and word in capi.lib().mnc_last_error(), capi.lib().mnc_last_error()


def test_a_valid_tree_gets_as_far_as_the_device(capi):
    assert create(capi, CHAIN(64), 1) == (capi.ERR_NODEVICE, None)            # 64 levels are held
    assert create(capi, [4, 4, 5, 6, 5, 6, -1], 4) == (capi.ERR_NODEVICE, None)
    idx = capi.Index.from_seqs(["a:1", "b:1"], [np.frombuffer(b"ACGTTGCA" * 20, dtype=np.uint8)] * 2)
    assert create(capi, [2, 2, -1], 2, idx=idx) == (capi.ERR_NODEVICE, None)
    rc, h = create(capi, [3, 3, 3, -1], 3, idx=idx)                           # the index holds two genomes
    assert rc == capi.ERR_ARG and not h and b"the index holds 2 genomes" in capi.lib().mnc_last_error()
    assert capi.lib().mnc_engine_add_lca(None, None) == capi.ERR_ARG


def test_taxonomy_from_names(capi):
    names = ["Escherichia_coli:A1", "Escherichia_coli:A2", "Escherichia_fergusonii:B1", "Bacillus_subtilis:C1", "Phage:D1"]
    parent, node_names = capi.taxonomy_from_names(names)
    assert parent.dtype == np.int32 and parent.tolist() == [5, 5, 8, 9, 11, 6, 7, -1, 6, 10, 7, 12, 7]
    assert node_names == names + ["Escherichia_coli", "Escherichia", "root", "Escherichia_fergusonii", "Bacillus_subtilis", "Bacillus", "Phage", "Phage"]
    assert lcaref.lca(parent, [0, 1]) == 5 and lcaref.lca(parent, [1, 2]) == 6 and lcaref.lca(parent, [2, 3]) == 7 and lcaref.lca(parent, [4]) == 4
    assert create(capi, parent, 5) == (capi.ERR_NODEVICE, None)


def test_reference_on_seven_nodes_by_hand():
    """Genomes 0 .. 3; node 4 = the species of 0 and 1; node 5 = the genus of 4 and 2; node 6 = the root, over 5 and 3."""
    parent = [4, 4, 5, 6, 5, 6, -1]
    for nodes, want in (([0], 0), ([0, 1], 4), ([1, 0, 1], 4), ([0, 2], 5), ([1, 3], 6), ([0, 4], 4), ([5, 1], 5), ([], -1)):
        assert lcaref.lca(parent, nodes) == want, nodes
    assert lcaref.clade(parent, [3, 1, 2, 1, 5, 0, 1]).tolist() == [3, 1, 2, 1, 9, 11, 13]
    regs = lambda *rows: np.array(list(rows), dtype=[("rid", "<i4"), ("dp_max", "<i4"), ("n_cigar", "<i4")])
    per_read = [regs((0, 100, 3), (1, 30, 1)),                                 # genomes 0 and 1, 70 apart
                regs((4, 50, 1), (2, 60, 0), (3, 45, 2)),                      # contig 4 is genome 0's; the record without a CIGAR does not count
                regs()]
    cg = [0, 1, 2, 3, 0]
    assert lcaref.place(per_read, cg, parent, 80).tolist() == [4, 6, -1]
    assert lcaref.place(per_read, cg, parent, 69).tolist() == [0, 6, -1]
    assert lcaref.place(per_read, cg, parent, 4).tolist() == [0, 0, -1]
    assert lcaref.direct(parent, [4, 6, -1, 4]).tolist() == [0, 0, 0, 0, 2, 0, 1]
