"""Reads placed on a taxonomy by lowest common ancestor, on the device (mnc_lca_*, mnc_engine_add_lca; csrc/k_lca.hip).

Reference: tests/lcaref.py -- the contract in plain Python -- applied to the CPU ORACLE's regions through abundref's
candidates (and, for the carry, to carryref's rows).  Nothing is compared against the engine's own dumps.  Every comparison
is exact integer equality."""
import numpy as np
import pytest

import carryref
import lcaref
import util
from monica_amd import synth
from test_gpu_abundance import MIN_MAPQ, corpus, world          # noqa: F401 -- the four genomes and ~150 reads of the abundance tests
from test_gpu_carry import reference, split                    # noqa: F401 -- ... and the same world as two index parts

pytestmark = pytest.mark.gpu

# genomes A 0, B 1, C 2, D 3 (D 0.3 % from A, C 1 % from A's first 50 kb, B unrelated)
TREE = [4, 7, 5, 4, 6, 6, 8, 8, -1]              # 4 = the species of A and D, 5 = C's species, 6 = their genus, 7 = B's genus, 8 = the root
# A at the bottom of 64 levels (62 inner nodes 4 .. 65 up to the root 66), D beside it; B and C under node 67, which the DFS
# meets after A's line: the climb from A to the root is the longest there is, 63 steps
CHAIN = [4, 67, 67, 4] + list(range(5, 67)) + [-1, 66]
NESTED = [3, 7, 5, 4, 6, 6, 8, 8, -1]            # genome D is the parent of genome A
TREES = dict(tree=TREE, chain=CHAIN, nested=NESTED)


def padded(parent, n_nodes):
    """The same tree with unused inner nodes under the root, up to n_nodes."""
    return list(parent) + [parent.index(-1)] * (n_nodes - len(parent))


def classify(world, corpus, a=0, b=None):
    off = corpus["offsets"]
    b = len(corpus["reads"]) if b is None else b
    world.eng.classify(corpus["bases"][off[a]:off[b]], off[a:b + 1] - off[a], MIN_MAPQ)


@pytest.fixture(scope="module")
def want(world, corpus):
    """The reference's nodes per (tree, max_delta), computed once on the CPU and checked to hold every level."""
    out = {(name, md): lcaref.place(corpus["regs"], world.cg, parent, md) for name, parent in TREES.items() for md in (0, 80)}
    w = out["tree", 80]
    assert (w == -1).sum() >= 1 and (w == 4).sum() >= 5 and (w == 6).sum() >= 5 and ((w >= 0) & (w < 4)).sum() >= 20, np.bincount(w + 1)
    assert (out["chain", 80] == 66).sum() >= 5 and (out["nested", 80] == 3).sum() >= 5
    assert (out["tree", 0] != w).any()
    return out


def check(lca, parent, nodes, n_truncated=0, scale=1):
    direct, clade = lca.counts()
    w_direct = lcaref.direct(parent, nodes) * scale
    assert direct.dtype == clade.dtype == np.int64 and np.array_equal(direct, w_direct) and np.array_equal(clade, lcaref.clade(parent, w_direct))
    assert lca.info() == dict(n_placed=int((nodes >= 0).sum()) * scale, n_unplaced=int((nodes < 0).sum()) * scale, n_truncated=n_truncated)


# 1. parity below and above the LDS cut-off (4 097 = MNC_LCA_LDS_NODES + 1), a line of 64 levels, a genome under a genome
@pytest.mark.parametrize("name,n_nodes,max_delta", [("tree", 9, 0), ("tree", 9, 80), ("tree", 4097, 0), ("tree", 4097, 80),
                                                    ("chain", 68, 80), ("nested", 9, 80)])
def test_nodes_and_counts_equal_the_reference(capi, world, corpus, want, name, n_nodes, max_delta):
    assert capi.LCA_LDS_NODES + 1 == 4097
    parent = padded(TREES[name], n_nodes)
    lca = capi.Lca(world.idx, parent, max_delta=max_delta, cap_reads=len(corpus["reads"]))
    classify(world, corpus)
    world.eng.add_lca(lca)
    nodes = lca.nodes()
    assert nodes.dtype == np.int32 and np.array_equal(nodes, want[name, max_delta])
    check(lca, parent, nodes)
    check(lca, parent, nodes)                                     # reading does not change it
    assert all(lca.device()) and lca.device_bytes() >= 44 * n_nodes
    lca.close()


# 2. shape
def test_direct_is_additive_and_nodes_are_the_latest_adds(capi, world, corpus, want):
    n, w = len(corpus["reads"]), want["tree", 80]
    cuts = [0, n // 3, 2 * n // 3, n]
    lca = capi.Lca(world.idx, TREE, cap_reads=n)
    for a, b in zip(cuts, cuts[1:]):
        classify(world, corpus, a, b)
        world.eng.add_lca(lca)
    assert np.array_equal(lca.nodes(), w[cuts[2]:])
    check(lca, TREE, w)                                           # three batches = one batch (test 1)
    world.eng.add_lca(lca)                                        # the last batch once more
    assert np.array_equal(lca.nodes(), w[cuts[2]:])
    assert np.array_equal(lca.counts()[0], lcaref.direct(TREE, w) + lcaref.direct(TREE, w[cuts[2]:]))
    lca.reset()
    check(lca, TREE, w[:0])
    assert (lca.nodes(0, n) == -1).all()
    classify(world, corpus)
    world.eng.add_lca(lca), world.eng.add_lca(lca)                # the batch added twice
    check(lca, TREE, w, scale=2)
    lca.close()


def test_a_batch_beyond_cap_reads_is_refused(capi, world, corpus, want):
    n = len(corpus["reads"])
    lca = capi.Lca(world.idx, TREE, cap_reads=n - 1)
    classify(world, corpus, 0, n - 1)
    world.eng.add_lca(lca)
    before = (lca.counts(), lca.info(), lca.nodes())
    classify(world, corpus)
    assert capi.lib().mnc_engine_add_lca(world.eng._h, lca._h) == capi.ERR_RANGE
    after = (lca.counts(), lca.info(), lca.nodes())
    assert all(np.array_equal(x, y) for x, y in zip(before[0] + (before[2],), after[0] + (after[2],))) and before[1] == after[1]
    assert np.array_equal(after[2], want["tree", 80][:n - 1])
    lca.close()


# 3. a known answer, without the oracle
def test_reads_of_a_shared_piece_land_on_the_parent(capi):
    g = synth.genome(0x1CA, 40_000)
    piece = g[10_000:13_000].copy()
    idx = capi.Index.from_seqs(["Xus_a:1", "Xus_a:2"], [g, piece])
    assert len(idx.genome_names) == 2
    shared = [piece[0:1000], piece[500:1700], util.revcomp(piece[1500:2900]), piece[100:2900]]
    alone = [g[2_000:3_500], util.revcomp(g[20_000:21_200]), g[30_000:32_000]]
    eng, lca = capi.Engine(idx, 0), capi.Lca(idx, [2, 2, -1], cap_reads=16)
    eng.classify(*util.pack_reads(shared + alone), MIN_MAPQ)
    eng.add_lca(lca)
    assert lca.nodes().tolist() == [2] * len(shared) + [0] * len(alone)
    direct, clade = lca.counts()
    assert direct.tolist() == [3, 0, 4] and clade.tolist() == [3, 0, 7] and lca.info()["n_placed"] == 7
    lca.close(), eng.close()


# 4. the carry, into a global accumulator
@pytest.mark.parametrize("width", [16, 2])
def test_rows_of_a_carry_over_two_parts(capi, split, width):
    n = split["n"]
    carry = capi.Carry(0, n, width=width)
    for part in split["parts"]:
        part.eng.classify(split["bases"], split["offsets"], MIN_MAPQ)
        part.eng.carry_candidates(carry, 0, part.genome_offset)
    rows = reference(split["pairs"], width, 80)
    nodes = np.array([lcaref.lca(TREE, [g for g, _ in carryref.candidates(r)]) for r in rows], dtype=np.int32)
    assert (nodes == -1).sum() >= 1 and (nodes == 6).sum() >= 5 and (width == 16 or carryref.info(rows)[2] >= 5)
    lca = capi.Lca(None, TREE, n_genomes=4, cap_reads=n)
    assert capi.lib().mnc_engine_add_lca(split["parts"][0].eng._h, lca._h) == capi.ERR_ARG      # it is for no index
    assert capi.lib().mnc_lca_add_carry(lca._h, carry._h, 1, n) == capi.ERR_RANGE
    check(lca, TREE, nodes[:0])
    lca.add_carry(carry, 0, 50), lca.add_carry(carry, 50, n - 50)                                # rows in two pieces
    assert np.array_equal(lca.nodes(), nodes)
    check(lca, TREE, nodes, n_truncated=carryref.info(rows)[2])
    other = capi.Lca(None, TREE, n_genomes=4, max_delta=70, cap_reads=n)
    small = capi.Lca(None, [2, 2, -1], n_genomes=2, cap_reads=n)                                 # the carry holds genome 3
    for acc in (other, small):
        assert capi.lib().mnc_lca_add_carry(acc._h, carry._h, 0, n) == capi.ERR_ARG and acc.info()["n_placed"] == 0
    for x in (lca, other, small, carry):
        x.close()
