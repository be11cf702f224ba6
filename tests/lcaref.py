"""The lca contract (include/monica_amd.h, "lca") in plain Python: the reference of test_lca_host.py and test_gpu_lca.py.
Written from the header, not from csrc/k_lca.hip: the LCA by ancestor sets, the clade counts by a walk to the root per node."""
import numpy as np

import abundref


def line(parent, v):
    """v and its ancestors, v first."""
    out = []
    while v != -1:
        out.append(int(v))
        v = parent[v]
    return out


def lca(parent, nodes):
    """The deepest node that is an ancestor of (or is) every one of `nodes`; -1 for none."""
    nodes = list(nodes)
    if not nodes:
        return -1
    common = set(line(parent, nodes[0]))
    for v in nodes[1:]:
        common &= set(line(parent, v))
    return next(v for v in line(parent, nodes[0]) if v in common)


def place(per_read_regs, contig_genome, parent, max_delta=abundref.MAX_DELTA):
    """int32[n_reads]: every read's node -- the LCA of abundref's candidates."""
    return np.array([lca(parent, [g for g, _ in abundref.candidates(regs, contig_genome, max_delta)]) for regs in per_read_regs], dtype=np.int32)


def direct(parent, node):
    return np.bincount(np.asarray(node)[np.asarray(node) >= 0], minlength=len(parent)).astype(np.int64)


def clade(parent, direct_counts):
    out = np.zeros(len(parent), dtype=np.int64)
    for v, c in enumerate(direct_counts):
        for a in line(parent, v):
            out[a] += int(c)
    return out
