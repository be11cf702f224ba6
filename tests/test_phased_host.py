"""Phased pileup (include/monica_amd.h, "phased pileup"): what needs no GPU -- tests/phaseref.py, the reference of
test_gpu_phased.py, on two hand-made records whose answers are written out here."""
import numpy as np

import covref
import phaseref
import pileref

# Thirty A's.  Block 0 = sites 0, 1 (extent 2 .. 5), block 1 = sites 2, 3 (5 .. 8; position 5 is block 0's), block 2 = sites
# 4, 5 (12 .. 15); 9 .. 11 lie between two extents.  One vote decides.
SEQS = [np.frombuffer(b"A" * 30, dtype=np.uint8)]
SITES = np.array([(0, p, 0, 0, b"A", a, 0) for p, a in ((2, b"C"), (5, b"C"), (5, b"G"), (8, b"C"), (12, b"C"), (15, b"C"))], dtype=pileref.VARIANT_DTYPE)
BLOCK, PHASE = np.array([0, 0, 1, 1, 2, 2]), np.array([0, 1, 0, 0, 0, 0])
# record 0: 0 .. 19, two bases inserted behind 8 (block 1's last base); C at 2, 12, 15.  Block 0: ALT at phase 0 and REF at
# phase 1, haplotype 1; block 1: REF twice, haplotype 0; block 2: ALT twice, haplotype 1.
# record 1: 4 .. 13 with 7, 8, 9 deleted; C at 5.  Block 0: ALT at phase 1, haplotype 0; block 1: nothing said (C is not G,
# and 8 is deleted); block 2: REF at 12, haplotype 0.
READS = [b"AACAAAAAAGGAAACAACAAAA", b"ACAAAAA"]
PRIMARY = dict(rid=0, rev=0, qs=0, id=0, parent=0, mapq=60)
PER_READ = [([dict(PRIMARY, rs=0, re=20, qe=22)], [[(9, "M"), (2, "I"), (11, "M")]]), ([dict(PRIMARY, rs=4, re=14, qe=7)], [[(3, "M"), (3, "D"), (4, "M")]])]
WANT = {phaseref.HAP0: {"depth": (6, 7, 8, 4, 5, 12, 13), "A": (6, 7, 8, 4, 12, 13), "C": (5,), "INS": (8,)},
        phaseref.HAP1: {"depth": (2, 3, 4, 5, 12, 13, 14, 15), "A": (3, 4, 5, 13, 14), "C": (2, 12, 15)},
        phaseref.REST: {"depth": (0, 1, 9, 10, 11, 16, 17, 18, 19, 6, 10, 11), "A": (0, 1, 9, 10, 11, 16, 17, 18, 19, 6, 10, 11), "DEL": (7, 8, 9)}}


def test_hand_made_records():
    planes, notes = phaseref.tally(PER_READ, READS, covref.ALL, 0, SEQS, SITES, BLOCK, PHASE, 1, 0)
    assert notes["decided"] == [(0, {0: 1, 1: 0, 2: 1}), (0, {0: 0, 2: 0})]
    for dest, want in WANT.items():
        P = np.zeros((8, 30), dtype=np.int64)
        for plane, at in want.items():
            np.add.at(P[pileref.PLANES.index(plane)], list(at), 1)
        assert np.array_equal(planes[dest][0], P), (dest, np.argwhere(planes[dest][0] != P))
    plain = pileref.tally(pileref.records_of(PER_READ, READS, covref.ALL, 0), SEQS)
    assert np.array_equal(planes[0][0] + planes[1][0] + planes[2][0], plain[0])
    # record 0 passes from haplotype 1 to 0 at 6; record 1's deletion leaves block 1's extent at 9; the I sits on 8
    assert (notes["M changes haplotype"], notes["D over a border"], notes["I on a last base"]) == (1, 1, 1)
    assert [phaseref.block_of(SITES, BLOCK, 0, p) for p in (1, 2, 5, 6, 9, 11, 12, 16)] == [None, 0, 0, 1, None, None, 2, None]
    assert phaseref.block_of(SITES, BLOCK, 1, 5) is None
