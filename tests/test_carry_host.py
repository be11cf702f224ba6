"""What the candidate carry promises without a GPU: the library exports the new symbols, the binding matches the header, the
argument checks that need no device, the properties of the merge rule as tests/carryref.py states it, and what the aligner
loop refuses and no longer refuses."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import abundref
import carryref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "monica_amd.h")
CARRY_SYMBOLS = ("create", "free", "reset", "reserve", "device_bytes", "add_lists", "merge", "info", "fetch", "device")


def test_library_exports_every_new_symbol(capi):
    names = ["mnc_carry_" + n for n in CARRY_SYMBOLS] + ["mnc_engine_carry_candidates", "mnc_abundance_create_global", "mnc_abundance_add_carry"]
    for name in names:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name), name
    text = open(HEADER).read()
    section = text[text.index("------ candidate carry"):text.index("------ FASTQ batches")]
    assert text.index("------ abundance") < text.index("------ candidate carry")
    for name in names:
        assert re.search(r"\b" + name + r"\(", section), name
    for phrase in ("commutative, associative and idempotent", "ties going to the smaller genome id", "Only n_truncated_reads may depend on the order",
                   "8 * width + 8 bytes"):
        assert phrase in section, phrase
    limits = text[text.index("limits, and what happens at each"):text.index("---- classify")]
    assert "mnc_engine_carry_candidates: MNC_ERR_UNSUPPORTED" in limits and "n_truncated_reads" in limits


def test_python_signatures(capi):
    from monica_amd import aligner
    p = inspect.signature(capi.Carry.__init__).parameters
    assert list(p)[1:] == ["device", "cap_reads", "width", "max_delta"] and (p["width"].default, p["max_delta"].default) == (16, 80)
    for name in ("reset", "reserve", "info", "fetch", "add_lists", "merge", "device_bytes", "close"):
        assert callable(getattr(capi.Carry, name)), name
    assert list(inspect.signature(capi.Engine.carry_candidates).parameters)[1:] == ["carry", "first_read", "genome_offset"]
    assert list(inspect.signature(capi.Abundance.add_carry).parameters)[1:4] == ["carry", "first_read", "n_reads"]
    assert list(inspect.signature(capi.Abundance.global_).parameters)[:2] == ["device", "n_genomes"]
    # neither function's parameter list has changed
    assert list(inspect.signature(aligner.aligner_coverage).parameters) == [
        "sample", "sample_name", "index", "mode", "hits_folder", "mapping_quality", "overnight", "focus_species", "mapped_folder", "unmapped_folder",
        "ambiguous_folder", "focus_folder", "last_index", "abundance", "coverage", "pileup"]
    assert list(inspect.signature(aligner.multi_threaded_aligner).parameters)[-3:] == ["abundance", "coverage", "pileup"]
    assert "ONE index part" in aligner.ABUNDANCE_MULTI_PART


def test_argument_checks_without_a_device(capi):
    for kw in (dict(cap_reads=-1), dict(cap_reads=10, width=0), dict(cap_reads=10, width=65), dict(cap_reads=10, max_delta=-1)):
        with pytest.raises(ValueError):
            capi.Carry(0, **kw)
    with pytest.raises(ValueError):
        capi.Abundance.global_(0, -1)
    with pytest.raises(ValueError):
        capi.Abundance.global_(0, 3, max_delta=-1)
    L = capi.lib()
    h = C.c_void_p()
    n_dev = capi.device_count()                                    # a device that does not exist -- without a GPU that is device 0
    for args in ((-1, 16, 80), (10, 0, 80), (10, 65, 80), (10, -3, 80), (10, 16, -1)):
        assert L.mnc_carry_create(n_dev, *args, C.byref(h)) == capi.ERR_ARG and not h.value, args     # ERR_ARG before ERR_NODEVICE
    for width in (1, 16, 64):
        assert L.mnc_carry_create(n_dev, 10, width, 0, C.byref(h)) == capi.ERR_NODEVICE and not h.value
    assert L.mnc_carry_create(n_dev, 10, 16, 80, None) == capi.ERR_ARG
    with pytest.raises(capi.MncError) as err:
        capi.Carry(n_dev, 10)
    assert err.value.code == capi.ERR_NODEVICE
    for args in ((-1, 100, 80, 3), (4, -1, 80, 3), (4, 100, -1, 3), (4, 100, 80, 0), (4, 100, 1001, 4)):
        assert L.mnc_abundance_create_global(n_dev, *args, C.byref(h)) == capi.ERR_ARG and not h.value, args
    assert L.mnc_abundance_create_global(n_dev, 4, 100, 80, 3, C.byref(h)) == capi.ERR_NODEVICE and not h.value
    assert L.mnc_abundance_create_global(n_dev, 4, 100, 80, 3, None) == capi.ERR_ARG
    with pytest.raises(capi.MncError) as err:
        capi.Abundance.global_(n_dev, 4)
    assert err.value.code == capi.ERR_NODEVICE
    n = C.c_int64(7)
    assert L.mnc_carry_reset(None) == capi.ERR_ARG
    assert L.mnc_carry_reserve(None, 5) == capi.ERR_ARG
    assert L.mnc_carry_device_bytes(None, C.byref(n)) == capi.ERR_ARG
    assert L.mnc_carry_add_lists(None, 0, 0, None, None, None) == capi.ERR_ARG
    assert L.mnc_carry_merge(None, None) == capi.ERR_ARG
    assert L.mnc_carry_info(None, None, None, None, None) == capi.ERR_ARG
    assert L.mnc_carry_fetch(None, 0, 0, None, None, None, None) == capi.ERR_ARG
    assert L.mnc_carry_device(None, None, None, None, None) == capi.ERR_ARG
    assert L.mnc_engine_carry_candidates(None, None, 0, 0) == capi.ERR_ARG
    assert L.mnc_abundance_add_carry(None, None, 0, 0) == capi.ERR_ARG
    L.mnc_carry_free(None)


# ---------------------------------------------------------------- the rule's properties, on the reference
def random_parts(rng, n_parts, n_genomes, max_score, repeat):
    """One read's pairs part by part.  `repeat`: a genome id may come from several parts (as through add_lists or a part
    carried twice); otherwise every part has its own range of ids (as index parts have)."""
    parts = []
    for p in range(n_parts):
        k = int(rng.integers(0, 6))
        ids = rng.choice(n_genomes, size=min(k, n_genomes), replace=False) if repeat else p * n_genomes + rng.choice(n_genomes, size=min(k, n_genomes), replace=False)
        parts.append(sorted((int(g), int(rng.integers(0, max_score + 1))) for g in ids))
    return parts


def final(parts, width, max_delta):
    row = carryref.empty()
    for p in parts:
        carryref.merge(row, p, width, max_delta)
    return row


@pytest.mark.parametrize("width", [1, 2, 3, 64])
@pytest.mark.parametrize("max_delta", [0, 5, 80])
@pytest.mark.parametrize("repeat", [False, True])
def test_the_rows_do_not_depend_on_order_grouping_or_repetition(width, max_delta, repeat):
    rng = np.random.default_rng(1000 * width + 10 * max_delta + repeat)
    for _ in range(150):
        # scores close together, so the delta cut, ties and the width all bite
        parts = random_parts(rng, int(rng.integers(1, 6)), 8, int(rng.choice([3, 12, 200])), repeat)
        want = carryref.closed_form([pair for p in parts for pair in p], width, max_delta)
        row = final(parts, width, max_delta)
        assert row["pairs"] == want                                           # top-width-then-cut on the union
        assert (row["best"] is None) == (not want) and (not want or row["best"] == max(want.values()))
        assert len(want) <= width and all(row["best"] - s <= max_delta for s in want.values())
        for _ in range(3):                                                    # any permutation of the parts
            order = rng.permutation(len(parts))
            assert final([parts[i] for i in order], width, max_delta)["pairs"] == want
        # any regrouping: the parts' pairs delivered one by one, and as unions of neighbouring parts (per genome the largest)
        singles = [[pair] for p in parts for pair in p]
        assert final([singles[i] for i in rng.permutation(len(singles))], width, max_delta)["pairs"] == want
        cut = int(rng.integers(0, len(parts) + 1))
        groups = [sorted(carryref.closed_form([pair for p in g for pair in p], 1 << 30, 1 << 40).items()) for g in (parts[:cut], parts[cut:])]
        assert final(groups, width, max_delta)["pairs"] == want
        # carrying a part twice changes nothing
        assert final(parts + [parts[0]] + parts, width, max_delta)["pairs"] == want
        # two carries merged row for row
        a, b = final(parts[:cut], width, max_delta), final(parts[cut:], width, max_delta)
        assert carryref.merge_rows(a, b, width, max_delta)["pairs"] == want


def test_known_rows():
    row = carryref.merge(carryref.empty(), [(3, 100), (5, 100), (7, 99)], 2, 80)
    assert row == {"best": 100, "pairs": {3: 100, 5: 100}, "truncated": True}          # the tie goes to the smaller id
    assert carryref.fetched(row, 2) == (2, 100, [3, 5], [100, 100])
    carryref.merge(row, [(9, 181)], 2, 80)                                              # a higher best cuts both
    assert row["pairs"] == {9: 181} and row["best"] == 181 and carryref.candidates(row) == [(9, 0)]
    carryref.merge(row, [(9, 150), (1, 101)], 2, 80)                                    # a lower score for a genome there changes nothing
    assert row["pairs"] == {1: 101, 9: 181} and carryref.fetched(row, 4) == (2, 181, [1, 9, -1, -1], [101, 181, 0, 0])
    assert carryref.candidates(row) == [(1, 80), (9, 0)]
    # cut first, then room: (2, 10) and (0, 100), (1, 95) leave by the cut, nobody for room
    row = carryref.merge(carryref.empty(), [(0, 100), (1, 95)], 2, 80)
    carryref.merge(row, [(2, 10), (3, 200)], 2, 80)
    assert row == {"best": 200, "pairs": {3: 200}, "truncated": False}
    assert carryref.fetched(carryref.empty(), 3) == (0, 0, [-1, -1, -1], [0, 0, 0]) and carryref.candidates(carryref.empty()) == []
    assert carryref.info([row, carryref.empty(), carryref.merge(carryref.empty(), [(0, 1), (1, 1)], 1, 0)]) == (2, 2, 1)
    # in abundref's terms: what one part's reads give equals abundref.candidates
    rec = np.array([(2, 900, 5), (0, 1000, 7), (1, 700, 3), (3, 920, 4), (0, 400, 2), (1, 999, 0)], dtype=[("rid", "<i4"), ("dp_max", "<i4"), ("n_cigar", "<i4")])
    cg = [0, 1, 2, 1]
    for max_delta in (79, 80, 100):
        row = carryref.merge(carryref.empty(), carryref.offered(rec, cg), 16, max_delta)
        assert carryref.candidates(row) == abundref.candidates(rec, cg, max_delta)
    assert carryref.offered(rec, cg, 10) == [(10, 1000), (11, 920), (12, 900)]


# ---------------------------------------------------------------- the aligner loop
def two_part_query(tmp_path):
    query = tmp_path / "query"
    query.mkdir()
    (query / "s.fastq").write_bytes(b"@r1\nACGT\n+\nIIII\n")
    return query


def test_abundance_true_with_two_parts_still_raises(tmp_path):
    from monica_amd import aligner
    query = two_part_query(tmp_path)
    cwd = os.getcwd()
    try:
        for abundance in (True, {"max_delta": 40}, {"across_parts": False}):
            with pytest.raises(ValueError, match="ONE index part"):
                aligner.multi_threaded_aligner(str(query), ["index0.mmi", "index1.mmi"], mode="basic", abundance=abundance)
        assert os.getcwd() == cwd and sorted(os.listdir(query)) == ["s.fastq"]
    finally:
        os.chdir(cwd)


def test_across_parts_passes_the_multi_part_check(tmp_path):
    """With "across_parts" the call gets past the refusal and on to loading the first part -- which does not exist here, so
    that is where it ends, with another error than ABUNDANCE_MULTI_PART."""
    from monica_amd import aligner
    query = two_part_query(tmp_path)
    cwd = os.getcwd()
    try:
        with pytest.raises(Exception) as err:
            aligner.multi_threaded_aligner(str(query), [str(tmp_path / "index0.mmi"), str(tmp_path / "index1.mmi")], mode="basic",
                                           abundance={"across_parts": True, "width": 4})
        assert "ONE index part" not in str(err.value)
        assert not list((query / "mapped").glob("*.abundance.csv")) if (query / "mapped").exists() else True
    finally:
        os.chdir(cwd)
