"""The switch for reads of 2^20 bases or more, as far as it can be checked without a device: the entry point in the
header, the library and the binding, its argument check, and how `mappy_compat.Aligner` applies it to the engines it
hands out (a stub engine stands in for the device)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "monica_amd.h")) as f:
        return f.read()


def test_the_entry_point_is_declared_exported_and_bound(capi):
    assert re.search(r"\bint\s+mnc_engine_set_long_reads\s*\(\s*mnc_engine\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", _header())
    assert "mnc_engine_set_long_reads" in capi.EXPORTS
    assert hasattr(capi.lib(), "mnc_engine_set_long_reads")
    assert callable(getattr(capi.Engine, "set_long_reads", None))


def test_a_null_engine_is_an_argument_error(capi):
    for on in (0, 1):
        assert capi.lib().mnc_engine_set_long_reads(None, on) == capi.ERR_ARG


def test_the_limits_in_the_header_are_the_bindings(capi):
    defs = dict(re.findall(r"^#define\s+(MNC_MAX_READ\w+)\s+(.+?)\s*$", _header(), flags=re.M))
    value = lambda text: eval(text, {"__builtins__": {}})            # "((1 << 24) - 1)": integer arithmetic only
    assert re.fullmatch(r"[\d\s()<\-+]+", defs["MNC_MAX_READ_LEN_WIDE"]) and re.fullmatch(r"[\d\s()<\-+]+", defs["MNC_MAX_READS_WIDE"])
    assert value(defs["MNC_MAX_READ_LEN_WIDE"]) == capi.MAX_READ_LEN_WIDE == (1 << 24) - 1
    assert value(defs["MNC_MAX_READS_WIDE"]) == capi.MAX_READS_WIDE == 1 << 16
    assert capi.MAX_READ_LEN == (1 << 20) - 1


class _StubEngine:
    made = []

    def __init__(self, index, device=0):
        self.index, self.device, self.long_reads, self.calls, self._h = index, device, None, [], True
        _StubEngine.made.append(self)

    def set_index(self, index):
        self.index = index
        self.calls.append("set_index")

    def set_long_reads(self, on=True):
        self.long_reads = bool(on)
        self.calls.append(("set_long_reads", bool(on)))

    def device_bytes(self):
        return 0

    def close(self):
        self._h = None


@pytest.fixture()
def stubbed(capi, monkeypatch):
    from monica_amd import mappy_compat
    monkeypatch.setattr(capi, "Engine", _StubEngine)
    monkeypatch.setattr(mappy_compat, "_ENGINE_POOLS", {})
    monkeypatch.setattr(mappy_compat, "_INDEX_CACHE", {})
    monkeypatch.setattr(mappy_compat, "_device_budget", lambda device: 1 << 62)
    monkeypatch.delenv("MONICA_AMD_LONG_READS", raising=False)
    _StubEngine.made = []
    return mappy_compat


def _seq():
    return np.frombuffer(b"ACGTTGCAGTCCATGACGTAGCTAGGATCCATGCAATTGGCCATGCATCGATCGGATTAGC" * 4, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("env, arg, want", [(None, None, False), ("1", None, True), ("0", None, False), ("true", None, False), ("", None, False),
                                            (" 1 ", None, True), ("1", False, False), (None, True, True), ("0", True, True)])
def test_aligner_takes_the_switch_from_its_argument_or_the_environment(stubbed, monkeypatch, env, arg, want):
    if env is not None:
        monkeypatch.setenv("MONICA_AMD_LONG_READS", env)
    al = stubbed.Aligner(seq=_seq(), long_reads=arg, device=0)
    assert al
    eng = al.engine()
    assert isinstance(eng, _StubEngine) and eng.long_reads is want
    assert al.engine() is eng and eng.calls.count(("set_long_reads", want)) == 1       # one engine a thread, set once


def test_pooled_engines_get_the_switch_and_go_back_without_it(stubbed):
    first = stubbed.Aligner(seq=_seq(), long_reads=True, device=0)
    stubbed._INDEX_CACHE["part"] = first.index                      # a cached part: its engines are pooled, not closed
    eng = first.engine()
    assert eng.long_reads is True
    first.__del__()
    pool = stubbed._ENGINE_POOLS[0]
    assert pool == [eng] and eng.long_reads is False                # back in the pool with the switch reset
    # the next object is handed the pooled engine, rebound, with its own setting
    second = stubbed.Aligner(seq=_seq(), long_reads=True, device=0)
    stubbed._INDEX_CACHE["part2"] = second.index
    again = second.engine()
    assert again is eng and eng.calls[-2:] == ["set_index", ("set_long_reads", True)] and len(_StubEngine.made) == 1
    second.__del__()
    third = stubbed.Aligner(seq=_seq(), device=0)                   # default: off
    assert third.engine() is eng and eng.long_reads is False and eng.calls[-1] == ("set_long_reads", False)
    third._borrowed = []
