"""Drop-in for the slice of `mappy` that monica consumes.

The reference uses exactly this surface (monica/genomes/aligner.py):

* `mappy.Aligner(fn_idx_in=<fasta.gz>, preset='map-ont', best_n=15, fn_idx_out=<path>)`  (45-46)
* `mappy.Aligner(fn_idx_in=<index file>)`                                                  (59)
* truthiness of the object (`if not index: raise ...`)                                     (47, 60)
* `index.map(str(seq))` yielding hits with `.is_primary .mapq .ctg .NM .mlen`              (193-195, 215-217)

`Aligner.map` is the per-read slow path kept for fidelity; `Aligner.map_batch` is what
`monica_amd.aligner.aligner` uses: one C-ABI call per micro-batch, all compute on the GPU.
Hits carry what mappy computes with its always-on base-level alignment (MM_F_CIGAR): `mapq` from
the DP branch of minimap2's formula, `mlen` / `blen` / `NM = blen - mlen + n_ambi` from the CIGAR
(the restatement is unpinned against the real library, see there).
"""
import os
import sys
import threading

import numpy as np

from . import _capi


# monica re-invokes `index_loader` on every pass of its real-time loop (aligner.py:56-62 from
# monica.py:437-439); the loaded index and its device-resident tables are kept across those
# calls, keyed by the file's identity, so a pass does not pay the load and upload again.
_INDEX_CACHE = {}
# re-entrant: `Aligner.__del__` takes it, and the collector may run a finaliser on the thread that already holds it
# (any allocation inside a locked region can start a collection); the locked regions below iterate over snapshots
_INDEX_CACHE_LOCK = threading.RLock()
_INDEX_CACHE_MAX = 4
# ... and by bytes: the reference holds ONE part at a time (aligner.py:91-103 rebinds `index` per part); a
# database of many parts kept resident would exhaust host memory or HBM.  Host side: the file sizes of the
# cached parts against a share of physical memory; device side: what the parts' tables and the idle engines'
# batch buffers hold against a share of the device's HBM (the alignment scratch is one per device and is not
# counted).  The most recently used part always stays.
_HOST_SHARE, _DEVICE_SHARE = 0.5, 0.6
_CACHE_BYTES = {}                    # key -> file size (the in-memory form of a part is about its file)
# idle engines (stream + per-batch HBM buffers), per DEVICE: an engine is not tied to an index part -- it is
# rebound to the part at hand (`mnc_engine_set_index`), as the reference's threads keep running while `index` is
# rebound in the loop over the parts (aligner.py:91-103).  So a database of many parts needs as many engines as
# monica has threads, not threads x parts.  (Kept outside the Index objects: an Engine refers to its Index.)
_ENGINE_POOLS = {}
_POOL_MAX_PER_DEVICE = 8


def reserve_index_cache(n_parts):
    """Make room for every part of a multi-part database (monica loops over all parts on every
    pass, aligner.py:91-103: a cache smaller than the loop would miss on every load).  The byte
    bounds still hold: parts that do not fit together are loaded again, as the reference does."""
    global _INDEX_CACHE_MAX
    with _INDEX_CACHE_LOCK:
        _INDEX_CACHE_MAX = max(_INDEX_CACHE_MAX, int(n_parts))


def _host_budget():
    try:
        return int(os.sysconf("SC_PAGE_SIZE") * os.sysconf("SC_PHYS_PAGES") * _HOST_SHARE)
    except (ValueError, OSError):
        return 1 << 62


def _device_budget(device):
    try:
        return int(_capi.device_mem_info(device)[1] * _DEVICE_SHARE)
    except _capi.MncError:
        return 1 << 62                                         # no device: nothing is resident either


def _device_bytes_locked(device):
    # (a closed handle holds nothing)
    n = sum(index.device_bytes(device) for index in list(_INDEX_CACHE.values()) if getattr(index, "_h", True))
    return n + sum(eng.device_bytes() for eng in list(_ENGINE_POOLS.get(device, [])) if getattr(eng, "_h", True))


def _drop_locked(key):
    old = _INDEX_CACHE.pop(key)
    _CACHE_BYTES.pop(key, None)
    for pool in _ENGINE_POOLS.values():                        # idle engines still bound to the part would keep it alive
        for eng in [e for e in pool if e.index is old]:
            pool.remove(eng)
            eng.close()
    # the Index frees its host and device tables when the last Aligner using it lets go


def _evict_locked(device=None):
    """Least recently used parts go until the count and both byte budgets hold (the newest stays)."""
    while len(_INDEX_CACHE) > _INDEX_CACHE_MAX:
        _drop_locked(next(iter(_INDEX_CACHE)))
    host = _host_budget()
    while len(_INDEX_CACHE) > 1 and sum(_CACHE_BYTES.values()) > host:
        _drop_locked(next(iter(_INDEX_CACHE)))
    if device is not None:
        dev = _device_budget(device)
        while len(_INDEX_CACHE) > 1 and _device_bytes_locked(device) > dev:
            _drop_locked(next(iter(_INDEX_CACHE)))
        pool = _ENGINE_POOLS.get(device, [])
        while pool and _device_bytes_locked(device) > dev:      # one part alone and still over: the idle engines go
            pool.pop().close()


def release_idle(keep_index=None):
    """Free what the cache holds beyond `keep_index`: every idle engine and every other part.
    Called when an allocation fails (MNC_ERR_NOMEM) before the one retry."""
    with _INDEX_CACHE_LOCK:
        for key in [k for k, v in _INDEX_CACHE.items() if v is not keep_index]:
            _drop_locked(key)
        for pool in _ENGINE_POOLS.values():
            while pool:
                pool.pop().close()


def _load_index_cached(path, device=None):
    st = os.stat(path)
    key = (os.path.realpath(path), st.st_mtime_ns, st.st_size)
    with _INDEX_CACHE_LOCK:
        hit = _INDEX_CACHE.get(key)
        if hit is not None:
            _INDEX_CACHE[key] = _INDEX_CACHE.pop(key)          # most recently used last
            return hit
    try:
        index = _capi.Index.load(path)
    except _capi.MncError as e:
        if e.code != _capi.ERR_NOMEM:
            raise
        release_idle()
        index = _capi.Index.load(path)
    with _INDEX_CACHE_LOCK:
        _INDEX_CACHE[key] = index
        _CACHE_BYTES[key] = st.st_size
        _evict_locked(device)
    return index


def _is_cached(index):
    return any(v is index for v in _INDEX_CACHE.values())


def default_device():
    for var in ("MONICA_AMD_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(var)
        if v is not None and v.strip().lstrip("-").isdigit():
            return int(v)
    return 0


def long_reads_default():
    """MONICA_AMD_LONG_READS=1: reads of 2^20 bases or more are classified (`mnc_engine_set_long_reads`); anything
    else, or unset: they come back SKIPPED, as ever."""
    return os.environ.get("MONICA_AMD_LONG_READS", "").strip() == "1"


def _build_device(device):
    """The device that sketches and sorts an index being built (csrc/k_idxbuild.hip), or None for the host builder
    when no device is visible (building an index is not part of the classified path; both give the same index)."""
    try:
        return device if 0 <= device < _capi.device_count() else None
    except _capi.MncError:
        return None


class Hit:
    """The attributes of a mappy alignment."""
    __slots__ = ("ctg", "ctg_len", "r_st", "r_en", "q_st", "q_en", "strand", "mapq", "mlen", "blen", "NM",
                 "is_primary", "score", "n_anchors", "cigar", "cs", "MD", "trans_strand", "read_num")

    @classmethod
    def from_record(cls, rec, index, cigar_words, cs=None, md=None):
        """From one alignment record of `Engine.alignments()` (ALN_DTYPE) and the pools it points into."""
        h = cls.__new__(cls)
        rid = int(rec["rid"])
        h.ctg, h.ctg_len = index.contig_names[rid], index.contig_lens[rid]
        h.r_st, h.r_en, h.q_st, h.q_en = int(rec["rs"]), int(rec["re"]), int(rec["qs"]), int(rec["qe"])
        h.strand = -1 if rec["rev"] else 1
        h.mapq, h.mlen, h.blen, h.NM = int(rec["mapq"]), int(rec["mlen"]), int(rec["blen"]), int(rec["nm"])
        o, n = int(rec["cigar_off"]), int(rec["n_cigar"])
        h.cigar = [[int(w) >> 4, int(w) & 0xf] for w in cigar_words[o:o + n]]
        h.is_primary = bool(int(rec["flags"]) & _capi.ALN_PRIMARY)
        h.score, h.n_anchors = int(rec["score"]), int(rec["cnt"])
        h.cs = bytes(cs[int(rec["cs_off"]):int(rec["cs_off"]) + int(rec["cs_len"])]).decode() if cs is not None else ""
        h.MD = bytes(md[int(rec["md_off"]):int(rec["md_off"]) + int(rec["md_len"])]).decode() if md is not None else ""
        h.trans_strand, h.read_num = 0, 1
        return h

    def __init__(self, reg, index, cigar=None):
        self.cs, self.MD, self.trans_strand, self.read_num = "", "", 0, 1      # (mappy: empty unless asked for; unspliced, unpaired)
        rid = int(reg["rid"])
        self.ctg = index.contig_names[rid]
        self.ctg_len = index.contig_lens[rid]
        self.r_st, self.r_en = int(reg["rs"]), int(reg["re"])
        self.q_st, self.q_en = int(reg["qs"]), int(reg["qe"])
        self.strand = -1 if reg["rev"] else 1
        self.mapq = int(reg["mapq"])
        self.mlen, self.blen = int(reg["mlen"]), int(reg["blen"])
        self.NM = self.blen - self.mlen + int(reg["n_ambi"])
        self.cigar = [[l, "MID".index(op)] for l, op in cigar] if cigar else []      # mappy: [[length, op], ...]
        self.is_primary = bool(reg["id"] == reg["parent"])
        self.score = int(reg["score"])
        self.n_anchors = int(reg["cnt"])

    @property
    def cigar_str(self):
        return "".join(f"{l}{'MID'[op]}" for l, op in self.cigar)

    def __repr__(self):
        return (f"{self.q_st}\t{self.q_en}\t{'+' if self.strand > 0 else '-'}\t{self.ctg}\t{self.ctg_len}\t"
                f"{self.r_st}\t{self.r_en}\t{self.mlen}\t{self.blen}\t{self.mapq}\t"
                f"tp:A:{'P' if self.is_primary else 'S'}")


# What `fn_idx_out` writes: "native" (this library's file: loads without sorting) or "mmi" (minimap2's format, as
# mappy writes it at aligner.py:45-46 -- for an installation that also runs the reference).  Both load.
INDEX_FILE_FORMAT = "native"


class Aligner:
    """Index handle with mappy's constructor and truthiness."""

    def __init__(self, fn_idx_in=None, preset=None, k=None, w=None, min_cnt=None, min_chain_score=None,
                 min_dp_score=None, bw=None, best_n=None, n_threads=3, fn_idx_out=None, max_frag_len=None,
                 extra_flags=None, seq=None, scoring=None, device=None, long_reads=None):
        self._index = None
        # reads of 2^20 bases or more (up to _capi.MAX_READ_LEN_WIDE): classified when on; None: by MONICA_AMD_LONG_READS
        self._long_reads = long_reads_default() if long_reads is None else bool(long_reads)
        self._borrowed = []
        self._tls = threading.local()
        self._device = default_device() if device is None else int(device)
        self.error = None
        kk = 15 if k is None else int(k)
        ww = 10 if w is None else int(w)
        try:
            if seq is not None:
                self._index = _capi.Index.from_seqs(["N/A"], [seq], kk, ww)
            elif fn_idx_in is None:
                raise ValueError("fn_idx_in or seq is required")
            elif self._is_index_file(fn_idx_in):
                self._index = _load_index_cached(fn_idx_in, self._device)
            elif INDEX_FILE_FORMAT == "mmi" and fn_idx_out:
                self._index = _capi.Index.build(fn_idx_in, None, kk, ww, device=_build_device(self._device))
                self._index.save(fn_idx_out, mmi=True)
            else:
                self._index = _capi.Index.build(fn_idx_in, fn_idx_out, kk, ww, device=_build_device(self._device))
        except (_capi.MncError, OSError, ValueError) as e:      # mappy: a falsy Aligner, no exception ...
            self.error = e
            self._index = None
            print(f"[monica_amd] {fn_idx_in}: {type(e).__name__}: {e}", file=sys.stderr)     # ... and the C layer's line on stderr

    @staticmethod
    def _is_index_file(path):
        try:
            with open(path, "rb") as f:
                head = f.read(6)
                return head == b"MNCIDX" or head[:4] == b"MMI\x02"       # this library's file, or minimap2's own
        except OSError:
            return False

    def __bool__(self):
        return self._index is not None

    @property
    def index(self):
        return self._index

    @property
    def k(self):
        return self._index.k

    @property
    def w(self):
        return self._index.w

    @property
    def n_seq(self):
        return len(self._index.contig_names)

    @property
    def seq_names(self):
        return list(self._index.contig_names)

    def engine(self):
        """One engine (HIP stream + HBM batch buffers) per calling thread: the reference shares one
        index between the threads of its pool (aligner.py:89-103).  Engines outlive this object and
        are not tied to an index part: an idle engine of the device is rebound to this part."""
        e = getattr(self._tls, "engine", None)
        if e is None:
            with _INDEX_CACHE_LOCK:
                pool = _ENGINE_POOLS.setdefault(self._device, [])
                e = pool.pop() if pool else None
            if e is not None:
                try:
                    e.set_index(self._index)
                except _capi.MncError:                         # made for another k / w: not reusable here
                    e.close()
                    e = None
            if e is None:
                try:
                    e = _capi.Engine(self._index, self._device)
                except _capi.MncError as err:                  # HBM exhausted: free what is idle, once
                    if err.code != _capi.ERR_NOMEM:
                        raise
                    release_idle(self._index)
                    e = _capi.Engine(self._index, self._device)
            # every engine this object hands out, a pooled one that was rebound included
            e.set_long_reads(self._long_reads)
            self._tls.engine = e
            with _INDEX_CACHE_LOCK:
                self._borrowed.append(e)
        return e

    def __del__(self):
        try:
            if self._index is not None and self._borrowed:
                with _INDEX_CACHE_LOCK:
                    pool = _ENGINE_POOLS.setdefault(self._device, [])
                    # only engines of a cached part go back: one bound to an uncached index would keep that index alive
                    room = max(0, _POOL_MAX_PER_DEVICE - len(pool)) if _is_cached(self._index) else 0
                    keep, rest = self._borrowed[:room], self._borrowed[room:]
                    for eng in keep:                           # back to the pool as it came: the switch is this object's
                        eng.set_long_reads(False)
                    pool.extend(keep)
                    self._borrowed = []
                for eng in rest:                               # not pooled: release the HBM now
                    eng.close()
                with _INDEX_CACHE_LOCK:                        # the returned engines count against the device budget
                    _evict_locked(self._device)
        except Exception:
            pass

    # ------------------------------------------------------------------ batched fast path
    def coverage(self, bin_bases=1024):
        """A coverage accumulator (`_capi.Coverage`) for this index on this object's device: pass it to `map_batch`."""
        return _capi.Coverage(self._index, self._device, bin_bases)

    def pileup(self):
        """A per-base pileup accumulator (`_capi.Pileup`) for this index on this object's device: pass it to `map_batch`."""
        return _capi.Pileup(self._index, self._device)

    def abundance(self, cap_cands=_capi.ABUNDANCE_CAP_CANDS, max_delta=_capi.ABUNDANCE_MAX_DELTA, scale_q=_capi.ABUNDANCE_SCALE_Q):
        """An abundance accumulator (`_capi.Abundance`) for this index on this object's device: pass it to `map_batch`,
        then `solve()` it."""
        return _capi.Abundance(self._index, self._device, cap_cands, max_delta, scale_q)

    def carry(self, cap_reads=0, width=_capi.CARRY_WIDTH, max_delta=_capi.ABUNDANCE_MAX_DELTA):
        """A candidate carry (`_capi.Carry`) on this object's device, for a database of several index parts: every part's
        engine carries its batches into it (`Engine.carry_candidates`), and `abundance_global` takes it at the end."""
        return _capi.Carry(self._device, cap_reads, width, max_delta)

    def abundance_global(self, genome_names, cap_cands=_capi.ABUNDANCE_CAP_CANDS, max_delta=_capi.ABUNDANCE_MAX_DELTA, scale_q=_capi.ABUNDANCE_SCALE_Q):
        """An abundance accumulator for the genomes of a whole database (`_capi.Abundance.global_`) on this object's device."""
        return _capi.Abundance.global_(self._device, len(genome_names), cap_cands, max_delta, scale_q, genome_names=genome_names)

    def map_batch(self, bases, offsets, min_mapq=0, coverage=None, coverage_what=_capi.COV_ASSIGNED, pileup=None, pileup_what=_capi.COV_GATED,
                  abundance=None):
        """Classify one micro-batch.  Returns (assign, best, nhits, hit_offsets, hits) where
        hits[hit_offsets[r]:hit_offsets[r+1]] are the (rid, mapq, nm, mlen) of the hits of read r
        that pass `is_primary and mapq >= min_mapq`.  With `coverage` (an accumulator of `coverage()`), the batch is
        added to it -- `coverage_what`: one `_capi.COV_*` selector, optionally | COV_SPAN -- before the hits are fetched; with
        `pileup` (an accumulator of `pileup()`) likewise, `pileup_what` one selector; with `abundance` (an accumulator of
        `abundance()`) every read's candidate genomes are added to it."""
        eng = self.engine()
        try:
            assign, best, nhits = eng.classify(bases, offsets, min_mapq)
        except _capi.MncError as err:                          # the batch's buffers did not fit beside the cache
            if err.code != _capi.ERR_NOMEM:
                raise
            release_idle(self._index)
            assign, best, nhits = eng.classify(bases, offsets, min_mapq)
        if coverage is not None:
            eng.add_coverage(coverage, coverage_what)
        if pileup is not None:
            eng.add_pileup(pileup, pileup_what)
        if abundance is not None:
            eng.add_abundance(abundance)
        hit_off, hits = eng.fetch_hits()
        return assign, best, nhits, hit_off, hits

    # ------------------------------------------------------------------ per-read compatibility path
    def map(self, seq, seq2=None, buf=None, cs=False, MD=False, max_frag_len=None, extra_flags=None):
        if self._index is None:
            return
        b = seq if isinstance(seq, (bytes, bytearray)) else str(seq).encode()
        eng = self.engine()
        eng.classify(np.frombuffer(b, dtype=np.uint8), np.array([0, len(b)], dtype=np.int64), 0)
        _, recs, cig, cs_b, md_b = eng.alignments(cs=cs, MD=MD)
        for rec in recs:
            yield Hit.from_record(rec, self._index, cig, cs_b if cs else None, md_b if MD else None)

    def map_batch_alignments(self, bases, offsets, cs=False, MD=False, min_mapq=0):
        """Everything `map()` yields, for a whole batch in one go: (aln_offsets[n + 1], records (`_capi.ALN_DTYPE`), cigar
        words, cs bytes, md bytes) -- `Engine.alignments()` of the batch; `min_mapq` only sets the records' gate bit.  The
        engine holds one pass: with long reads on, a batch that mixes reads of 2^20 bases or more with shorter ones is
        classified as two calls here and the two sets of records are merged by read ordinal."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        eng = self.engine()
        lens = np.diff(offsets)
        long_ = lens > _capi.MAX_READ_LEN
        if not self._long_reads or not long_.any() or long_.all():
            eng.classify(bases, offsets, min_mapq)
            return eng.alignments(cs=cs, MD=MD)
        parts = []
        for sel in (np.flatnonzero(~long_), np.flatnonzero(long_)):
            sub_b, sub_o = _take_reads(bases, offsets, sel)
            eng.classify(sub_b, sub_o, min_mapq)
            parts.append((sel,) + eng.alignments(cs=cs, MD=MD))
        return _merge_alignments(n, parts)

    def seq(self, name, start=0, end=0x7fffffff):
        """mappy's `Aligner.seq`: bases [start, end) of contig `name` (end clipped to the contig), None for an unknown
        name or an empty / inverted interval."""
        if self._index is None:
            return None
        try:
            rid = self._index.contig_names.index(name)
        except ValueError:
            return None
        end = min(int(end), self._index.contig_lens[rid])
        if start < 0 or start >= end:
            return None
        return self._index.getseq(rid, int(start), end).decode()


def _take_reads(bases, offsets, sel):
    """The reads `sel` (ordinals) of a batch as a batch of their own."""
    out_o = np.zeros(len(sel) + 1, dtype=np.int64)
    np.cumsum(offsets[sel + 1] - offsets[sel], out=out_o[1:])
    out_b = np.concatenate([bases[offsets[r]:offsets[r + 1]] for r in sel]) if out_o[-1] else np.zeros(0, dtype=np.uint8)
    return out_b, out_o


def _merge_alignments(n, parts):
    """Records of several calls over disjoint reads of one batch -> one set in read order.  parts: (read ordinals of the
    call, offsets, records, cigar, cs, md); pool offsets and `read` are rewritten for the merged pools."""
    owner = np.zeros(n, dtype=np.int64)
    local = np.zeros(n, dtype=np.int64)
    for k, part in enumerate(parts):
        owner[part[0]], local[part[0]] = k, np.arange(len(part[0]))
    offs = np.zeros(n + 1, dtype=np.int64)
    recs, pools = [], [[], [], []]
    fill = [0, 0, 0]
    for r in range(n):
        _, off, rec, cig, cs_b, md_b = parts[owner[r]]
        lo, hi = off[local[r]], off[local[r] + 1]
        for a in rec[lo:hi]:
            a = a.copy()
            a["read"] = r
            for j, (src, o_key, n_key) in enumerate(((cig, "cigar_off", "n_cigar"), (cs_b, "cs_off", "cs_len"), (md_b, "md_off", "md_len"))):
                pools[j].append(src[a[o_key]:a[o_key] + a[n_key]])
                a[o_key] = fill[j]
                fill[j] += int(a[n_key])
            recs.append(a)
        offs[r + 1] = len(recs)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt, copy=False) if xs else np.zeros(0, dtype=dt)
    records = np.array(recs, dtype=_capi.ALN_DTYPE) if recs else np.zeros(0, dtype=_capi.ALN_DTYPE)
    return offs, records, cat(pools[0], np.uint32), cat(pools[1], np.uint8), cat(pools[2], np.uint8)
