"""ctypes binding of ``libmonica_amd.so`` (C-ABI: ``include/monica_amd.h``).

The library holds the hand-written gfx950 kernels; there is no CPU execution path.  Loading
fails loudly when the shared object is missing -- build it with ``python -c 'import
__graft_entry__ as g; g.build()'`` or ``make -C monica_amd/csrc``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# The host passes of the library (FASTQ parse, routing, index build) are OpenMP teams started from several Python threads
# at once; with an ACTIVE wait policy their idle threads spin on every core and the pipeline of aligner.py runs 15x slower
# (measured: 2.7 s instead of 0.16 s per GB of FASTQ).  Only a default: a policy the user has set is left alone.
os.environ.setdefault("OMP_WAIT_POLICY", "passive")
LIB_PATH = os.environ.get("MONICA_AMD_LIB") or os.path.join(_HERE, "libmonica_amd.so")   # (the override: an experimental build of the same ABI)

OK = 0
ERR_ARG, ERR_IO, ERR_FORMAT, ERR_NOMEM, ERR_HIP, ERR_NODEVICE, ERR_UNSUPPORTED, ERR_RANGE = range(-1, -9, -1)
UNMAPPED = -1
AMBIGUOUS = -2
SKIPPED = -3            # MNC_SKIPPED: a read outside the kernels' limits (include/monica_amd.h, "limits"): not classified, no hits

HIT_DTYPE = np.dtype([("rid", "<i4"), ("mapq", "<i4"), ("nm", "<i4"), ("mlen", "<i4")])
REG_DTYPE = np.dtype([("id", "<i4"), ("parent", "<i4"), ("rid", "<i4"), ("rev", "<i4"),
                      ("rs", "<i4"), ("re", "<i4"), ("qs", "<i4"), ("qe", "<i4"),
                      ("score", "<i4"), ("score0", "<i4"), ("cnt", "<i4"), ("as", "<i4"),
                      ("mlen", "<i4"), ("blen", "<i4"), ("subsc", "<i4"), ("n_sub", "<i4"),
                      ("mapq", "<i4"), ("hash", "<u4"),
                      ("dp_score", "<i4"), ("dp_max", "<i4"), ("dp_max2", "<i4"), ("n_ambi", "<i4"),
                      ("n_cigar", "<i4"), ("flags", "<i4")])
# mnc_aln_t: one alignment record of Engine.alignments() (104 bytes, no padding)
ALN_DTYPE = np.dtype([(k, "<i4") for k in ("read", "rid", "rev", "qs", "qe", "rs", "re", "mapq", "mlen", "blen", "nm", "score", "cnt",
                                           "dp_score", "dp_max", "n_ambi", "flags", "n_cigar")]
                     + [("cigar_off", "<i8"), ("cs_off", "<i8"), ("md_off", "<i8"), ("cs_len", "<i4"), ("md_len", "<i4")])
assert ALN_DTYPE.itemsize == 104
ALN_CS, ALN_MD = 1, 2
ALN_PRIMARY, ALN_GATED = 1, 2           # mnc_aln_t.flags bits 0 / 1; bits 8.. are mnc_reg_t.flags << 8
PAF_PRIMARY_ONLY = 1
# MNC_COV_*: what Engine.add_coverage adds -- exactly one selector, optionally | COV_SPAN
COV_GATED, COV_PRIMARY, COV_ALL, COV_ASSIGNED, COV_SPAN = 1, 2, 4, 8, 16
# one row per contig of Coverage.summary()
COV_SUMMARY_DTYPE = np.dtype([("covered", "<i8"), ("depth_sum", "<i8"), ("max_depth", "<i4"), ("n_aln", "<i8")])
# the planes of Pileup.counts(), in order (MNC_PILE_*), and one row of Pileup.variants() (mnc_variant_t, 20 bytes)
PILE_PLANES = ("depth", "A", "C", "G", "T", "N", "DEL", "INS")
VARIANT_DTYPE = np.dtype([("rid", "<i4"), ("pos", "<i4"), ("span", "<i4"), ("count", "<i4"), ("ref", "S1"), ("alt", "S1"), ("pad", "<u2")])
assert VARIANT_DTYPE.itemsize == 20
MZ_DTYPE = np.dtype([("hash", "<u4"), ("pos_strand", "<u4")])
ANCHOR_DTYPE = np.dtype([("x", "<u8"), ("y", "<u8")])

N_STAGES = 22
(STAGE_PACK, STAGE_SKETCH, STAGE_PARTITION, STAGE_PROBE, STAGE_COLLECT, STAGE_SORT, STAGE_SORT2, STAGE_CHAIN,
 STAGE_BACKTRACK, STAGE_REGIONS, STAGE_GATHER, STAGE_DP_PLAN, STAGE_DP_ALIGN, STAGE_DP_STITCH,
 STAGE_DP_POST, STAGE_DP_FILL, STAGE_DP_FILL_T1, STAGE_DP_FILL_T2, STAGE_DP_FILL_T3, STAGE_DP_EXT, STAGE_DP_FILL_TM, STAGE_DP_LFILL) = range(N_STAGES)
(DUMP_MINIMIZERS, DUMP_MZ_OFFSETS, DUMP_ANCHORS, DUMP_AN_OFFSETS, DUMP_CHAIN_F, DUMP_CHAIN_P,
 DUMP_CHAIN_V, DUMP_REGS, DUMP_REG_OFFSETS, DUMP_REP_LEN, DUMP_CIGARS, DUMP_SEGS, DUMP_SEG_CIGARS) = range(1, 14)
SEG_DTYPE = np.dtype([(k, np.int32) for k in ("read", "reg", "kind", "rid", "rev", "ts", "tlen", "qs", "qlen", "w", "zdrop", "flag",
                                              "ai", "big", "n_cigar", "zdropped", "zdrop_code", "max", "max_t", "max_q", "score",
                                              "reach_end", "mqe_t", "pad")] + [("cig_off", np.int64)])
CONTRACT_DP, CONTRACT_CHAIN = 0, 1
MAX_READ_LEN = (1 << 20) - 1            # the longest read the usual pass classifies
MAX_READ_LEN_WIDE = (1 << 24) - 1       # MNC_MAX_READ_LEN_WIDE: ... and the pass for long reads (Engine.set_long_reads)
MAX_READS_WIDE = 1 << 16                # MNC_MAX_READS_WIDE

# every symbol include/monica_amd.h declares (checked by tests/test_capi.py)
EXPORTS = [
    "mnc_strerror", "mnc_last_error", "mnc_device_count", "mnc_device_name", "mnc_device_mem_info",
    "mnc_index_build", "mnc_index_build_mem", "mnc_index_build_device", "mnc_index_build_mem_device", "mnc_index_save", "mnc_index_save_mmi", "mnc_index_load", "mnc_index_free",
    "mnc_index_info", "mnc_index_contig_name", "mnc_index_contig_len", "mnc_index_contig_genome",
    "mnc_index_genome_name", "mnc_index_genome_len", "mnc_index_dump", "mnc_index_set_mid_occ",
    "mnc_engine_create", "mnc_engine_destroy", "mnc_engine_stream", "mnc_engine_device_bytes", "mnc_index_device_bytes", "mnc_engine_set_index",
    "mnc_classify_batch", "mnc_engine_prefetch", "mnc_engine_prefetch_cancel", "mnc_classify_device", "mnc_engine_sync", "mnc_engine_fetch_hits",
    "mnc_counts", "mnc_best_hit",
    "mnc_engine_set_profiling", "mnc_engine_set_debug", "mnc_engine_set_contract", "mnc_engine_set_long_reads", "mnc_index_set_host_tables", "mnc_index_set_region_bits", "mnc_engine_dump_tables",
    "mnc_comm_unique_id", "mnc_comm_init_rank", "mnc_comm_destroy", "mnc_comm_count", "mnc_allreduce_counts", "mnc_allgather_summaries", "mnc_shard_summary", "mnc_merge_summaries", "mnc_engine_get_timings", "mnc_stage_name", "mnc_stage_kernel",
    "mnc_engine_get_counters", "mnc_engine_dump",
    "mnc_fastq_open", "mnc_fastq_close", "mnc_fastq_next", "mnc_fastq_detach_batch", "mnc_fastq_remaining", "mnc_fastq_bases", "mnc_fastq_offsets",
    "mnc_fastq_quals", "mnc_fastq_title", "mnc_fastq_route",
    "mnc_hitmap_create", "mnc_hitmap_load", "mnc_hitmap_save", "mnc_hitmap_free", "mnc_hitmap_size",
    "mnc_hitmap_update", "mnc_hitmap_n_names", "mnc_hitmap_name", "mnc_host_alloc", "mnc_host_free", "mnc_host_set_io_workers",
    "mnc_synth_genome", "mnc_synth_diverge", "mnc_synth_reads", "mnc_synth_reads_device", "mnc_version",
    "mnc_engine_export_alignments", "mnc_engine_fetch_alignments", "mnc_engine_alignments_device", "mnc_engine_export_ms",
    "mnc_index_getseq", "mnc_fastq_write_paf",
    "mnc_coverage_create", "mnc_coverage_free", "mnc_coverage_reset", "mnc_coverage_device_bytes", "mnc_engine_add_coverage",
    "mnc_coverage_summary", "mnc_coverage_fetch_bins", "mnc_coverage_fetch_depth", "mnc_coverage_device",
    "mnc_pileup_create", "mnc_pileup_free", "mnc_pileup_reset", "mnc_pileup_device_bytes", "mnc_pileup_device", "mnc_engine_add_pileup",
    "mnc_pileup_fetch_counts", "mnc_pileup_call_variants", "mnc_pileup_consensus",
    "mnc_abundance_create", "mnc_abundance_free", "mnc_abundance_reset", "mnc_abundance_device_bytes", "mnc_engine_add_abundance",
    "mnc_abundance_add_lists", "mnc_abundance_info", "mnc_abundance_fetch_unique", "mnc_abundance_fetch_lists", "mnc_abundance_solve",
    "mnc_abundance_device", "mnc_abundance_create_global", "mnc_abundance_add_carry",
    "mnc_carry_create", "mnc_carry_free", "mnc_carry_reset", "mnc_carry_reserve", "mnc_carry_device_bytes", "mnc_engine_carry_candidates",
    "mnc_carry_add_lists", "mnc_carry_merge", "mnc_carry_info", "mnc_carry_fetch", "mnc_carry_device",
]


class IndexInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("n_contigs", C.c_int32), ("n_genomes", C.c_int32),
                ("mid_occ", C.c_int32), ("reserved", C.c_int32), ("n_keys", C.c_int64),
                ("n_occ", C.c_int64), ("total_len", C.c_int64), ("table_slots", C.c_int64),
                ("device_bytes", C.c_int64)]


class MncError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        msg = lib().mnc_strerror(code).decode()
        super().__init__(f"{msg}" + (f": {detail}" if detail else ""))


_LIB = None


def lib():
    """Load the shared object once.  Raises if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: the HIP extension has not been built "
                          "(run __graft_entry__.build() or make -C monica_amd/csrc)")
    # PyTorch wheels bundle their own libamdhip64 under the same SONAME.  Two HIP runtimes in
    # one process cannot both open the GPU, so when torch is installed let it load its copy
    # first; our NEEDED entry then resolves to that already-loaded runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u64, u32, cp = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_uint32, C.c_char_p
    pp = C.POINTER(vp)

    def sig(name, res, args):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args

    sig("mnc_strerror", cp, [i32])
    sig("mnc_last_error", cp, [])
    sig("mnc_version", cp, [])
    sig("mnc_device_count", i32, [C.POINTER(i32)])
    sig("mnc_device_name", i32, [i32, cp, C.c_size_t])
    sig("mnc_device_mem_info", i32, [i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
    sig("mnc_index_build", i32, [cp, cp, i32, i32, pp])
    sig("mnc_index_build_mem", i32, [i32, C.POINTER(cp), C.POINTER(cp), C.POINTER(i64), i32, i32, pp])
    sig("mnc_index_build_device", i32, [cp, cp, i32, i32, i32, pp])
    sig("mnc_index_build_mem_device", i32, [i32, C.POINTER(cp), C.POINTER(cp), C.POINTER(i64), i32, i32, i32, pp])
    sig("mnc_index_save", i32, [vp, cp])
    sig("mnc_index_save_mmi", i32, [vp, cp])
    sig("mnc_index_load", i32, [cp, pp])
    sig("mnc_index_free", None, [vp])
    sig("mnc_index_info", i32, [vp, C.POINTER(IndexInfo)])
    sig("mnc_index_contig_name", cp, [vp, i32])
    sig("mnc_index_contig_len", i64, [vp, i32])
    sig("mnc_index_contig_genome", i32, [vp, i32])
    sig("mnc_index_genome_name", cp, [vp, i32])
    sig("mnc_index_genome_len", i64, [vp, i32])
    sig("mnc_index_dump", i32, [vp, vp, vp, i64, C.POINTER(i64)])
    sig("mnc_index_set_mid_occ", i32, [vp, i32])
    sig("mnc_engine_create", i32, [vp, i32, pp])
    sig("mnc_engine_destroy", None, [vp])
    sig("mnc_engine_stream", vp, [vp])
    sig("mnc_engine_prefetch", i32, [vp, vp, vp, u32, C.POINTER(C.c_int)])
    sig("mnc_engine_prefetch_cancel", i32, [vp])
    sig("mnc_engine_set_index", i32, [vp, vp])
    sig("mnc_engine_device_bytes", i32, [vp, C.POINTER(C.c_int64)])
    sig("mnc_index_device_bytes", i32, [vp, i32, C.POINTER(C.c_int64)])
    sig("mnc_classify_batch", i32, [vp, vp, vp, u32, i32, vp, vp, vp])
    sig("mnc_classify_device", i32, [vp, vp, vp, u32, i64, i32, i32, vp, vp, vp, vp])
    sig("mnc_engine_sync", i32, [vp])
    sig("mnc_engine_fetch_hits", i32, [vp, vp, vp, i64, C.POINTER(i64)])
    sig("mnc_counts", i32, [vp, vp, vp, vp, u32, i32, vp])
    sig("mnc_best_hit", i32, [vp, i32, C.POINTER(i32)])
    sig("mnc_engine_set_profiling", i32, [vp, i32])
    sig("mnc_engine_set_debug", i32, [vp, i32])
    sig("mnc_index_set_host_tables", i32, [vp, i32])
    sig("mnc_index_set_region_bits", i32, [vp, i32])
    sig("mnc_engine_dump_tables", i32, [vp, vp, C.c_int64, vp])
    sig("mnc_engine_set_contract", i32, [vp, i32])
    sig("mnc_engine_set_long_reads", i32, [vp, i32])
    sig("mnc_comm_unique_id", i32, [vp])
    sig("mnc_comm_init_rank", i32, [vp, i32, i32, C.POINTER(vp)])
    sig("mnc_comm_destroy", i32, [vp])
    sig("mnc_comm_count", i32, [vp, C.POINTER(i32)])
    sig("mnc_allreduce_counts", i32, [vp, i32, vp, vp])
    sig("mnc_allgather_summaries", i32, [vp, vp, C.c_size_t, vp, vp])
    sig("mnc_shard_summary", i32, [vp, vp, vp, i64, i32, vp, vp])
    sig("mnc_merge_summaries", i32, [vp, i32, i64, vp, vp, vp, vp, vp])
    sig("mnc_engine_get_timings", i32, [vp, vp, vp, i32])
    sig("mnc_stage_name", cp, [i32])
    sig("mnc_stage_kernel", cp, [i32])
    sig("mnc_engine_get_counters", i32, [vp, vp, i32])
    sig("mnc_engine_dump", i32, [vp, i32, vp, i64, C.POINTER(i64)])
    sig("mnc_synth_genome", i32, [u64, i64, vp])
    sig("mnc_synth_diverge", i32, [vp, i64, u64, i32, vp])
    sig("mnc_synth_reads", i32, [i32, C.POINTER(vp), C.POINTER(i64), u64, i64, i32, i32,
                                 i32, i32, i32, i32, vp, vp])
    sig("mnc_synth_reads_device", i32, [i32, vp, vp, u64, i64, i32, i32, i32, i32, i32, i32, vp, vp, vp])
    sig("mnc_fastq_open", i32, [cp, pp])
    sig("mnc_fastq_close", None, [vp])
    sig("mnc_fastq_detach_batch", i32, [vp, pp])
    sig("mnc_fastq_remaining", i32, [vp, C.POINTER(i64)])
    sig("mnc_fastq_next", i32, [vp, u32, u64, C.POINTER(u32)])
    sig("mnc_fastq_bases", vp, [vp])
    sig("mnc_fastq_offsets", vp, [vp])
    sig("mnc_fastq_quals", vp, [vp])
    sig("mnc_fastq_title", i32, [vp, u32, C.POINTER(vp), C.POINTER(u32), C.POINTER(u32)])
    sig("mnc_fastq_route", i32, [vp, vp, vp, C.POINTER(cp), i32, C.POINTER(cp)])
    sig("mnc_hitmap_create", i32, [pp])
    sig("mnc_hitmap_load", i32, [cp, pp])
    sig("mnc_hitmap_save", i32, [vp, cp])
    sig("mnc_hitmap_free", None, [vp])
    sig("mnc_hitmap_size", i64, [vp])
    sig("mnc_hitmap_update", i32, [vp, vp, vp, vp, vp, vp, vp])
    sig("mnc_hitmap_n_names", i32, [vp])
    sig("mnc_hitmap_name", cp, [vp, i32])
    sig("mnc_host_alloc", vp, [C.c_size_t])
    sig("mnc_host_free", None, [vp])
    sig("mnc_host_set_io_workers", i32, [i32])
    sig("mnc_engine_export_alignments", i32, [vp, i32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)])
    sig("mnc_engine_fetch_alignments", i32, [vp, vp, vp, i64, vp, i64, vp, i64, vp, i64])
    sig("mnc_engine_alignments_device", i32, [vp, pp, pp, pp, pp, pp])
    sig("mnc_engine_export_ms", i32, [vp, C.POINTER(C.c_double)])
    sig("mnc_index_getseq", i32, [vp, i32, i64, i64, vp])
    sig("mnc_fastq_write_paf", i32, [vp, vp, vp, vp, vp, vp, vp, i32, cp])
    sig("mnc_coverage_create", i32, [vp, i32, i32, pp])
    sig("mnc_coverage_free", None, [vp])
    sig("mnc_coverage_reset", i32, [vp])
    sig("mnc_coverage_device_bytes", i32, [vp, C.POINTER(i64)])
    sig("mnc_engine_add_coverage", i32, [vp, vp, i32])
    sig("mnc_coverage_summary", i32, [vp, vp, vp, vp, vp])
    sig("mnc_coverage_fetch_bins", i32, [vp, i32, vp, vp, i64, C.POINTER(i64)])
    sig("mnc_coverage_fetch_depth", i32, [vp, i32, i64, i64, vp])
    sig("mnc_coverage_device", i32, [vp, pp, C.POINTER(i64)])
    sig("mnc_pileup_create", i32, [vp, i32, pp])
    sig("mnc_pileup_free", None, [vp])
    sig("mnc_pileup_reset", i32, [vp])
    sig("mnc_pileup_device_bytes", i32, [vp, C.POINTER(i64)])
    sig("mnc_pileup_device", i32, [vp, pp, pp, C.POINTER(i64)])
    sig("mnc_engine_add_pileup", i32, [vp, vp, i32])
    sig("mnc_pileup_fetch_counts", i32, [vp, i32, i64, i64, vp])
    sig("mnc_pileup_call_variants", i32, [vp, i32, i32, i32, i32, vp, i64, C.POINTER(i64)])
    sig("mnc_pileup_consensus", i32, [vp, i32, i64, i64, i32, vp])
    sig("mnc_abundance_create", i32, [vp, i32, i64, C.c_int32, C.c_int32, pp])
    sig("mnc_abundance_free", None, [vp])
    sig("mnc_abundance_reset", i32, [vp])
    sig("mnc_abundance_device_bytes", i32, [vp, C.POINTER(i64)])
    sig("mnc_engine_add_abundance", i32, [vp, vp])
    sig("mnc_abundance_add_lists", i32, [vp, i64, vp, vp, vp])
    sig("mnc_abundance_info", i32, [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)])
    sig("mnc_abundance_fetch_unique", i32, [vp, vp])
    sig("mnc_abundance_fetch_lists", i32, [vp, vp, vp, vp, i64, i64])
    sig("mnc_abundance_solve", i32, [vp, C.c_int32, u64, vp, vp, C.POINTER(C.c_int32)])
    sig("mnc_abundance_device", i32, [vp, pp, pp, pp, pp])
    sig("mnc_abundance_create_global", i32, [i32, C.c_int32, i64, C.c_int32, C.c_int32, pp])
    sig("mnc_abundance_add_carry", i32, [vp, vp, i64, i64])
    sig("mnc_carry_create", i32, [i32, i64, C.c_int32, C.c_int32, pp])
    sig("mnc_carry_free", None, [vp])
    sig("mnc_carry_reset", i32, [vp])
    sig("mnc_carry_reserve", i32, [vp, i64])
    sig("mnc_carry_device_bytes", i32, [vp, C.POINTER(i64)])
    sig("mnc_engine_carry_candidates", i32, [vp, vp, i64, C.c_int32])
    sig("mnc_carry_add_lists", i32, [vp, i64, i64, vp, vp, vp])
    sig("mnc_carry_merge", i32, [vp, vp])
    sig("mnc_carry_info", i32, [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)])
    sig("mnc_carry_fetch", i32, [vp, i64, i64, vp, vp, vp, vp])
    sig("mnc_carry_device", i32, [vp, pp, pp, C.POINTER(i64), C.POINTER(C.c_int32)])
    _LIB = L
    return L


def check(code):
    if code != OK:
        raise MncError(code, lib().mnc_last_error().decode(errors="replace"))


def _b(s):
    return s if isinstance(s, (bytes, bytearray)) else str(s).encode()


class Comm:
    """An RCCL communicator made through the C-ABI (`mnc_comm_*`): rank 0 calls `Comm.unique_id()`,
    hands the 128 bytes to the other ranks by any means, every rank constructs `Comm(id, n, rank)`
    with its device current."""

    def __init__(self, unique_id, n_ranks, rank):
        h = C.c_void_p()
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        check(lib().mnc_comm_init_rank(buf, int(n_ranks), int(rank), C.byref(h)))
        self._h, self.n_ranks, self.rank = h, int(n_ranks), int(rank)

    @staticmethod
    def unique_id():
        buf = (C.c_char * 128)()
        check(lib().mnc_comm_unique_id(buf))
        return bytes(buf)

    def count(self):
        """ncclCommCount: the number of ranks RCCL itself reports for this communicator."""
        n = C.c_int32(0)
        check(lib().mnc_comm_count(self._h, C.byref(n)))
        return int(n.value)

    def allreduce_counts(self, d_counts_ptr, n, stream=None):
        check(lib().mnc_allreduce_counts(C.c_void_p(d_counts_ptr), int(n), self._h, C.c_void_p(stream or 0)))

    def allgather_summaries(self, d_send_ptr, d_recv_ptr, bytes_per_rank, stream=None):
        check(lib().mnc_allgather_summaries(C.c_void_p(d_send_ptr), C.c_void_p(d_recv_ptr), int(bytes_per_rank), self._h,
                                            C.c_void_p(stream or 0)))

    def close(self):
        if getattr(self, "_h", None):
            lib().mnc_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_summary_device(d_assign, d_best, d_nhits, n, rid_offset, d_out, stream=None):
    """`mnc_shard_summary`: one index part's 20-byte per-read records [n][5] from the device outputs of
    `mnc_classify_device`; all arguments but `n` / `rid_offset` are device addresses."""
    check(lib().mnc_shard_summary(C.c_void_p(d_assign), C.c_void_p(d_best), C.c_void_p(d_nhits), int(n), int(rid_offset),
                                  C.c_void_p(d_out), C.c_void_p(stream or 0)))


def merge_summaries_device(d_parts, n_parts, n, d_assign, d_nm=0, d_mlen=0, d_total=0, stream=None):
    """`mnc_merge_summaries`: best_hit over [n_parts][n][5] records in part order (device addresses)."""
    check(lib().mnc_merge_summaries(C.c_void_p(d_parts), int(n_parts), int(n), C.c_void_p(d_assign), C.c_void_p(d_nm or 0),
                                    C.c_void_p(d_mlen or 0), C.c_void_p(d_total or 0), C.c_void_p(stream or 0)))


def set_io_workers(n):
    """`mnc_host_set_io_workers`: the FASTQ readers' parse / routing teams share the cores over `n` samples in flight."""
    check(lib().mnc_host_set_io_workers(int(max(1, n))))


def pinned_array(a):
    """A copy of `a` in page-locked host memory (mnc_host_alloc), as the FASTQ reader's batches are."""
    a = np.ascontiguousarray(a)
    L = lib()
    L.mnc_host_alloc.restype = C.c_void_p
    L.mnc_host_alloc.argtypes = [C.c_size_t]
    p = L.mnc_host_alloc(max(a.nbytes, 1))
    out = np.frombuffer((C.c_uint8 * max(a.nbytes, 1)).from_address(p), dtype=np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out                                          # (freed with the process)


def device_count():
    n = C.c_int(0)
    check(lib().mnc_device_count(C.byref(n)))
    return n.value


def device_mem_info(device=0):
    """(free, total) HBM bytes of a device."""
    f, t = C.c_int64(0), C.c_int64(0)
    check(lib().mnc_device_mem_info(device, C.byref(f), C.byref(t)))
    return f.value, t.value


# ---------------------------------------------------------------------------------- index
class Index:
    """Owner of an ``mnc_index`` handle (the object mappy.Aligner is for monica)."""

    def __init__(self, handle):
        self._h = handle
        info = self.info()
        self.k, self.w = info.k, info.w
        L = lib()
        self.contig_names = [L.mnc_index_contig_name(handle, i).decode() for i in range(info.n_contigs)]
        self.contig_lens = [int(L.mnc_index_contig_len(handle, i)) for i in range(info.n_contigs)]
        self.contig_genome = np.array([L.mnc_index_contig_genome(handle, i) for i in range(info.n_contigs)],
                                      dtype=np.int32)
        self.genome_names = [L.mnc_index_genome_name(handle, g).decode() for g in range(info.n_genomes)]
        self.genome_lens = [int(L.mnc_index_genome_len(handle, g)) for g in range(info.n_genomes)]

    @classmethod
    def build(cls, fasta_path, out_path=None, k=15, w=10, device=None):
        h = C.c_void_p()
        if device is None:
            check(lib().mnc_index_build(_b(fasta_path), _b(out_path) if out_path else None, k, w, C.byref(h)))
        else:                                       # sketch + sort on that device: the same index
            check(lib().mnc_index_build_device(_b(fasta_path), _b(out_path) if out_path else None, k, w, int(device), C.byref(h)))
        return cls(h)

    @classmethod
    def from_seqs(cls, names, seqs, k=15, w=10, device=None):
        n = len(names)
        bn = [_b(x) for x in names]
        bs = [x if isinstance(x, (bytes, bytearray)) else (x.tobytes() if isinstance(x, np.ndarray) else _b(x))
              for x in seqs]
        an = (C.c_char_p * n)(*bn)
        as_ = (C.c_char_p * n)(*bs)
        al = (C.c_int64 * n)(*[len(x) for x in bs])
        h = C.c_void_p()
        if device is None:
            check(lib().mnc_index_build_mem(n, an, as_, al, k, w, C.byref(h)))
        else:                                       # sketch + sort on that device: the same index
            check(lib().mnc_index_build_mem_device(n, an, as_, al, k, w, int(device), C.byref(h)))
        return cls(h)

    @classmethod
    def load(cls, path):
        h = C.c_void_p()
        check(lib().mnc_index_load(_b(path), C.byref(h)))
        return cls(h)

    def save(self, path, mmi=False):
        """This library's own file (loads without a sort), or -- `mmi=True` -- minimap2's format, the one mappy writes at
        aligner.py:45-46; `load` reads either."""
        check((lib().mnc_index_save_mmi if mmi else lib().mnc_index_save)(self._h, _b(path)))

    def info(self):
        info = IndexInfo()
        check(lib().mnc_index_info(self._h, C.byref(info)))
        return info

    def device_bytes(self, device):
        """HBM this index holds on one device (info().device_bytes sums over all devices)."""
        n = C.c_int64(0)
        check(lib().mnc_index_device_bytes(self._h, int(device), C.byref(n)))
        return int(n.value)

    @property
    def mid_occ(self):
        return self.info().mid_occ

    def set_mid_occ(self, v):
        check(lib().mnc_index_set_mid_occ(self._h, int(v)))

    def getseq(self, rid, start=0, end=None):
        """Bases [start, end) of contig `rid` as bytes over "ACGTN" (`mnc_index_getseq`; MncError ERR_ARG out of range)."""
        end = (self.contig_lens[rid] if 0 <= rid < len(self.contig_lens) else 0) if end is None else int(end)
        buf = C.create_string_buffer(max(end - int(start), 1))
        check(lib().mnc_index_getseq(self._h, int(rid), int(start), end, buf))
        return buf.raw[:max(end - int(start), 0)]

    def dump(self):
        n = C.c_int64(0)
        lib().mnc_index_dump(self._h, None, None, 0, C.byref(n))
        h = np.zeros(n.value, dtype=np.uint64)
        y = np.zeros(n.value, dtype=np.uint64)
        check(lib().mnc_index_dump(self._h, h.ctypes.data, y.ctypes.data, n.value, C.byref(n)))
        return h, y

    def close(self):
        if getattr(self, "_h", None):
            lib().mnc_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------- engine
class Engine:
    """One HIP stream + HBM workspace on one device, bound to one index."""

    def __init__(self, index, device=0):
        self.index = index
        self.device = device
        h = C.c_void_p()
        check(lib().mnc_engine_create(index._h, device, C.byref(h)))
        self._h = h
        self.n_reads = 0

    def close(self):
        if getattr(self, "_h", None):
            lib().mnc_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return lib().mnc_engine_stream(self._h)

    def set_index(self, index):
        """Another index part behind the same stream and batch buffers (aligner.py:91-103 rebinds `index`)."""
        check(lib().mnc_engine_set_index(self._h, index._h))
        self.index = index

    def device_bytes(self):
        """HBM held by this engine's own batch buffers."""
        n = C.c_int64(0)
        check(lib().mnc_engine_device_bytes(self._h, C.byref(n)))
        return n.value

    def classify(self, bases, offsets, min_mapq=60):
        """Host buffers in, host arrays out: (assign, best, nhits)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        assign = np.empty(n, dtype=np.int32)
        best = np.zeros(n, dtype=HIT_DTYPE)
        nhits = np.zeros(n, dtype=np.int32)
        check(lib().mnc_classify_batch(self._h, bases.ctypes.data, offsets.ctypes.data, n, min_mapq,
                                       assign.ctypes.data, best.ctypes.data, nhits.ctypes.data))
        self.n_reads = n
        return assign, best, nhits

    def prefetch_ptr(self, bases_ptr, offsets_ptr, n):
        """Start the H2D copy of the NEXT batch (same pointers as its classify_ptr call will pass) behind the kernels
        of the one being classified.  False: a prefetched batch is still waiting for its call; nothing was done."""
        started = C.c_int(0)
        check(lib().mnc_engine_prefetch(self._h, bases_ptr, offsets_ptr, n, C.byref(started)))
        return bool(started.value)

    def prefetch_cancel(self):
        """Forget an announced batch that will not be classified (its host arrays may be reused afterwards)."""
        check(lib().mnc_engine_prefetch_cancel(self._h))

    def classify_ptr(self, bases_ptr, offsets_ptr, n, min_mapq=60):
        """As classify(), on caller-owned host buffers given by address (e.g. a FastqReader batch)."""
        assign = np.empty(n, dtype=np.int32)
        best = np.zeros(n, dtype=HIT_DTYPE)
        nhits = np.zeros(n, dtype=np.int32)
        check(lib().mnc_classify_batch(self._h, bases_ptr, offsets_ptr, n, min_mapq,
                                       assign.ctypes.data, best.ctypes.data, nhits.ctypes.data))
        self.n_reads = n
        return assign, best, nhits

    def classify_device(self, d_bases, d_offsets, n_reads, total_bases, max_read_len, min_mapq,
                        d_assign, d_best=0, d_nhits=0, d_counts=0):
        """All arguments are raw device pointers (ints); asynchronous on the engine stream."""
        check(lib().mnc_classify_device(self._h, d_bases, d_offsets, n_reads, total_bases, max_read_len,
                                        min_mapq, d_assign, d_best or None, d_nhits or None,
                                        d_counts or None))
        self.n_reads = n_reads

    def sync(self):
        check(lib().mnc_engine_sync(self._h))

    def fetch_hits(self):
        """Gated hit lists of the last batch as CSR (offsets[n+1], hits)."""
        n = C.c_int64(0)
        off = np.zeros(self.n_reads + 1, dtype=np.int64)
        rc = lib().mnc_engine_fetch_hits(self._h, None, None, 0, C.byref(n))
        if rc not in (OK, ERR_RANGE):
            check(rc)
        hits = np.zeros(max(n.value, 1), dtype=HIT_DTYPE)
        check(lib().mnc_engine_fetch_hits(self._h, off.ctypes.data, hits.ctypes.data, len(hits), C.byref(n)))
        return off, hits[:n.value]

    def export_alignments(self, cs=False, MD=False):
        """`mnc_engine_export_alignments`: build the records (and cs / MD) of the last batch in HBM; returns the four
        sizes (records, CIGAR words, cs bytes, MD bytes).  The pools stay on the device until the next classify / export."""
        n = [C.c_int64(0) for _ in range(4)]
        check(lib().mnc_engine_export_alignments(self._h, (ALN_CS if cs else 0) | (ALN_MD if MD else 0), *[C.byref(x) for x in n]))
        return tuple(int(x.value) for x in n)

    def fetch_alignments(self, sizes):
        """`mnc_engine_fetch_alignments` into fresh arrays of exactly the exported sizes."""
        n_aln, n_cig, n_cs, n_md = sizes
        off = np.zeros(self.n_reads + 1, dtype=np.int64)
        alns = np.zeros(n_aln, dtype=ALN_DTYPE)
        cig = np.zeros(n_cig, dtype=np.uint32)
        cs = np.zeros(n_cs, dtype=np.uint8)
        md = np.zeros(n_md, dtype=np.uint8)
        check(lib().mnc_engine_fetch_alignments(self._h, off.ctypes.data, alns.ctypes.data if n_aln else None, n_aln,
                                                cig.ctypes.data if n_cig else None, n_cig, cs.ctypes.data if n_cs else None, n_cs,
                                                md.ctypes.data if n_md else None, n_md))
        return off, alns, cig, cs, md

    def alignments(self, cs=False, MD=False):
        """Everything `index.map()` yields for the last batch, as flat arrays: (offsets[n_reads + 1], records (ALN_DTYPE),
        cigar words (len << 4 | op), cs bytes, md bytes).  Record i of read r: offsets[r] <= i < offsets[r + 1]; its CIGAR is
        cigar[cigar_off : cigar_off + n_cigar], its strings cs[cs_off : cs_off + cs_len] / md[md_off : md_off + md_len]."""
        return self.fetch_alignments(self.export_alignments(cs, MD))

    def alignments_device(self):
        """Device addresses (ints, 0 for an empty pool) of the exported pools: (offsets, records, cigar, cs, md)."""
        p = [C.c_void_p() for _ in range(5)]
        check(lib().mnc_engine_alignments_device(self._h, *[C.byref(x) for x in p]))
        return tuple(int(x.value or 0) for x in p)

    def export_ms(self):
        """Device time span of the last export (with profiling on)."""
        ms = C.c_double(0)
        check(lib().mnc_engine_export_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def add_coverage(self, cov, what=COV_ASSIGNED):
        """`mnc_engine_add_coverage`: add the last classified batch, as it stands in HBM, to the accumulator `cov`.
        `what` is one of COV_GATED / COV_PRIMARY / COV_ALL / COV_ASSIGNED, optionally | COV_SPAN.  Asynchronous."""
        self._add("mnc_engine_add_coverage", cov, int(what))

    def add_pileup(self, pileup, what=COV_GATED):
        """`mnc_engine_add_pileup`: add the last classified batch, as it stands in HBM, to the accumulator `pileup`.
        `what` is one of COV_GATED / COV_PRIMARY / COV_ALL / COV_ASSIGNED.  Asynchronous."""
        self._add("mnc_engine_add_pileup", pileup, int(what))

    def add_abundance(self, abundance):
        """`mnc_engine_add_abundance`: add the candidate genomes of every read of the last classified batch, as it stands in
        HBM, to the accumulator `abundance`.  Asynchronous."""
        self._add("mnc_engine_add_abundance", abundance)

    def carry_candidates(self, carry, first_read, genome_offset):
        """`mnc_engine_carry_candidates`: merge the candidate genomes of every read of the last classified batch into the
        rows `first_read ..` of `carry`; genome g of this engine's index is genome `genome_offset` + g there.  Asynchronous."""
        self._add("mnc_engine_carry_candidates", carry, int(first_read), int(genome_offset))

    def _add(self, symbol, acc, *args):
        check(getattr(lib(), symbol)(self._h, acc._h if acc is not None else None, *args))

    def set_profiling(self, on=True):
        check(lib().mnc_engine_set_profiling(self._h, 1 if on else 0))

    def set_contract(self, contract):
        """CONTRACT_DP (default): base-level alignment as mappy runs it; CONTRACT_CHAIN: stop after chaining."""
        check(lib().mnc_engine_set_contract(self._h, int(contract)))

    def set_long_reads(self, on=True):
        """Reads of 2^20 .. MAX_READ_LEN_WIDE bases are classified (a second, wide pass over them) instead of coming
        back SKIPPED.  Off by default."""
        check(lib().mnc_engine_set_long_reads(self._h, 1 if on else 0))

    def cigars(self):
        """CIGARs [(len, op), ...] of the regions of the last batch, in DUMP_REGS order."""
        regs = self.dump(DUMP_REGS, REG_DTYPE)
        words = self.dump(DUMP_CIGARS, np.uint32)
        out, k = [], 0
        for r in regs:
            n = int(r["n_cigar"])
            out.append([(int(c) >> 4, "MID"[int(c) & 0xf]) for c in words[k:k + n]])
            k += n
        return out

    def set_debug(self, mode=1):
        """mode 2 = stress build of the chaining kernel (every look-back through HBM)."""
        check(lib().mnc_engine_set_debug(self._h, int(mode)))

    def dump_tables(self):
        """The device tables of this engine's index as bytes (test hook)."""
        n = C.c_int64(0)
        rc = lib().mnc_engine_dump_tables(self._h, None, 0, C.byref(n))
        if rc not in (OK, ERR_RANGE):
            check(rc)
        buf = np.zeros(n.value, dtype=np.uint8)
        check(lib().mnc_engine_dump_tables(self._h, buf.ctypes.data, len(buf), C.byref(n)))
        return buf

    def timings(self, reset=False):
        ms = np.zeros(N_STAGES, dtype=np.float64)
        ln = np.zeros(N_STAGES, dtype=np.int64)
        check(lib().mnc_engine_get_timings(self._h, ms.ctypes.data, ln.ctypes.data, 1 if reset else 0))
        names = [lib().mnc_stage_name(s).decode() for s in range(N_STAGES)]
        return {names[s]: (float(ms[s]), int(ln[s])) for s in range(N_STAGES)}

    def counters(self):
        c = np.zeros(24, dtype=np.int64)
        check(lib().mnc_engine_get_counters(self._h, c.ctypes.data, 24))
        keys = ["minimizers", "probe_hits", "anchors", "chains", "regions", "gated_hits", "ambiguous_reads", "batch_redone",
                "dp_segments", "dp_fill_tier1", "dp_fill_tier2", "dp_fill_handed_back",
                "dp_fill_steps_t1", "dp_fill_steps_t2", "dp_fill_steps_t3", "dp_ext_cell_steps",
                "dp_literal_big", "dp_literal_mid", "dp_long_gaps", "dp_literal_big_handed_back", "dp_long_extensions", "dp_fill_tier3",
                "dp_fill_tier_mid", "dp_fill_steps_tm"]
        return dict(zip(keys, (int(x) for x in c)))

    def dump(self, what, dtype):
        n = C.c_int64(0)
        rc = lib().mnc_engine_dump(self._h, what, None, 0, C.byref(n))
        if rc not in (OK, ERR_RANGE):
            check(rc)
        buf = np.zeros(max(n.value, 1), dtype=np.uint8)
        check(lib().mnc_engine_dump(self._h, what, buf.ctypes.data, len(buf), C.byref(n)))
        return buf[:n.value].view(dtype).copy()


# ---------------------------------------------------------------------------------- the accumulators
class _Accumulator:
    """What the owners of the accumulator handles share: ``mnc_<_c>_create`` / ``_reset`` / ``_device_bytes`` / ``_free``."""

    _c = None                                                   # "coverage", "pileup", "abundance"

    def _create(self, index, device, *args):
        h = C.c_void_p()
        check(getattr(lib(), f"mnc_{self._c}_create")(index._h if index is not None else None, int(device), *args, C.byref(h)))
        self._h = h

    def reset(self):
        check(getattr(lib(), f"mnc_{self._c}_reset")(self._h))

    def device_bytes(self):
        n = C.c_int64(0)
        check(getattr(lib(), f"mnc_{self._c}_device_bytes")(self._h, C.byref(n)))
        return int(n.value)

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), f"mnc_{self._c}_free")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------- coverage
class Coverage(_Accumulator):
    """Owner of an ``mnc_coverage``: depth of coverage over every reference base of one index on one device, accumulated
    from batch to batch by `Engine.add_coverage` (include/monica_amd.h, "coverage")."""

    _c = "coverage"

    def __init__(self, index, device=0, bin_bases=1024):
        self.index = index
        self.device = device
        self.bin_bases = int(bin_bases)
        self._create(index, device, self.bin_bases)

    def summary(self):
        """One row per contig (COV_SUMMARY_DTYPE): covered bases, depth sum, maximal depth, records added.  Waits for the
        adds queued so far; the accumulator stays as it is."""
        n = len(self.index.contig_lens)
        cov, dsum, nal = (np.zeros(n, dtype=np.int64) for _ in range(3))
        mx = np.zeros(n, dtype=np.int32)
        check(lib().mnc_coverage_summary(self._h, cov.ctypes.data, dsum.ctypes.data, mx.ctypes.data, nal.ctypes.data))
        out = np.zeros(n, dtype=COV_SUMMARY_DTYPE)
        out["covered"], out["depth_sum"], out["max_depth"], out["n_aln"] = cov, dsum, mx, nal
        return out

    def bins(self, rid):
        """The profile of contig `rid`: (covered bases int32[n_bins], depth sum int64[n_bins]) per bin of `bin_bases`."""
        n = C.c_int64(0)
        rc = lib().mnc_coverage_fetch_bins(self._h, int(rid), None, None, 0, C.byref(n))
        if rc not in (OK, ERR_RANGE):
            check(rc)
        cov = np.zeros(n.value, dtype=np.int32)
        dsum = np.zeros(n.value, dtype=np.int64)
        check(lib().mnc_coverage_fetch_bins(self._h, int(rid), cov.ctypes.data, dsum.ctypes.data, len(cov), C.byref(n)))
        return cov, dsum

    def depth(self, rid, start=0, end=None):
        """Per-base depth of bases [start, end) of contig `rid` (int32)."""
        end = (self.index.contig_lens[rid] if 0 <= rid < len(self.index.contig_lens) else 0) if end is None else int(end)
        out = np.zeros(max(end - int(start), 0), dtype=np.int32)
        check(lib().mnc_coverage_fetch_depth(self._h, int(rid), int(start), end, out.ctypes.data if len(out) else None))
        return out

    def device_track(self):
        """(device address of the raw difference track, words): `mnc_coverage_device`."""
        p, n = C.c_void_p(), C.c_int64(0)
        check(lib().mnc_coverage_device(self._h, C.byref(p), C.byref(n)))
        return int(p.value or 0), int(n.value)


# ---------------------------------------------------------------------------------- pileup
class Pileup(_Accumulator):
    """Owner of an ``mnc_pileup``: what the reads say at every reference base of one index on one device -- depth, the
    counts of A C G T N, deletions and insertions -- accumulated from batch to batch by `Engine.add_pileup`
    (include/monica_amd.h, "pileup")."""

    _c = "pileup"

    def __init__(self, index, device=0):
        self.index = index
        self._device = device                                   # (`device` is the method below)
        self._create(index, device)

    def _end(self, rid, end):
        return (self.index.contig_lens[rid] if 0 <= rid < len(self.index.contig_lens) else 0) if end is None else int(end)

    def counts(self, rid, start=0, end=None):
        """The eight planes (PILE_PLANES) of bases [start, end) of contig `rid`: int32[8, end - start]."""
        end = self._end(rid, end)
        out = np.zeros((len(PILE_PLANES), max(end - int(start), 0)), dtype=np.int32)
        check(lib().mnc_pileup_fetch_counts(self._h, int(rid), int(start), end, out.ctypes.data if out.size else None))
        return out

    def variants(self, rid=-1, min_depth=1, min_count=1, min_permille=0):
        """The called variants (VARIANT_DTYPE) of contig `rid`, or of every contig for -1, in (rid, pos, allele) order."""
        n = C.c_int64(0)
        args = (int(rid), int(min_depth), int(min_count), int(min_permille))
        rc = lib().mnc_pileup_call_variants(self._h, *args, None, 0, C.byref(n))
        if rc not in (OK, ERR_RANGE):
            check(rc)
        out = np.zeros(n.value, dtype=VARIANT_DTYPE)
        if len(out):
            check(lib().mnc_pileup_call_variants(self._h, *args, out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value]

    def consensus(self, rid, start=0, end=None, min_depth=1):
        """One byte per base of [start, end) of contig `rid`: A C G T, '-' (deleted) or N (span < min_depth)."""
        end = self._end(rid, end)
        out = np.zeros(max(end - int(start), 0), dtype=np.uint8)
        check(lib().mnc_pileup_consensus(self._h, int(rid), int(start), end, int(min_depth), out.ctypes.data if len(out) else None))
        return out.tobytes()

    def device(self):
        """(device address of the depth differences, of the seven alt planes, words per plane): `mnc_pileup_device`."""
        d, a, n = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        check(lib().mnc_pileup_device(self._h, C.byref(d), C.byref(a), C.byref(n)))
        return int(d.value or 0), int(a.value or 0), int(n.value)


# ---------------------------------------------------------------------------------- abundance
# Abundance(): the defaults of the Python layer (include/monica_amd.h, "abundance": the weights)
ABUNDANCE_MAX_DELTA, ABUNDANCE_SCALE_Q = 80, 3
ABUNDANCE_CAP_CANDS = 1 << 22           # candidate slots when the caller names none: 48 MiB of HBM
ABUNDANCE_TOL_Q32 = 1 << 22             # solve(): stop once no genome's expected reads move by more than 2^-10 of a read
ABUNDANCE_MAX_PRODUCT = 4000            # max_delta * scale_q at most: every weight a normal double


class Abundance(_Accumulator):
    """Owner of an ``mnc_abundance``: per read the genomes that fit it about as well as its best one, accumulated from
    batch to batch by `Engine.add_abundance`, and the EM over them (include/monica_amd.h, "abundance")."""

    _c = "abundance"

    def __init__(self, index, device=0, cap_cands=ABUNDANCE_CAP_CANDS, max_delta=ABUNDANCE_MAX_DELTA, scale_q=ABUNDANCE_SCALE_Q, n_genomes=None):
        cap_cands, max_delta, scale_q = int(cap_cands), int(max_delta), int(scale_q)
        if cap_cands < 0:
            raise ValueError(f"cap_cands = {cap_cands}: a number of candidate slots")
        if max_delta < 0 or scale_q < 1 or max_delta * scale_q > ABUNDANCE_MAX_PRODUCT:
            raise ValueError(f"max_delta = {max_delta}, scale_q = {scale_q}: max_delta >= 0, scale_q >= 1 and "
                             f"max_delta * scale_q <= {ABUNDANCE_MAX_PRODUCT} are required")
        self.index = index
        self.device = device
        self.cap_cands, self.max_delta, self.scale_q = cap_cands, max_delta, scale_q
        self.n_genomes = len(index.genome_names) if index is not None else 0
        self.genome_names = list(index.genome_names) if index is not None else []
        if n_genomes is None:
            self._create(index, device, cap_cands, max_delta, scale_q)
            return
        # for the genomes of a whole database, of no index: `global_`
        if index is not None or int(n_genomes) < 0:
            raise ValueError(f"n_genomes = {n_genomes}: a number of genomes, and no index beside it")
        self.n_genomes = int(n_genomes)
        h = C.c_void_p()
        check(lib().mnc_abundance_create_global(int(device), self.n_genomes, cap_cands, max_delta, scale_q, C.byref(h)))
        self._h = h

    @classmethod
    def global_(cls, device, n_genomes, cap_cands=ABUNDANCE_CAP_CANDS, max_delta=ABUNDANCE_MAX_DELTA, scale_q=ABUNDANCE_SCALE_Q, genome_names=None):
        """`mnc_abundance_create_global`: an accumulator for `n_genomes` genomes that is tied to no index -- the genomes of a
        database of several parts, in part order.  It is added to by `add_carry` and `add_lists`; `Engine.add_abundance`
        refuses it.  `genome_names` (optional) is kept for whoever writes the result out."""
        ab = cls(None, device, cap_cands, max_delta, scale_q, n_genomes=n_genomes)
        if genome_names is not None:
            if len(genome_names) != ab.n_genomes:
                ab.close()
                raise ValueError(f"{len(genome_names)} genome names for {ab.n_genomes} genomes")
            ab.genome_names = list(genome_names)
        return ab

    def add_carry(self, carry, first_read=0, n_reads=None):
        """`mnc_abundance_add_carry`: rows `first_read .. first_read + n_reads - 1` of the candidate carry `carry` (default: to
        its end), each as one read.  The carry is left as it is."""
        if n_reads is None:
            n_reads = carry.info()["cap_reads"] - int(first_read)
        check(lib().mnc_abundance_add_carry(self._h, carry._h if carry is not None else None, int(first_read), int(n_reads)))

    def add_lists(self, offsets, genome, delta):
        """Rows made by the caller: row r is (genome, delta)[offsets[r]:offsets[r + 1]], genome ids ascending.  A row of one
        candidate counts as a unique read, a longer one is stored."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        genome = np.ascontiguousarray(genome, dtype=np.int32)
        delta = np.ascontiguousarray(delta, dtype=np.int32)
        if offsets.ndim != 1 or len(offsets) < 1 or len(genome) != len(delta) or (len(offsets) > 1 and int(offsets[-1]) > len(genome)):
            raise ValueError("offsets holds n_reads + 1 entries into genome / delta, which have one length")
        check(lib().mnc_abundance_add_lists(self._h, len(offsets) - 1, offsets.ctypes.data, genome.ctypes.data if len(genome) else None,
                                            delta.ctypes.data if len(delta) else None))

    def info(self):
        """{"n_reads", "n_stored_reads", "n_cands", "n_dropped"} as they stand (waits for the adds queued so far)."""
        v = [C.c_int64(0) for _ in range(4)]
        check(lib().mnc_abundance_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("n_reads", "n_stored_reads", "n_cands", "n_dropped"), (int(x.value) for x in v)))

    def unique(self):
        """int64[G]: the reads with exactly one candidate genome."""
        out = np.zeros(self.n_genomes, dtype=np.int64)
        check(lib().mnc_abundance_fetch_unique(self._h, out.ctypes.data if len(out) else None))
        return out

    def lists(self):
        """The stored rows, sorted lexicographically by their (genome, delta) sequence: (offsets int64[n + 1], genome
        int32, delta int32)."""
        inf = self.info()
        off = np.zeros(inf["n_stored_reads"] + 1, dtype=np.int64)
        gen = np.zeros(inf["n_cands"], dtype=np.int32)
        dlt = np.zeros(inf["n_cands"], dtype=np.int32)
        check(lib().mnc_abundance_fetch_lists(self._h, off.ctypes.data, gen.ctypes.data if len(gen) else None, dlt.ctypes.data if len(dlt) else None,
                                              len(off) - 1, len(gen)))
        return off, gen, dlt

    def solve(self, max_iter=200, tol_q32=ABUNDANCE_TOL_Q32):
        """The EM: (theta float64[G], expected reads float64[G], iterations run).  Exact and reproducible; MncError
        (ERR_RANGE) while rows have been dropped."""
        theta = np.zeros(self.n_genomes, dtype=np.float64)
        expected = np.zeros(self.n_genomes, dtype=np.float64)
        iters = C.c_int32(0)
        check(lib().mnc_abundance_solve(self._h, int(max_iter), int(tol_q32), theta.ctypes.data if len(theta) else None,
                                        expected.ctypes.data if len(expected) else None, C.byref(iters)))
        return theta, expected, int(iters.value)

    def device_arrays(self):
        """Device addresses (ints) of unique, the CSR's offsets, genome and delta as stored: `mnc_abundance_device`."""
        p = [C.c_void_p() for _ in range(4)]
        check(lib().mnc_abundance_device(self._h, *[C.byref(x) for x in p]))
        return tuple(int(x.value or 0) for x in p)


# ---------------------------------------------------------------------------------- candidate carry
CARRY_WIDTH = 16                        # pairs per read when the caller names none: 136 bytes of HBM a read
CARRY_MAX_WIDTH = 64                    # a row lives in one wave, one pair per lane


class Carry(_Accumulator):
    """Owner of an ``mnc_carry``: one row per read of a sample -- the best score any index part has given the read and up
    to `width` (global genome id, score) pairs -- merged into from every part's batches by `Engine.carry_candidates` and
    handed to a global `Abundance` by `Abundance.add_carry` (include/monica_amd.h, "candidate carry").  It belongs to a
    device, not to an index."""

    _c = "carry"

    def __init__(self, device, cap_reads, width=CARRY_WIDTH, max_delta=ABUNDANCE_MAX_DELTA):
        cap_reads, width, max_delta = int(cap_reads), int(width), int(max_delta)
        if cap_reads < 0:
            raise ValueError(f"cap_reads = {cap_reads}: a number of reads")
        if not 1 <= width <= CARRY_MAX_WIDTH:
            raise ValueError(f"width = {width}: 1 .. {CARRY_MAX_WIDTH} pairs per read")
        if max_delta < 0:
            raise ValueError(f"max_delta = {max_delta}: max_delta >= 0 is required")
        self.device, self.width, self.max_delta = int(device), width, max_delta
        h = C.c_void_p()
        check(lib().mnc_carry_create(self.device, cap_reads, width, max_delta, C.byref(h)))
        self._h = h

    def reserve(self, n_reads):
        """Grow to at least `n_reads` rows; contents kept, new rows empty."""
        check(lib().mnc_carry_reserve(self._h, int(n_reads)))

    def info(self):
        """{"cap_reads", "n_rows_used", "n_cands", "n_truncated_reads"} as they stand (waits for the merges queued so far)."""
        v = [C.c_int64(0) for _ in range(4)]
        check(lib().mnc_carry_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("cap_reads", "n_rows_used", "n_cands", "n_truncated_reads"), (int(x.value) for x in v)))

    def fetch(self, first_read=0, n_reads=None):
        """Rows `first_read .. first_read + n_reads - 1` (default: to the end): (count int32[n], best int32[n], genome
        int32[n, width], score int32[n, width]); a row's pairs in ascending genome id, unused places -1 / 0."""
        if n_reads is None:
            n_reads = self.info()["cap_reads"] - int(first_read)
        n = max(int(n_reads), 0)
        count, best = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        genome, score = np.zeros((n, self.width), dtype=np.int32), np.zeros((n, self.width), dtype=np.int32)
        check(lib().mnc_carry_fetch(self._h, int(first_read), int(n_reads), *[a.ctypes.data if a.size else None for a in (count, best, genome, score)]))
        return count, best, genome, score

    def add_lists(self, first_read, offsets, genome, score):
        """Rows made by the caller: row r is (genome, score)[offsets[r]:offsets[r + 1]], global genome ids ascending, merged
        into read `first_read` + r by the carry's rule."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        genome = np.ascontiguousarray(genome, dtype=np.int32)
        score = np.ascontiguousarray(score, dtype=np.int32)
        if offsets.ndim != 1 or len(offsets) < 1 or len(genome) != len(score) or (len(offsets) > 1 and int(offsets[-1]) > len(genome)):
            raise ValueError("offsets holds n_reads + 1 entries into genome / score, which have one length")
        check(lib().mnc_carry_add_lists(self._h, int(first_read), len(offsets) - 1, offsets.ctypes.data, genome.ctypes.data if len(genome) else None,
                                        score.ctypes.data if len(score) else None))

    def merge(self, src):
        """`mnc_carry_merge`: the rows of `src` merged into this carry's, row for row; `src` is left as it is."""
        check(lib().mnc_carry_merge(self._h, src._h if src is not None else None))

    def device_rows(self):
        """(device address of the heads, of the slots, cap_reads, width): `mnc_carry_device`."""
        h, s, n, w = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int32(0)
        check(lib().mnc_carry_device(self._h, C.byref(h), C.byref(s), C.byref(n), C.byref(w)))
        return int(h.value or 0), int(s.value or 0), int(n.value), int(w.value)


# ---------------------------------------------------------------------------------- host helpers
def best_hit(hits):
    """Exact-integer restatement of aligner.best_hit over (nm, mlen) pairs -> index or -1."""
    arr = np.zeros(len(hits), dtype=HIT_DTYPE)
    for i, (nm, mlen) in enumerate(hits):
        arr[i]["nm"], arr[i]["mlen"] = nm, mlen
    out = C.c_int(0)
    check(lib().mnc_best_hit(arr.ctypes.data, len(hits), C.byref(out)))
    return out.value


def counts(index, assign, best, offsets, mode):
    """Host accumulation of aligner.py:247-263 into an int64[n_genomes] vector."""
    assign = np.ascontiguousarray(assign, dtype=np.int32)
    best = np.ascontiguousarray(best, dtype=HIT_DTYPE)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    out = np.zeros(len(index.genome_names), dtype=np.int64)
    check(lib().mnc_counts(index._h, assign.ctypes.data, best.ctypes.data, offsets.ctypes.data,
                           len(assign), mode, out.ctypes.data))
    return out


# ---------------------------------------------------------------------------------- FASTQ + carried hits
TO_UNMAPPED, TO_AMBIGUOUS, TO_MAPPED, TO_FOCUS = 1, 2, 4, 8


class FastqReader:
    """Batches of a FASTQ file as flat arrays held by the library (``mnc_fastq``).  A malformed
    file raises ValueError with Biopython's message, as SeqIO.parse would."""

    def __init__(self, path, _handle=None, _n=0):
        if _handle is not None:                     # a detached batch (see detach)
            self._h, self.n = _handle, _n
            return
        h = C.c_void_p()
        check(lib().mnc_fastq_open(_b(path), C.byref(h)))
        self._h = h
        self.n = 0

    def remaining(self):
        """Bytes of the file that no batch has taken yet (-1 when unknown)."""
        n = C.c_int64(-1)
        check(lib().mnc_fastq_remaining(self._h, C.byref(n)))
        return n.value

    def detach(self):
        """The current batch as an object of its own; this reader goes on with the next batch in fresh
        arrays.  The detached batch has the reader's accessors, `route`, and is what HitMap.update takes."""
        h = C.c_void_p()
        check(lib().mnc_fastq_detach_batch(self._h, C.byref(h)))
        out = FastqReader(None, _handle=h, _n=self.n)
        self.n = 0
        return out

    def next(self, max_reads=100_000, max_bases=1 << 29):
        n = C.c_uint32(0)
        rc = lib().mnc_fastq_next(self._h, max_reads, max_bases, C.byref(n))
        if rc == ERR_FORMAT:
            raise ValueError(lib().mnc_last_error().decode(errors="replace"))
        check(rc)
        self.n = n.value
        return self.n

    @property
    def bases_ptr(self):
        return lib().mnc_fastq_bases(self._h)

    @property
    def offsets_ptr(self):
        return lib().mnc_fastq_offsets(self._h)

    def offsets(self):
        """int64[n + 1] view, valid until the next batch."""
        return np.ctypeslib.as_array(C.cast(self.offsets_ptr, C.POINTER(C.c_int64)), shape=(self.n + 1,))

    def bases(self):
        total = int(self.offsets()[-1])
        if total == 0:
            return np.zeros(0, dtype=np.uint8)
        return np.ctypeslib.as_array(C.cast(self.bases_ptr, C.POINTER(C.c_uint8)), shape=(total,))

    def quals(self):
        total = int(self.offsets()[-1])
        if total == 0:
            return np.zeros(0, dtype=np.uint8)
        return np.ctypeslib.as_array(C.cast(lib().mnc_fastq_quals(self._h), C.POINTER(C.c_uint8)), shape=(total,))

    def title(self, r):
        p, ln, idl = C.c_void_p(), C.c_uint32(0), C.c_uint32(0)
        check(lib().mnc_fastq_title(self._h, r, C.byref(p), C.byref(ln), C.byref(idl)))
        return C.string_at(p.value, ln.value).decode(errors="replace") if ln.value else ""

    def route(self, dest, label=None, labels=(), paths=(None, None, None, None)):
        """Append the batch's records to paths = (unmapped, ambiguous, mapped, focus) by dest bits."""
        dest = np.ascontiguousarray(dest, dtype=np.uint8)
        assert len(dest) == self.n
        lab = np.ascontiguousarray(label, dtype=np.int32) if label is not None else None
        bl = [_b(x) for x in labels]
        al = (C.c_char_p * max(len(bl), 1))(*bl)
        ap = (C.c_char_p * 4)(*[(_b(x) if x is not None else None) for x in paths])
        check(lib().mnc_fastq_route(self._h, dest.ctypes.data, lab.ctypes.data if lab is not None else None,
                                    al, len(bl), ap))

    def write_paf(self, index, offsets, records, path, cigar=None, cs=None, md=None, primary_only=False):
        """Append one PAF line per alignment record of this batch (`Engine.alignments()` of its classify call) to `path`;
        cg:Z: / cs:Z: / MD:Z: for each pool given."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        records = np.ascontiguousarray(records, dtype=ALN_DTYPE)
        assert len(offsets) == self.n + 1 and int(offsets[-1]) <= len(records)
        pools = [None if p is None else np.ascontiguousarray(p, dtype=t) for p, t in ((cigar, np.uint32), (cs, np.uint8), (md, np.uint8))]
        keep = [np.zeros(1, dtype=p.dtype) if p is not None and p.size == 0 else p for p in pools]     # an empty pool is still "given"
        check(lib().mnc_fastq_write_paf(self._h, index._h, offsets.ctypes.data, records.ctypes.data if len(records) else None,
                                        *[(p.ctypes.data if p is not None else None) for p in keep],
                                        PAF_PRIMARY_ONLY if primary_only else 0, _b(path)))

    def close(self):
        if getattr(self, "_h", None):
            lib().mnc_fastq_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HitMap:
    """`sample_hits` of the reference as per-id summaries (``mnc_hitmap``)."""

    def __init__(self, path=None):
        h = C.c_void_p()
        if path is None:
            check(lib().mnc_hitmap_create(C.byref(h)))
        else:
            check(lib().mnc_hitmap_load(_b(path), C.byref(h)))
        self._h = h

    def save(self, path):
        check(lib().mnc_hitmap_save(self._h, _b(path)))

    def __len__(self):
        return int(lib().mnc_hitmap_size(self._h))

    def update(self, reader, index, assign, best, nhits):
        """Extend every read's list by this part's hits; returns int32[n, 5] =
        {hits, nm, mlen, name id, tied} of the lists as they stand."""
        out = np.zeros((reader.n, 5), dtype=np.int32)
        assign = np.ascontiguousarray(assign, dtype=np.int32)
        best = np.ascontiguousarray(best, dtype=HIT_DTYPE)
        nhits = np.ascontiguousarray(nhits, dtype=np.int32)
        check(lib().mnc_hitmap_update(self._h, reader._h, index._h, assign.ctypes.data, best.ctypes.data,
                                      nhits.ctypes.data, out.ctypes.data))
        return out

    def names(self):
        L = lib()
        return [L.mnc_hitmap_name(self._h, i).decode() for i in range(L.mnc_hitmap_n_names(self._h))]

    def close(self):
        if getattr(self, "_h", None):
            lib().mnc_hitmap_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
