/*
 * monica_amd.h -- C-ABI of the MI355X-native read-classification engine.
 *
 * This is the drop-in boundary for monica's aligner hot path.  In the reference the
 * boundary is the Python->C crossing into mappy (minimap2 2.17) at
 *   monica/genomes/aligner.py:45-46   mappy.Aligner(fn_idx_in=<fasta.gz>, preset='map-ont',
 *                                                   best_n=15, fn_idx_out=<index file>)
 *   monica/genomes/aligner.py:59      mappy.Aligner(fn_idx_in=<index file>)
 *   monica/genomes/aligner.py:193,215 index.map(str(seq_record.seq)) -> hits
 *                                     (.is_primary .mapq .ctg .NM .mlen, lines 194-195, 216-217)
 * and the per-read Python that consumes the hits (aligner.py:218-263, 328-339).
 * Each entry point below names the reference interface it replaces.
 *
 * Conventions: every function returns MNC_OK (0) or a negative MNC_ERR_* code and never
 * throws or aborts across the ABI.  Handles are opaque.  The library never keeps a caller
 * pointer past the call.  An mnc_index is immutable after build/load/upload and may be
 * shared by any number of engines and threads; an mnc_engine (stream + HBM workspace)
 * must be used by one thread at a time.
 *
 * There is no CPU execution path in this library: classification entry points fail with
 * MNC_ERR_NODEVICE when no gfx950 device is present.
 */
#ifndef MONICA_AMD_H
#define MONICA_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MNC_OK               0
#define MNC_ERR_ARG         (-1)   /* bad argument                                        */
#define MNC_ERR_IO          (-2)   /* file cannot be opened / read / written               */
#define MNC_ERR_FORMAT      (-3)   /* damaged or empty index / FASTA                       */
#define MNC_ERR_NOMEM       (-4)   /* host or device allocation failed                     */
#define MNC_ERR_HIP         (-5)   /* HIP runtime error (see mnc_last_error())             */
#define MNC_ERR_NODEVICE    (-6)   /* no usable gfx950 device                              */
#define MNC_ERR_UNSUPPORTED (-7)   /* parameter outside what the kernels implement         */
#define MNC_ERR_RANGE       (-8)   /* caller buffer too small; required size is reported   */

/* per-read decision codes in out_assign[] (aligner.py:218-233, 264-265) */
#define MNC_UNMAPPED   (-1)        /* no gated hit        -> unmapped/<sample>             */
#define MNC_AMBIGUOUS  (-2)        /* best_hit() returned 0 -> ambiguous/<sample>          */
#define MNC_SKIPPED    (-3)        /* the read is outside what the kernels hold (see "Limits" below): not classified; no
                                      gated hits.  index.map() has no such case (aligner.py:193, 215): the host side
                                      routes the read as unmapped and says so, the rest of its batch is unaffected      */

typedef struct mnc_index  mnc_index;
typedef struct mnc_engine mnc_engine;

/* one gated hit = the (ctg, NM, mlen) tuple of aligner.py:195,217 plus its mapq */
typedef struct {
	int32_t rid;    /* contig index; ctg = mnc_index_contig_name(rid) */
	int32_t mapq;
	int32_t nm;     /* hit.NM = blen - mlen + n_ambi after base-level alignment (blen - mlen of the
	                   chain under MNC_CONTRACT_CHAIN) */
	int32_t mlen;
} mnc_hit_t;

typedef struct {
	int32_t k, w;
	int32_t n_contigs;
	int32_t n_genomes;      /* distinct contig names ("tax_unit:accession", database.py:59) */
	int32_t mid_occ;        /* occurrence cut-off derived from the index (mid_occ_frac 2e-4) */
	int32_t reserved;
	int64_t n_keys;         /* distinct minimizer hashes    */
	int64_t n_occ;          /* minimizer occurrences        */
	int64_t total_len;      /* sum of contig lengths        */
	int64_t table_slots;    /* HBM hash-table slots         */
	int64_t device_bytes;   /* bytes resident in HBM after upload (0 before) */
} mnc_index_info_t;

/* ---------------------------------------------------------------- errors */
const char *mnc_strerror(int code);
const char *mnc_last_error(void);          /* thread-local detail of the last failure */

/* ---------------------------------------------------------------- device */
int mnc_device_count(int *n);              /* counts devices without initialising them */
int mnc_device_name(int device, char *buf, size_t cap);
/* free / total HBM of a device: what the host side sizes its cache of resident index parts against
 * (the reference holds one part at a time, aligner.py:91-103; this library keeps parts resident
 * between the passes of monica's loop as long as they fit) */
int mnc_device_mem_info(int device, int64_t *free_bytes, int64_t *total_bytes);

/* ---------------------------------------------------------------- index: build / load
 * mnc_index_build      <- mappy.Aligner(fn_idx_in=fasta(.gz), preset='map-ont', best_n=15,
 *                         fn_idx_out=out_path)                      aligner.py:45-46
 *                         out_path may be NULL (no file written).  k=15,w=10 is 'map-ont'.
 * mnc_index_load       <- mappy.Aligner(fn_idx_in=index file)       aligner.py:59
 *                         a falsy Aligner maps to MNC_ERR_FORMAT ('Damaged or empty index').
 */
int  mnc_index_build(const char *fasta_path, const char *out_path, int k, int w, mnc_index **out);
int  mnc_index_build_mem(int n_seq, const char *const *names, const char *const *seqs,
                         const int64_t *lens, int k, int w, mnc_index **out);
/* The same two with the sketch and the sort on a device (contig pieces through the batch sketch kernel, radix sort,
 * run lengths; csrc/k_idxbuild.hip): the same index, array for array, in a fraction of the time.  gz decompression and
 * the 4-bit packing of the contig bases stay on the host. */
int  mnc_index_build_device(const char *fasta_path, const char *out_path, int k, int w, int device, mnc_index **out);
int  mnc_index_build_mem_device(int n_seq, const char *const *names, const char *const *seqs,
                                const int64_t *lens, int k, int w, int device, mnc_index **out);
int  mnc_index_save(const mnc_index *idx, const char *path);
int  mnc_index_load(const char *path, mnc_index **out);
/* minimap2's own index format ("MMI\2", what mappy writes at aligner.py:45-46): mnc_index_load reads either format;
 * this writes it, so that an index built here can be handed to mappy / minimap2 as well */
int  mnc_index_save_mmi(const mnc_index *idx, const char *path);
void mnc_index_free(mnc_index *idx);
int  mnc_index_info(const mnc_index *idx, mnc_index_info_t *info);
const char *mnc_index_contig_name(const mnc_index *idx, int rid);      /* hit.ctg, aligner.py:195 */
int64_t     mnc_index_contig_len(const mnc_index *idx, int rid);
int         mnc_index_contig_genome(const mnc_index *idx, int rid);    /* contig -> genome id     */
const char *mnc_index_genome_name(const mnc_index *idx, int gid);      /* "tax_unit:accession"    */
int64_t     mnc_index_genome_len(const mnc_index *idx, int gid);       /* database.py:57-65 sum   */
/* dump (hash, y) pairs sorted by (hash, y); for tests.  *n receives the pair count. */
int  mnc_index_dump(const mnc_index *idx, uint64_t *hash, uint64_t *y, int64_t cap, int64_t *n);
/* override the occurrence cut-off (index shards of one logical index share one value) */
int  mnc_index_set_mid_occ(mnc_index *idx, int mid_occ);

/* ---------------------------------------------------------------- engine
 * One engine = one HIP stream + a growable HBM workspace on `device`.  The first engine
 * created for an index on a device uploads the index tables to that device's HBM.
 */
int  mnc_engine_create(mnc_index *idx, int device, mnc_engine **out);
/* What index.map() computes before monica's gate (aligner.py:193-195, 215-217):
 *   MNC_CONTRACT_DP     (default) minimap2's base-level alignment of every region, as mappy always
 *                       runs it (MM_F_CIGAR): mapq from dp_max / dp_max2 and identity, NM and
 *                       mlen from the CIGAR -- the values monica reads
 *   MNC_CONTRACT_CHAIN  stop after chaining: chain-level MAPQ, NM := blen - mlen of the chain
 *                       (the path BASELINE.json's north_star lists; ~10x faster, other numbers) */
#define MNC_CONTRACT_DP    0
#define MNC_CONTRACT_CHAIN 1
int  mnc_engine_set_contract(mnc_engine *eng, int contract);
/* Reads of 2^20 bases or more, which index.map() takes like any other (aligner.py:193, 215).  off (0, the default): such a
 * read comes back MNC_SKIPPED.  on (1): reads of up to MNC_MAX_READ_LEN_WIDE bases are classified.  In mnc_classify_batch
 * the reads below 2^20 bases take the usual pass, untouched by the others; the long ones take one more pass with
 * 24-bit query positions in the probe's records (an internal batch of those reads alone; at most MNC_MAX_READS_WIDE of
 * them per call), and the results are put back by read ordinal: out_assign / out_best / out_nhits, mnc_engine_fetch_hits
 * (one CSR over all reads, in read order) and mnc_engine_get_counters (sums of both passes) cover the whole call.  The
 * stage dumps (mnc_engine_dump) and timings after such a mixed call describe the wide pass -- the long reads, in their
 * order -- only; after a call whose reads are all long they describe the call in full. */
#define MNC_MAX_READ_LEN_WIDE ((1 << 24) - 1)
#define MNC_MAX_READS_WIDE    (1 << 16)
int  mnc_engine_set_long_reads(mnc_engine *eng, int on);
void mnc_engine_destroy(mnc_engine *eng);
/* another index part behind the same engine: `index = index_loader(part)` in the reference's loop over the
 * parts of a database (aligner.py:91-103).  Same k / w / match score as the index the engine was made for. */
int  mnc_engine_set_index(mnc_engine *eng, mnc_index *idx);
void *mnc_engine_stream(mnc_engine *eng);                              /* hipStream_t */
int  mnc_index_device_bytes(const mnc_index *idx, int device, int64_t *bytes); /* HBM the index holds on that one device */
int  mnc_engine_device_bytes(mnc_engine *eng, int64_t *bytes);         /* HBM held by the engine's own batch buffers */

/* ---------------------------------------------------------------- limits, and what happens at each
 *   k = 15, w = 10 only                          mnc_index_build*: MNC_ERR_UNSUPPORTED (the one setting monica uses,
 *                                                aligner.py:45: preset 'map-ont')
 *   a read of 2^20 bases or more                 mnc_classify_batch: that read alone comes back MNC_SKIPPED (no hits); the
 *   (default)                                    other reads of the batch are classified as ever.  mnc_classify_device
 *                                                (device-resident batches; the caller states max_read_len): MNC_ERR_UNSUPPORTED
 *   ... after mnc_engine_set_long_reads(eng, 1)  classified like any other read, up to MNC_MAX_READ_LEN_WIDE bases (exact; a
 *                                                second pass over those reads with wide probe records).  A longer read
 *                                                alone comes back MNC_SKIPPED; mnc_classify_device runs the whole call wide
 *                                                when max_read_len >= 2^20, with at most MNC_MAX_READS_WIDE reads, and
 *                                                answers MNC_ERR_UNSUPPORTED beyond either bound
 *   one kernel call of a read's alignment whose  that read alone comes back MNC_SKIPPED.  (tlen x qlen <= 1e8 with more
 *   direction matrix exceeds 256 MB              than 256 MB of direction bytes: a few hundred query bases against > 300 000
 *                                                target bases -- mm_align1 makes no such call with max_gap = 5 000)
 *   more than 2^20 reads in one call             MNC_ERR_UNSUPPORTED before anything runs (the probe's records hold a 20-bit
 *                                                read ordinal); monica_amd.aligner passes at most 100 000 per call
 *   2^40 bases or more in one call               MNC_ERR_UNSUPPORTED before anything runs
 *   reads with > 8 192 anchors or >= 65 536      exact; slower forms (sort in HBM, sequential backtrack, a wave per region
 *   bases                                        in the plan, bases read in place by the stitch kernel)
 *   a batch that outgrows a pool (query records, exact: the batch is redone with more room (mnc_engine_get_counters [7] counts
 *   segments, CIGAR words, region slots)         the passes); MNC_ERR_NOMEM when HBM itself is exhausted
 *   alignment records after a call that ran      mnc_engine_export_alignments: MNC_ERR_UNSUPPORTED (the engine holds the wide
 *   both the usual and the wide pass             pass alone); classify the two groups in separate calls.  A call whose reads
 *                                                are all long exports like any other
 *   cs / MD under MNC_CONTRACT_CHAIN             mnc_engine_export_alignments: MNC_ERR_ARG (no base-level alignment: records
 *                                                only, n_cigar = 0)
 *   coverage after a call that ran both the      mnc_engine_add_coverage: MNC_ERR_UNSUPPORTED, the accumulator untouched (the
 *   usual and the wide pass                      engine holds the wide pass alone); classify the two groups in separate calls
 *   coverage without MNC_COV_SPAN under          mnc_engine_add_coverage: MNC_ERR_ARG (no CIGAR to take the M columns from)
 *   MNC_CONTRACT_CHAIN
 *   a reference base overlapped by 2^31 or more  outside the contract: the depth track holds int32 (mnc_coverage_reset
 *   added records                                starts over)
 *   pileup after a call that ran both the usual  mnc_engine_add_pileup: MNC_ERR_UNSUPPORTED, the accumulator untouched (as for
 *   and the wide pass                            coverage); a call whose reads are all long adds like any other
 *   pileup under MNC_CONTRACT_CHAIN              mnc_engine_add_pileup: MNC_ERR_ARG (no CIGAR to take the columns from)
 *   the bases of an insertion                    inserted bases are not stored: mnc_pileup counts an insertion once, at the
 *                                                reference base on its left, whatever it inserts
 *   a reference base with 2^31 or more           outside the contract: every plane of mnc_pileup holds int32 per base
 *   observations in one pileup plane             (mnc_pileup_reset starts over)
 *   abundance after a call that ran both the     mnc_engine_add_abundance: MNC_ERR_UNSUPPORTED, the accumulator untouched (as for
 *   usual and the wide pass                      coverage); a call whose reads are all long adds like any other
 *   abundance under MNC_CONTRACT_CHAIN           mnc_engine_add_abundance: MNC_ERR_ARG (no dp_max to compare the genomes by)
 *   a candidate row beyond cap_cands             not stored and counted in n_dropped; mnc_abundance_solve: MNC_ERR_RANGE until
 *                                                mnc_abundance_reset
 *   a read that fits more than six genomes       sees six: a region list holds a primary and best_n = 5 secondaries
 *   carried candidates after a call that ran     mnc_engine_carry_candidates: MNC_ERR_UNSUPPORTED, the carry untouched (as for
 *   both the usual and the wide pass             mnc_engine_add_abundance); MNC_ERR_ARG under MNC_CONTRACT_CHAIN
 *   a read with more than `width` candidates     the `width` ranked highest stay (score descending, ties to the smaller genome
 *   within max_delta, over all parts             id); the read is counted in n_truncated_reads of mnc_carry_info
 */

/* ---------------------------------------------------------------- classify
 * mnc_classify_batch   <- the per-read loop body aligner.py:212-233 for one index part:
 *                         index.map(seq) -> gate `is_primary and mapq >= min_mapq`
 *                         -> single hit | best_hit(hits) | ambiguous.
 *   bases     host, concatenated read bases (ASCII; anything but ACGTUacgtu is ambiguous)
 *   offsets   host, n_reads+1 byte offsets into bases
 *   out_assign[n_reads]  contig index of the chosen hit | MNC_UNMAPPED | MNC_AMBIGUOUS
 *   out_best[n_reads]    the hit with the smallest NM/mlen (the last such hit when tied, i.e.
 *                        also for MNC_AMBIGUOUS; zero when there is no gated hit); may be NULL
 *   out_nhits[n_reads]   number of gated hits of the read; may be NULL
 * The gated hit lists themselves stay in HBM until the next call; fetch them with
 * mnc_engine_fetch_hits (needed for the multi-part merge, aligner.py:196-203, 218-223).
 */
int mnc_classify_batch(mnc_engine *eng, const uint8_t *bases, const int64_t *offsets,
                       uint32_t n_reads, int min_mapq,
                       int32_t *out_assign, mnc_hit_t *out_best, int32_t *out_nhits);

/* The next batch's bases on their way while this one is classified: starts the host-to-device copy of (bases,
 * offsets) into a spare device buffer on a stream of its own and returns.  The mnc_classify_batch call that
 * follows with the SAME pointers and n_reads skips its copy.  The reference has no counterpart -- its loop
 * hands mappy one read at a time (aligner.py:191-193, 212-215); here a batch crosses PCIe (5 kB of ASCII per
 * read), which would otherwise sit in front of every batch's kernels.  The caller leaves the host arrays as they
 * are until that call (page-locked arrays, e.g. mnc_fastq's, make the copy asynchronous).  *started = 0 when a
 * prefetched batch is still waiting for its call (one spare buffer): nothing was done.  Thread-safe against the
 * engine's classifying thread. */
int mnc_engine_prefetch(mnc_engine *eng, const uint8_t *bases, const int64_t *offsets, uint32_t n_reads, int *started);
/* Forget the batch announced last, if any (waits for its copy; the host arrays are the caller's again).  For a caller
 * that gives up on an announced batch -- an error in its loop (the reference's loop simply raises, aligner.py:212-215),
 * an engine handed to another sample: the announcement is matched by host address, so it must not outlive its arrays. */
int mnc_engine_prefetch_cancel(mnc_engine *eng);

/* Same, all buffers device-resident (HBM), asynchronous on the engine's stream.
 * total_bases = offsets[n_reads].  d_counts (may be NULL) is an int64[n_genomes*3] table
 * that the call ADDS to: {reads, read bases, mlen} per genome, i.e. the three counting
 * modes of aligner.py:247-263 ('basic', 'query_length', 'matching'). */
int mnc_classify_device(mnc_engine *eng, const uint8_t *d_bases, const int64_t *d_offsets,
                        uint32_t n_reads, int64_t total_bases, int max_read_len, int min_mapq,
                        int32_t *d_assign, mnc_hit_t *d_best, int32_t *d_nhits, int64_t *d_counts);
int mnc_engine_sync(mnc_engine *eng);

/* gated hits of the last batch: hit_offsets[n_reads+1] and hits[cap]; *n_hits = total.
 * Returns MNC_ERR_RANGE (with *n_hits set) if cap is too small. */
int mnc_engine_fetch_hits(mnc_engine *eng, int64_t *hit_offsets, mnc_hit_t *hits, int64_t cap,
                          int64_t *n_hits);

/* mnc_counts  <- the Counter accumulation aligner.py:247-263 on host arrays.
 * mode: 1 'basic' (+1), 2 'query_length' (+len(seq)), 3 'matching' (+mlen).
 * counts[n_genomes] is ADDED to. */
int mnc_counts(const mnc_index *idx, const int32_t *assign, const mnc_hit_t *best,
               const int64_t *offsets, uint32_t n_reads, int mode, int64_t *counts);

/* cross-part merge of gated hit lists <- aligner.py:219-233 + best_hit 328-339 in exact
 * integer arithmetic.  hits of all parts of one read are concatenated in part order;
 * rid values must already be global.  Writes the decision per read. */
int mnc_best_hit(const mnc_hit_t *hits, int n, int *best_index /* -1 = ambiguous */);

/* ---------------------------------------------------------------- profiling / introspection */
#define MNC_STAGE_PACK        0
#define MNC_STAGE_SKETCH      1
#define MNC_STAGE_PARTITION   2   /* scan + scatter of query records by table region        */
#define MNC_STAGE_PROBE       3   /* index probe: the HBM-roofline kernel                    */
#define MNC_STAGE_COLLECT     4   /* probe hits back to per-read lists                       */
#define MNC_STAGE_SORT        5   /* anchor offsets (scan) + size classes                    */
#define MNC_STAGE_SORT2       6   /* expand hits to anchors + sort                           */
#define MNC_STAGE_CHAIN       7   /* chaining DP (LDS ring per read)                         */
#define MNC_STAGE_BACKTRACK   8   /* backtrack -> chain records                              */
#define MNC_STAGE_REGIONS     9   /* regions, MAPQ, decision, counts                         */
#define MNC_STAGE_GATHER      10  /* gated hit lists -> CSR (mnc_engine_fetch_hits)          */
#define MNC_STAGE_DP_PLAN     11  /* chained anchors per region, DP windows, ksw2 segments   */
#define MNC_STAGE_DP_ALIGN    12  /* extensions, unusual gaps: ksw2's kernel in its own layout  */
#define MNC_STAGE_DP_STITCH   13  /* CIGAR merge / clean-up, mlen, blen, dp_max, Z-drop split */
#define MNC_STAGE_DP_POST     14  /* second hierarchy pass, DP MAPQ, gate, decision          */
#define MNC_STAGE_DP_FILL     15  /* gap filling between seeds: banded two-piece affine DP       */
#define MNC_STAGE_DP_FILL_T1  16  /* the next four only with debug bit 0x10000 (kernels one at a time):  */
#define MNC_STAGE_DP_FILL_T2  17  /*   the banded gap-filling kernel's 32- / 64- / 128-cell launches     */
#define MNC_STAGE_DP_FILL_T3  18
#define MNC_STAGE_DP_EXT      19  /*   all the extension kernels                                         */
#define MNC_STAGE_DP_FILL_TM  20  /*   the 42-cell launch of the banded kernel (between T1 and T2)       */
#define MNC_STAGE_DP_LFILL    21  /*   gaps of 512 .. 2047 bases on the int32 banded kernel              */
#define MNC_N_STAGES          22
int mnc_engine_set_profiling(mnc_engine *eng, int on);    /* HIP events around every stage */
int mnc_engine_set_debug(mnc_engine *eng, int mode);      /* test switches, a bit mask: 2 stress build of the
                                                             chaining ring, 4 displacement bytes read from HBM,
                                                             0x10 every region planned by mnc_dp_plan_long, 0x20 the
                                                             literal kernel's long calls on one wave (not four),
                                                             0x10000 the alignment kernels one at a time (per-kernel
                                                             timers), bits 8-15 a tuning value for the tier choice,
                                                             0x20000 / 0x40000 / 0x80000 / 0x100000 without the packed
                                                             extension / packed gap-filling / long-gap / long-extension
                                                             kernels (their calls go to the next kernel in line),
                                                             0x200000 the stitch kernel reads bases in place (its form
                                                             for regions beyond its LDS), 0x400000 without the 42-cell
                                                             tier, bits 24-30 that tier's tuning value, 0x800000 the
                                                             regions of long reads planned one lane each as all others
                                                             (not by mnc_dp_plan_long) */
/* accumulated since the last reset: ms[MNC_N_STAGES], launches[MNC_N_STAGES] */
int mnc_engine_get_timings(mnc_engine *eng, double *ms, int64_t *launches, int reset);
const char *mnc_stage_name(int stage);
const char *mnc_stage_kernel(int stage);                  /* kernel symbol, for rocprof matching */
/* counters of the last batch: [0] minimizers, [1] probe hits, [2] anchors, [3] chains,
 * [4] regions, [5] gated hits, [6] reads with ambiguous bases, [7] -; with n >= 12, of the base-level
 * alignment stage (last round): [8] kernel calls (segments), [9] gap fillings given to the banded kernel's
 * 32-cell tier, [10] those its 64-cell tier saw, [11] those handed back to the literal kernel; with
 * n >= 16: [12] / [13] / [14] anti-diagonals (steps) of the gap fillings the 32- / 64- / 128-cell tier
 * ran, [15] anti-diagonal steps x query bases of the extensions given to the packed extension kernel; with n >= 24
 * (last round): [16] / [17] calls planned for the literal kernel's large / small workspace, [18] long gaps (int32 banded
 * kernel), [19] those handed back that need the large workspace, [20] long extensions, [21] gap fillings the 128-cell tier saw */
int mnc_engine_get_counters(mnc_engine *eng, int64_t *c, int n);

/* Test hooks of the index residency: the device tables (hash-and-displace perfect hash per table region) are built
 * on the device; `on` = 1 makes the next upload of this index use the host form of the same construction instead;
 * mnc_engine_dump_tables copies what the engine's device holds ([region_bits, disp_bits] int32, salts, displacement
 * bytes, presence filter, table slots) so that the two can be compared. */
int mnc_index_set_host_tables(mnc_index *idx, int on);
/* the device tables are cut into 2^bits regions (8 .. 10; 0 = chosen from the number of keys so that a region stays at
 * 2 MiB): a speed matter only -- every value gives the same results (tests force the larger ones on small indexes) */
int mnc_index_set_region_bits(mnc_index *idx, int bits);
int mnc_engine_dump_tables(mnc_engine *eng, void *dst, int64_t cap_bytes, int64_t *n_bytes);

/* stage dumps of the last batch, for kernel-level parity tests */
#define MNC_DUMP_MINIMIZERS 1  /* u32 pairs {hash, pos<<1|strand} in read order                    */
#define MNC_DUMP_MZ_OFFSETS 2  /* int64[n_reads+1]                                              */
#define MNC_DUMP_ANCHORS    3  /* u64 x,y pairs sorted by (x,y), per read                       */
#define MNC_DUMP_AN_OFFSETS 4  /* int64[n_reads+1]                                              */
#define MNC_DUMP_CHAIN_F    5  /* int32 per anchor                                              */
#define MNC_DUMP_CHAIN_P    6  /* int32 per anchor (read-local index, -1 none)                  */
#define MNC_DUMP_CHAIN_V    7  /* int32 per anchor                                              */
#define MNC_DUMP_REGS       8  /* mnc_reg_t per region                                          */
#define MNC_DUMP_REG_OFFSETS 9 /* int64[n_reads+1]                                              */
#define MNC_DUMP_REP_LEN    10 /* int32 per read                                                */
#define MNC_DUMP_CIGARS     11 /* uint32 len<<4|op (0 M, 1 I, 2 D) of the dumped regions, back to back
                                  (regs[i].n_cigar words each); MNC_CONTRACT_DP only              */
#define MNC_DUMP_SEGS       12 /* the alignment stage's kernel calls (one per ksw_extd2 call of mm_align1): 24 int32
                                  {read, region slot, kind 0 left ext / 1 gap / 2 right ext, rid, rev, ts, tlen,
                                  qs, qlen, w, zdrop, flag, seed, kernel class, n_cigar, zdropped, zdrop_code,
                                  max, max_t, max_q, score, reach_end, mqe_t, pad} + int64 CIGAR offset (first word of the
                                  call's CIGAR in MNC_DUMP_SEG_CIGARS); MNC_CONTRACT_DP only.  tests/segments.py replays
                                  every call on the CPU oracle from it; tools/ read it as well.  Result fields a later
                                  step never reads for that kind and outcome may be left as planned (max 0, max_t / max_q /
                                  mqe_t -1, score -2^30): the table in tests/segments.py                              */
#define MNC_DUMP_SEG_CIGARS 13 /* the per-call CIGAR pool of those calls: uint32 len<<4|op (0 M, 1 I, 2 D), every word
                                  handed out in the last batch; a call's CIGAR is words [cig_off, cig_off + n_cigar), in the
                                  order ksw_extd2 returns them for that call: first to last operation of the sequences AS
                                  PASSED to the kernel for a gap filling and a right extension; for a left extension (both
                                  sequences reversed, KSW_EZ_REV_CIGAR) last to first of the reversed pair, i.e. left to
                                  right on the read -- so that a region's CIGAR is its calls' words back to back.  Calls
                                  land in the pool in the order the kernels finished them.  MNC_CONTRACT_DP only           */
typedef struct {
	int32_t id, parent, rid, rev, rs, re, qs, qe, score, score0, cnt, as, mlen, blen,
	        subsc, n_sub, mapq;
	uint32_t hash;
	/* base-level alignment (0 under MNC_CONTRACT_CHAIN): mm_extra_t's dp_score / dp_max / dp_max2 /
	 * n_ambi / n_cigar; flags: 1 a CIGAR exists, 2 / 4 split left / right part, 8 split_inv */
	int32_t dp_score, dp_max, dp_max2, n_ambi, n_cigar, flags;
} mnc_reg_t;
int mnc_engine_dump(mnc_engine *eng, int what, void *dst, int64_t cap_bytes, int64_t *n_bytes);

/* ---------------------------------------------------------------- alignment records
 * Everything index.map() yields per hit (aligner.py:193, 215; mappy's q_st q_en r_st r_en strand mlen blen mapq NM
 * cigar, and cs / MD on request) for the whole of the last classified batch, made on the device by a stage that runs
 * only when asked for (csrc/k_export.hip): without an export call a batch costs not one more kernel, allocation or byte.
 *
 *   mnc_engine_export_alignments   builds, in HBM pools the engine owns: one mnc_aln_t per region of every read's list
 *                                  (secondaries, Z-drop splits and inversion regions alike; read order, within a read the
 *                                  order of MNC_DUMP_REGS = the order mappy yields hits), the CSR over reads, the CIGARs
 *                                  back to back, and -- `what` = MNC_ALN_CS | MNC_ALN_MD -- the cs (short form, no "cs:Z:")
 *                                  and MD strings of minimap2 2.17's write_cs_core / write_MD_core.  Works on the engine's
 *                                  stream from the last batch as it stands in HBM (regions, region CIGARs, the batch's
 *                                  bases, the contig bases), so after mnc_classify_device the caller's d_bases /
 *                                  d_offsets must still be there.  The host waits twice for a few bytes (the record count
 *                                  sizes the record pool, the three pool sizes the rest); the pass that fills the pools is
 *                                  left running on the stream.  Any size pointer may be NULL.
 *   mnc_engine_fetch_alignments    copies them to the host.  MNC_ERR_RANGE when any cap is below what export reported
 *                                  (nothing is copied then); a pool pointer may be NULL when its size is 0.
 *   mnc_engine_alignments_device   the pools themselves (device pointers; any out pointer may be NULL), valid until the
 *                                  next classify or export call on the engine; ordered on the engine's stream.
 * Under MNC_CONTRACT_CHAIN there are records only (n_cigar = 0; blen / mlen / nm of the chain) and asking for cs / MD is
 * MNC_ERR_ARG.  After a call that ran both the usual and the wide pass (a mixed batch with mnc_engine_set_long_reads(1))
 * the engine holds the wide pass alone: MNC_ERR_UNSUPPORTED -- classify the two groups in separate calls.
 * Strand: qs / qe are forward-strand read coordinates (mappy's q_st / q_en).  The CIGAR, cs and MD run left to right on
 * the contig; for rev = 1 the query side is the reverse complement of the read, i.e. column 0 faces read base qe - 1. */
typedef struct {
	int32_t read;              /* ordinal of the read in the call                                  */
	int32_t rid, rev;
	int32_t qs, qe, rs, re;    /* as mnc_reg_t: mappy's q_st q_en r_st r_en                         */
	int32_t mapq, mlen, blen, nm;   /* nm = blen - mlen + n_ambi                                    */
	int32_t score, cnt;        /* mnc_reg_t.score, .cnt                                            */
	int32_t dp_score, dp_max, n_ambi;
	int32_t flags;             /* bit 0 primary (id == parent), bit 1 passes the gate of the call
	                              (primary and mapq >= min_mapq), bits 8.. = mnc_reg_t.flags << 8   */
	int32_t n_cigar;
	int64_t cigar_off;         /* words, into the CIGAR pool (len<<4|op, 0 M 1 I 2 D)              */
	int64_t cs_off, md_off;    /* bytes, into the cs / MD pools; strings are NOT NUL-terminated     */
	int32_t cs_len, md_len;    /* 0 when not asked for                                             */
} mnc_aln_t;

#define MNC_ALN_CS 1
#define MNC_ALN_MD 2
int mnc_engine_export_alignments(mnc_engine *eng, int what,
        int64_t *n_aln, int64_t *n_cigar_words, int64_t *n_cs_bytes, int64_t *n_md_bytes);
int mnc_engine_fetch_alignments(mnc_engine *eng, int64_t *aln_offsets /* n_reads+1, may be NULL */,
        mnc_aln_t *alns, int64_t cap_aln, uint32_t *cigar, int64_t cap_cigar,
        char *cs, int64_t cap_cs, char *md, int64_t cap_md);
int mnc_engine_alignments_device(mnc_engine *eng, const int64_t **d_aln_offsets, const mnc_aln_t **d_alns,
        const uint32_t **d_cigar, const char **d_cs, const char **d_md);
/* device time of the last export (count pass + scans + write pass), with mnc_engine_set_profiling on; waits for it */
int mnc_engine_export_ms(mnc_engine *eng, double *ms);
/* mappy.Aligner.seq(): bases [start, end) of contig rid as "ACGTN" (not NUL-terminated); MNC_ERR_ARG when rid or the
 * interval is out of range (0 <= start <= end <= contig length) */
int mnc_index_getseq(const mnc_index *idx, int rid, int64_t start, int64_t end, char *out /* end-start bytes, "ACGTN" */);

/* ---------------------------------------------------------------- coverage
 * Where on the genomes the reads landed: depth and breadth of coverage per contig, accumulated on the device from batch
 * to batch the way mnc_classify_device's d_counts is.  The reference counts per genome in three modes (aligner.py:247-263:
 * 'basic', 'query_length', 'matching'); this is a fourth kind of count over the same hits -- per reference base instead of
 * per genome -- made from the regions and region CIGARs of the last batch as they stand in HBM (csrc/k_coverage.hip).  A
 * batch that does not ask for it costs not one more kernel, allocation or byte.
 *
 * An mnc_coverage belongs to one index on one device and holds a depth track over every reference base of that index.  It
 * is additive: adding batch A and then batch B equals adding one batch with the reads of both; it lives across any number
 * of classify calls and across engines of the same index and device.  Engines of the same index and device may add to one
 * mnc_coverage from their own threads at the same time; reset and the read-outs are for one thread at a time.
 *
 * What a call adds -- `what` = exactly ONE selector, optionally | MNC_COV_SPAN:
 *   MNC_COV_GATED     every record that passes the gate of the call (primary and mapq >= min_mapq: mnc_aln_t.flags bit 1)
 *   MNC_COV_PRIMARY   every primary record (flags bit 0)
 *   MNC_COV_ALL       every record: secondaries, Z-drop splits and inversion regions alike
 *   MNC_COV_ASSIGNED  for each read whose decision in THIS call is a contig (out_assign >= 0), the one gated record that
 *                     best_hit chose (aligner.py:328-339): the gated record with the smallest nm / mlen by int64
 *                     cross-products as in mnc_best_hit -- unique whenever the decision is a contig, since best_hit answers
 *                     ambiguous exactly when its last update was a tie.  Reads that come back unmapped, ambiguous or
 *                     skipped add nothing.  Across the parts of a multi-part database the final decision is known only
 *                     after the last part (aligner.py:196-203, 218-223): a caller there adds MNC_COV_GATED per part.
 *                     After mnc_classify_device the caller's d_assign must still be there.
 *   default           a record adds 1 to the depth of every reference base in its M columns; reference bases under a D are
 *                     not covered (as in `samtools depth`); insertions consume no reference
 *   MNC_COV_SPAN      a record adds 1 to every base of [rs, re) whatever its CIGAR.  Under MNC_CONTRACT_CHAIN there is no
 *                     CIGAR and SPAN is required: a call without it is MNC_ERR_ARG (the rule of cs / MD)
 * After a call that ran both the usual and the wide pass the engine holds the wide pass alone: MNC_ERR_UNSUPPORTED and the
 * accumulator untouched, as mnc_engine_export_alignments; a call whose reads are all long adds like any other. */
typedef struct mnc_coverage mnc_coverage;
#define MNC_COV_GATED    1
#define MNC_COV_PRIMARY  2
#define MNC_COV_ALL      4
#define MNC_COV_ASSIGNED 8
#define MNC_COV_SPAN     16
/* aligner.py:247-263 (a Counter per sample; here a track per index and device).  bin_bases >= 1: the width of the bins of
 * the per-contig profile (mnc_coverage_fetch_bins); bins do not cross contigs, the last bin of a contig is short.
 * MNC_ERR_ARG for bin_bases < 1, MNC_ERR_NODEVICE without a gfx950 device, MNC_ERR_NOMEM when HBM is short. */
int  mnc_coverage_create(mnc_index *idx, int device, int bin_bases, mnc_coverage **out);
/* frees the accumulator and the HBM it holds (waits for the work queued on it) */
void mnc_coverage_free(mnc_coverage *cov);
/* clears the depth track and the alignment counts (`Counter()` anew, aligner.py:247); asynchronous */
int  mnc_coverage_reset(mnc_coverage *cov);
/* HBM the accumulator holds: 4 bytes per reference base, a few words per contig and 8 bytes per 1 024 bases of scratch */
int  mnc_coverage_device_bytes(const mnc_coverage *cov, int64_t *bytes);
/* aligner.py:247-263, the fourth kind: adds the last classified batch of `eng` as it stands in HBM.  Needs no
 * mnc_engine_export_alignments and disturbs none made before or after.  Asynchronous on the engine's stream, no host wait.
 * MNC_ERR_ARG: `cov` is for another index or device than the engine's current ones; no selector or more than one; no
 * batch has been classified yet; no MNC_COV_SPAN under MNC_CONTRACT_CHAIN.  The accumulator is untouched on any error. */
int  mnc_engine_add_coverage(mnc_engine *eng, mnc_coverage *cov, int what);
/* aligner.py:247-263 read out: one value per contig, any pointer may be NULL.  covered = bases with depth > 0;
 * depth_sum = the sum of depth over the contig's bases; max_depth; n_aln = records added to the contig.  Waits for the
 * work queued so far and leaves the accumulator as it is: it can be called between the batches of a run. */
int  mnc_coverage_summary(mnc_coverage *cov, int64_t *covered, int64_t *depth_sum, int32_t *max_depth, int64_t *n_aln);
/* the profile of one contig: covered bases and depth sum per bin of bin_bases bases.  *n_bins = ceil(len / bin_bases);
 * MNC_ERR_RANGE, with *n_bins set and nothing written, when cap is short; MNC_ERR_ARG for a bad rid.  Either array may be
 * NULL. */
int  mnc_coverage_fetch_bins(mnc_coverage *cov, int rid, int32_t *bin_covered, int64_t *bin_depth_sum, int64_t cap, int64_t *n_bins);
/* per-base depth of bases [start, end) of contig rid; the interval is checked as by mnc_index_getseq (MNC_ERR_ARG).  For
 * tests and zoomed plots: the contig's track is summed from its first base up to `end`. */
int  mnc_coverage_fetch_depth(mnc_coverage *cov, int rid, int64_t start, int64_t end, int32_t *depth /* end - start */);
/* The raw additive track (device pointer), for ranks that sum their tracks with a collective of their own (int32 sum over
 * n_words words, e.g. ncclAllReduce; none is added here).  Layout: n_words = total_len int32 words, the contigs back to
 * back in index order without padding -- base p of contig c is word (sum of the lengths of contigs 0 .. c - 1) + p -- holding
 * depth DIFFERENCES: +1 where a covered run starts, -1 one past where it ends; depth(c, p) = the sum of contig c's words
 * 0 .. p, starting anew at every contig.  The -1 of a run that ends on a contig's last base would fall on the next contig's
 * first word and is dropped, so a contig's words need not sum to zero.  Ordered behind the adds only after
 * mnc_coverage_summary or a sync of the engines that added. */
int  mnc_coverage_device(mnc_coverage *cov, const int32_t **d_track, int64_t *n_words);

/* ---------------------------------------------------------------- pileup
 * What the reads say at each reference base: allele counts, variants and a consensus, the question the reference's focus
 * pass (`-F`, "focus analysis on their subspecies") is asked -- two strains 0.5 % apart differ at a few thousand positions.
 * An mnc_pileup sits beside mnc_coverage and has its lifetime rules: it belongs to one index on one device, lives across
 * classify calls, is added to from the last batch as it stands in HBM (regions, region CIGARs, the reads' bases, the
 * contigs' 4-bit store; csrc/k_pileup.hip) asynchronously on the engine's stream with no host wait, and runs only when
 * asked for: a batch that does not ask costs not one more kernel, allocation or byte.  Unlike mnc_coverage, engines of the
 * same index and device may add to one mnc_pileup from their own threads at the same time; reset and the read-outs are for
 * one thread at a time.
 *
 * What a call adds -- `what` = exactly ONE of MNC_COV_GATED / PRIMARY / ALL / ASSIGNED, with the meaning they have for
 * coverage (MNC_COV_SPAN has none here: MNC_ERR_ARG).  A selected record's CIGAR is walked from rs on the contig; its query
 * columns are taken on the hit's strand, as cs and MD take them: column p of the query side is read base qs + p for
 * rev = 0 and the COMPLEMENT of read base qe - 1 - p for rev = 1.  A read base counts as A, C, G or T in either case
 * (U / u as T), as N otherwise; a reference base r is A, C, G, T, or N for anything else in the 4-bit store.  Per column:
 *   M column at reference base p, query base b   depth[p] += 1 (the M columns of coverage without MNC_COV_SPAN) and one
 *                                                observation of b at p: count[b][p] += 1, b one of A C G T N
 *   D operation                                  del[p] += 1 for every base p under it (depth is not touched)
 *   I operation                                  ins[q] += 1 ONCE per operation, whatever its length: q is the reference
 *                                                position of the last reference-consuming column before it in that record.
 *                                                An I with no such column is not counted (mm_fix_cigar leaves none).
 *                                                THE INSERTED BASES ARE NOT STORED: an insertion is known by place and count
 * The result is eight planes per reference base, in this order: depth, A, C, G, T, N, DEL, INS (MNC_PILE_*), all exact
 * integers.  Addition commutes: the result does not depend on order or on how a sample was cut into batches.
 * Derived: span[p] = depth[p] + del[p], the records that say something about base p.
 *
 * Storage (what mnc_pileup_device hands out; 32 bytes of HBM per reference base): most columns match the reference, so a
 * column does not cost an atomic.  Word w of every plane below is base p of contig c with w = (sum of the lengths of
 * contigs 0 .. c - 1) + p, the layout of mnc_coverage_device:
 *   d_depth  int32[n_words]      depth DIFFERENCES, exactly mnc_coverage's track: +1 where a run of M columns starts, -1
 *                                one past its end, the -1 that would fall on the next contig's first word dropped;
 *                                depth(c, p) = the sum of contig c's words 0 .. p
 *   d_alt    int32[7][n_words]   channel-major, channels A C G T N DEL INS: an M column adds to its query base's channel
 *                                only where it is NOT a reference match -- a mismatch, a query N, or any column over a
 *                                reference N (which adds to its own base's channel); DEL and INS as above
 *   count[b][p] = alt[b][p] + (r == b ? depth[p] - (alt[A] + alt[C] + alt[G] + alt[T] + alt[N])[p] : 0)   for b in A C G T
 *   count[N][p] = alt[N][p]
 * Every word is additive, the depth differences included: ranks sum the 8 * n_words words with one collective of their own. */
typedef struct mnc_pileup mnc_pileup;
#define MNC_PILE_DEPTH 0
#define MNC_PILE_A     1
#define MNC_PILE_C     2
#define MNC_PILE_G     3
#define MNC_PILE_T     4
#define MNC_PILE_N     5
#define MNC_PILE_DEL   6
#define MNC_PILE_INS   7
#define MNC_PILE_PLANES 8
/* one called variant (mnc_pileup_call_variants): 20 bytes */
typedef struct {
	int32_t rid, pos;            /* contig, 0-based reference position (an insertion: the base on its left) */
	int32_t span;                /* depth + del at pos */
	int32_t count;               /* observations of `alt` at pos */
	uint8_t ref;                 /* 'A' 'C' 'G' 'T' */
	uint8_t alt;                 /* 'A' 'C' 'G' 'T', '-' (deleted), '+' (an insertion follows; its bases are not stored) */
	uint8_t pad[2];              /* 0 */
} mnc_variant_t;
/* MNC_ERR_NODEVICE without a gfx950 device, MNC_ERR_ARG for an index without contig bases, MNC_ERR_NOMEM when the 32 bytes
 * per reference base do not fit the HBM that is free (3.0 GB for an index of 94 Mbp). */
int  mnc_pileup_create(mnc_index *idx, int device, mnc_pileup **out);
/* frees the accumulator and the HBM it holds (waits for the work queued on it) */
void mnc_pileup_free(mnc_pileup *pu);
/* clears every plane; asynchronous */
int  mnc_pileup_reset(mnc_pileup *pu);
/* HBM the accumulator holds: 32 bytes per reference base, a few words per contig and 24 bytes per 1 024 bases of scratch */
int  mnc_pileup_device_bytes(const mnc_pileup *pu, int64_t *bytes);
/* The raw additive planes (device pointers), laid out as above; either pointer may be NULL.  Ordered behind the adds only
 * after a read-out call below or a sync of the engines that added. */
int  mnc_pileup_device(mnc_pileup *pu, const int32_t **d_depth, const int32_t **d_alt, int64_t *n_words);
/* Adds the last classified batch of `eng` as it stands in HBM.  Needs no mnc_engine_export_alignments and disturbs none.
 * Asynchronous on the engine's stream, no host wait.  MNC_ERR_ARG: `pu` is for another index or device than the engine's
 * current ones; no selector, more than one, or MNC_COV_SPAN; no batch has been classified yet; MNC_CONTRACT_CHAIN (no
 * CIGAR).  MNC_ERR_UNSUPPORTED: the last call ran both the usual and the wide pass (the engine holds the wide pass alone);
 * a call whose reads are all long adds like any other.  The accumulator is untouched on any error. */
int  mnc_engine_add_pileup(mnc_engine *eng, mnc_pileup *pu, int what);
/* The eight planes of bases [start, end) of contig rid, plane-major: out[k * (end - start) + (p - start)], k = MNC_PILE_*.
 * The interval is checked as by mnc_index_getseq (MNC_ERR_ARG).  Waits for the work queued so far and leaves the
 * accumulator as it is, like every read-out below. */
int  mnc_pileup_fetch_counts(mnc_pileup *pu, int rid, int64_t start, int64_t end, int32_t *out /* [8][end - start] */);
/* The variants of contig rid, or of every contig for rid = -1, compacted in (rid, pos, allele) order, the alleles of a
 * position in the order A, C, G, T, DEL, INS.  An allele with count c at a base with reference base r is called iff r is
 * not N, the allele is not r, span >= min_depth, c >= min_count and c * 1000 >= min_permille * span (compared in int64:
 * no floating point anywhere).  *n = the number of variants; MNC_ERR_RANGE, with *n set and nothing written, when cap is
 * short; MNC_ERR_ARG for a bad rid.  Two passes on the device -- count, scan, write -- so only the variants travel. */
int  mnc_pileup_call_variants(mnc_pileup *pu, int rid, int32_t min_depth, int32_t min_count, int32_t min_permille,
                              mnc_variant_t *out, int64_t cap, int64_t *n);
/* One character per base of [start, end) of contig rid (not NUL-terminated; the interval checked as above): 'N' where
 * span < min_depth; otherwise the largest of the counts of A, C, G, T and DEL -- on a tie the reference base if it is
 * among the tied, else the first of them in that order -- written 'A' 'C' 'G' 'T' or '-'.  Insertions do not appear:
 * their bases are not stored. */
int  mnc_pileup_consensus(mnc_pileup *pu, int rid, int64_t start, int64_t end, int32_t min_depth, char *out /* end - start */);

/* ---------------------------------------------------------------- abundance
 * Which of several close genomes is in the sample, and how much of each: the other half of the focus pass' question.  The
 * count table cannot answer it -- a read counts only with a primary hit of mapq >= min_mapq, and against genomes 0.5-1 %
 * apart MAPQ drops to single digits on every stretch they share -- but each read's region list already holds its primary
 * and up to best_n secondaries with a base-level score dp_max each.  An mnc_abundance collects, per read, the genomes that
 * fit it about equally well, and mnc_abundance_solve runs an expectation-maximisation over those candidate lists (as
 * Pathoscope and its descendants do on top of an aligner): theta = the share of the sample's reads each genome explains.
 * It sits beside mnc_coverage and mnc_pileup and has their lifetime rules: it belongs to one index on one device, lives
 * across classify calls and engines, is added to from the last batch as it stands in HBM (csrc/k_abundance.hip)
 * asynchronously on the engine's stream with no host wait, and runs only when asked for: a batch that does not ask costs
 * not one more kernel, allocation or byte.  Threading is mnc_pileup's: engines of the same index and device may add to one
 * mnc_abundance from their own threads at the same time; reset, add_lists and the read-outs (info, fetch_*, solve) are for
 * one thread at a time, and not while an engine adds.  A "genome" is the index's: mnc_index_contig_genome, G = n_genomes.
 *
 * What one read contributes (mnc_engine_add_abundance).  Take every record of the read's region list that has a CIGAR --
 * primaries, secondaries, Z-drop splits and inversion regions alike, the set MNC_COV_ALL walks.  For each genome g with at
 * least one such record, s_g = the largest dp_max of the read's records on contigs of g; best = the largest s_g;
 * delta_g = best - s_g >= 0.  Genome g is a CANDIDATE of the read iff delta_g <= max_delta.  A read with no record adds
 * nothing.  A read with exactly one candidate adds 1 to unique[g] (int64) and is not stored.  A read with two or more is
 * stored as one row of a CSR of (genome, delta) pairs in ascending genome id.  Rows are stored in no particular order --
 * nothing below depends on it -- and mnc_abundance_fetch_lists returns them SORTED: lexicographically by the row's sequence
 * genome[0], delta[0], genome[1], delta[1], ...; a row that is a prefix of another comes first.  n_reads counts every read
 * that added something (to unique or as a stored row).
 * Capacity: cap_cands candidate slots (12 bytes of HBM each: 4 + 4 and half a row offset).  A row that does not fit is not
 * stored: it is counted in n_dropped, adds nothing to unique or n_reads, and nothing is written past the end; a later,
 * shorter row may still fit.  mnc_abundance_solve answers MNC_ERR_RANGE while n_dropped > 0 (reset starts over).
 * Known limit: the candidates are what the region list holds -- a primary and at most best_n = 5 secondaries (MapParams) --
 * so a read that fits more than six genomes equally well sees six of them.
 *
 * Weights.  scale_q is quarter-bits of likelihood per unit of alignment score: with x = delta * scale_q a candidate weighs
 *   w = ldexp(T[x & 3], -(x >> 2)),   T[f] = 2^(-f/4) as exactly these doubles:
 *   0x1.0000000000000p+0, 0x1.ae89f995ad3adp-1, 0x1.6a09e667f3bcdp-1, 0x1.306fe0a31b715p-1
 * i.e. w = 2^(-x/4).  At the default scale_q = 3 one mismatch (6 units of score at a = 2, b = 4) costs a factor 2^-4.5,
 * about what a base call of 4-5 % error probability makes of a mismatch; the default is a guess of that kind and has not
 * been fitted to data.  max_delta * scale_q <= 4000 keeps every weight a normal double.
 *
 * mnc_abundance_solve: exact and reproducible -- one defined answer whatever the row order, the launch shape or the number
 * of batches the reads came in.  Start: theta[g] = 1.0 / G.  One iteration:
 *   acc[g] = unique[g] * 2^32                                      (uint64)
 *   for every stored row, candidates j in stored order:
 *     t_j = w_j * theta[genome_j];  z = t_0 + t_1 + ... added left to right, starting from 0.0
 *     if z > 0:  p_j = t_j / z;  acc[genome_j] += (uint64) floor(p_j * 4294967296.0)
 *   total = the sum of acc (uint64, exact);  theta[g] = (double) acc[g] / (double) total   (all zeros if total = 0)
 * Every multiply, add and divide is one IEEE double operation rounded to nearest, never a fused multiply-add; the two
 * conversions to double round to nearest.  The run stops after the iteration in which max_g |acc[g] - previous acc[g]| <=
 * tol_q32, compared as integers -- "previous" of the first iteration is all zeros, so with reads present the test can be met
 * from the second iteration on -- or after max_iter iterations.  *iters = the iterations run; expected[g] = (double) acc[g] /
 * 4294967296.0 of the last iteration (reads attributed to g; their sum falls short of the reads by less than 2^-32 per
 * stored candidate); theta is the last iteration's.  With nothing added theta and expected are zeros and *iters = 0.  The sums
 * are integer sums, so the M step does not depend on order: no floating-point atomic anywhere.  The accumulator is left as
 * it is: solve can be called between the batches of a run. */
typedef struct mnc_abundance mnc_abundance;
/* MNC_ERR_ARG: cap_cands < 0 (or >= 2^32), max_delta < 0, scale_q < 1, max_delta * scale_q > 4000.  MNC_ERR_NODEVICE without
 * a gfx950 device, MNC_ERR_NOMEM when HBM is short.  The Python layer's defaults: max_delta = 80, scale_q = 3. */
int  mnc_abundance_create(mnc_index *idx, int device, int64_t cap_cands, int32_t max_delta, int32_t scale_q, mnc_abundance **out);
/* frees the accumulator and the HBM it holds (waits for the work queued on it) */
void mnc_abundance_free(mnc_abundance *ab);
/* forgets every read: unique, the stored rows, n_reads and n_dropped; asynchronous */
int  mnc_abundance_reset(mnc_abundance *ab);
/* HBM the accumulator holds: 12 bytes per candidate slot and 32 bytes per genome */
int  mnc_abundance_device_bytes(const mnc_abundance *ab, int64_t *bytes);
/* Adds the last classified batch of `eng` as it stands in HBM.  Needs no mnc_engine_export_alignments and disturbs none.
 * Asynchronous on the engine's stream, no host wait.  MNC_ERR_ARG: `ab` is for another index or device than the engine's
 * current ones; no batch has been classified yet; MNC_CONTRACT_CHAIN (no dp_max).  MNC_ERR_UNSUPPORTED: the last call ran
 * both the usual and the wide pass (the engine holds the wide pass alone); a call whose reads are all long adds like any
 * other.  MNC_ERR_NODEVICE / MNC_ERR_NOMEM as elsewhere.  The accumulator is untouched on any error. */
int  mnc_engine_add_abundance(mnc_engine *eng, mnc_abundance *ab);
/* Adds rows made by the caller -- row r = (genome, delta)[offsets[r] .. offsets[r + 1]) -- with the same treatment: a row of
 * one candidate goes to unique, a row of two or more is stored; n_reads grows by n_reads.  For a caller who merges the
 * parts of a multi-part database itself (the library's own way is the candidate carry below).  Checked on the
 * host before anything is touched: MNC_ERR_ARG for an empty row, genome ids not strictly ascending within a row, a genome
 * id >= G or negative, a delta negative or above max_delta; MNC_ERR_RANGE when the rows would not fit -- nothing is added
 * then and n_dropped stays as it was.  Waits for the work queued so far. */
int  mnc_abundance_add_lists(mnc_abundance *ab, int64_t n_reads, const int64_t *offsets, const int32_t *genome, const int32_t *delta);
/* the counts as they stand (waits for the work queued so far); any pointer may be NULL.  n_stored_reads = rows of the CSR,
 * n_cands = candidate slots taken */
int  mnc_abundance_info(mnc_abundance *ab, int64_t *n_reads, int64_t *n_stored_reads, int64_t *n_cands, int64_t *n_dropped);
int  mnc_abundance_fetch_unique(mnc_abundance *ab, int64_t *unique /* [G] */);
/* the stored rows, sorted as stated above: offsets[n_stored_reads + 1] (offsets[0] = 0), genome / delta [n_cands].
 * MNC_ERR_RANGE, nothing written, when cap_reads < n_stored_reads or cap_cands < n_cands (mnc_abundance_info has both) */
int  mnc_abundance_fetch_lists(mnc_abundance *ab, int64_t *offsets, int32_t *genome, int32_t *delta, int64_t cap_reads, int64_t cap_cands);
/* the EM above.  MNC_ERR_ARG for max_iter < 1; MNC_ERR_RANGE while n_dropped > 0.  Queues every iteration without reading
 * anything back (a word on the device turns the launches behind the stop into no-ops) and waits once at the end. */
int  mnc_abundance_solve(mnc_abundance *ab, int32_t max_iter, uint64_t tol_q32, double *theta /* [G] */, double *expected /* [G] */, int32_t *iters);
/* The accumulator in place (device pointers; any out pointer may be NULL): unique int64[G]; the CSR as stored (NOT sorted):
 * d_offsets int64[n_stored_reads + 1], d_genome / d_delta int32[n_cands].  Ordered behind the adds only after a read-out
 * call above or a sync of the engines that added. */
int  mnc_abundance_device(mnc_abundance *ab, const int64_t **d_unique, const int64_t **d_offsets, const int32_t **d_genome, const int32_t **d_delta);

/* ---------------------------------------------------------------- candidate carry
 * Abundance over a database of SEVERAL index parts.  Close strains land in different parts, and a read's candidate genomes
 * have to be put together across them: that needs read identity, and a merge that does not depend on the order of the parts
 * or on how the reads were cut into batches.  An mnc_carry is both.  It belongs to a device, not to an index, and holds one
 * row per read of a sample, addressed by the read's ordinal in the sample (the sample file is the same for every part).  A
 * row is: best, the largest score seen for this read in any part so far; up to `width` pairs (global genome id, score); and
 * a sticky "truncated" bit.  8 * width + 8 bytes of HBM per read.  Every part's batches are carried into it from HBM as
 * they stand (mnc_engine_carry_candidates; csrc/k_carry.hip), and after the last part mnc_abundance_add_carry hands every
 * row to an accumulator made for the genomes of the whole database (mnc_abundance_create_global).  Runs only when asked
 * for: a batch that does not ask costs not one more kernel, allocation or byte.
 *
 * The merge rule.
 * 1. What one part gives a read.  For every genome g of the part with at least one counted record, s_g = the largest dp_max
 *    of the read's records on contigs of g.  A counted record is one that mnc_engine_add_abundance counts: of the set
 *    MNC_COV_ALL walks, with a CIGAR, on a contig of the index.  The part offers the pairs (g + genome_offset, s_g).  Only
 *    pairs within max_delta of the part's own best need be offered (the implementation passes over the others): that loses
 *    nothing, because the global best is at least the part's best.  A read with no counted record offers nothing and its
 *    row stays as it is.
 * 2. The incoming row.  best := max(best, the incoming scores).
 * 3. Merging into a row.  A genome already in the row keeps the larger of its two scores.  Then every pair with
 *    best - score > max_delta leaves.  If more than `width` pairs remain, the `width` pairs ranked highest stay -- ranking
 *    is by score descending, with ties going to the smaller genome id -- and the read's truncated bit is set.
 * 4. Consequences.  The final row is the top `width` pairs by that ranking among all pairs ever offered (per genome its
 *    largest score), cut at best - max_delta.  The operation is commutative, associative and idempotent, so the rows do not
 *    depend on the order of the parts, on how each part's reads were cut into batches, on which of the three entry points
 *    (mnc_engine_carry_candidates, mnc_carry_add_lists, mnc_carry_merge) delivered a pair, or on a part being carried
 *    twice.  Only n_truncated_reads may depend on the order: a pair can leave by the delta cut in one order and for room
 *    in another.  (mnc_carry_merge also hands on the source row's truncated bit.)
 *
 * Ordering and threading.  A carry's merges run one behind the other on the device: each waits for the previous merge's
 * event, whichever engine queued it, so engines may carry into one mnc_carry from their own threads -- by the property
 * above the result is the same.  Reset, reserve, add_lists, merge as dst, and the read-outs are for one thread at a time.
 * Nothing on the engine's stream waits on the host.  Every error leaves the carry untouched. */
typedef struct mnc_carry mnc_carry;
/* MNC_ERR_ARG: cap_reads < 0 (or > 2^32), width outside 1 .. 64 (a row lives in one wave of 64 lanes), max_delta < 0 -- all
 * checked before the device.  MNC_ERR_NODEVICE without a gfx950 device, MNC_ERR_NOMEM when HBM is short.  The Python
 * layer's defaults: width = 16, max_delta = 80. */
int  mnc_carry_create(int device, int64_t cap_reads, int32_t width /* 1..64 */, int32_t max_delta, mnc_carry **out);
/* frees the carry and the HBM it holds (waits for the work queued on it) */
void mnc_carry_free(mnc_carry *cc);
/* every row empty; asynchronous */
int  mnc_carry_reset(mnc_carry *cc);
/* grows to >= n_reads rows (by half as much again at least); contents kept, new rows empty.  Waits for the merges queued so
 * far when it has to grow; not while an engine carries.  MNC_ERR_NOMEM leaves the carry as it was. */
int  mnc_carry_reserve(mnc_carry *cc, int64_t n_reads);
/* HBM the carry holds: 8 * width + 8 bytes per row */
int  mnc_carry_device_bytes(const mnc_carry *cc, int64_t *bytes);
/* Merges the last classified batch of `eng`, as it stands in HBM, into rows first_read .. first_read + n_reads - 1: read r of
 * the batch is read first_read + r of the sample, genome g of the engine's index is genome genome_offset + g.  Asynchronous
 * on the engine's stream behind the carry's earlier merges, no host wait.  MNC_ERR_ARG: first_read < 0, genome_offset < 0,
 * genome_offset + the index's genomes beyond int32, a carry on another device than the engine's, no batch classified yet,
 * MNC_CONTRACT_CHAIN (no dp_max).  MNC_ERR_UNSUPPORTED: the last call ran both the usual and the wide pass, as for
 * mnc_engine_add_abundance.  MNC_ERR_RANGE: first_read + n_reads > cap_reads (mnc_carry_reserve first). */
int  mnc_engine_carry_candidates(mnc_engine *eng, mnc_carry *cc, int64_t first_read, int32_t genome_offset);
/* Host rows -- row r = (genome, score)[offsets[r] .. offsets[r + 1]), global genome ids -- merged by the same rule; row r goes
 * to read first_read + r.  Checked on the host before anything is touched: MNC_ERR_ARG for first_read < 0, an empty row,
 * genome ids negative or not strictly ascending within a row; MNC_ERR_RANGE for first_read + n_reads > cap_reads.  Waits. */
int  mnc_carry_add_lists(mnc_carry *cc, int64_t first_read, int64_t n_reads, const int64_t *offsets,
                         const int32_t *genome, const int32_t *score);
/* src's rows merged into dst's, row for row, by the same rule; src is left as it is.  MNC_ERR_ARG unless both are on one
 * device with one width and one max_delta; MNC_ERR_RANGE when src has more rows than dst.  Asynchronous. */
int  mnc_carry_merge(mnc_carry *dst, mnc_carry *src);
/* the counts as they stand (waits for the merges queued so far); any pointer may be NULL.  n_rows_used = rows that hold a
 * pair, n_cands = pairs held, n_truncated_reads = rows whose truncated bit is set */
int  mnc_carry_info(mnc_carry *cc, int64_t *cap_reads, int64_t *n_rows_used, int64_t *n_cands, int64_t *n_truncated_reads);
/* rows first_read .. first_read + n_reads - 1 (waits): count[r] pairs, best[r] (0 for an empty row), and the pairs in
 * ASCENDING GENOME ID in genome / score [n_reads][width], unused places -1 / 0.  Any out pointer may be NULL.
 * MNC_ERR_RANGE beyond cap_reads. */
int  mnc_carry_fetch(mnc_carry *cc, int64_t first_read, int64_t n_reads, int32_t *count, int32_t *best,
                     int32_t *genome, int32_t *score /* [n_reads][width], ascending genome id, unused slots -1 / 0 */);
/* The raw rows in place, for a collective of the caller's (gather them, then mnc_carry_add_lists or a carry of one's own and
 * mnc_carry_merge): d_head int32[cap_reads][2] = (best, flags: 1 the row holds a pair, 2 truncated); d_slots
 * int32[cap_reads][width][2] = (genome, score) in NO particular order, a free slot (-1, 0).  Any out pointer may be NULL.
 * Ordered behind the merges only after a read-out call above or a sync of the engines that carried; the pointers change
 * when mnc_carry_reserve grows the carry. */
int  mnc_carry_device(mnc_carry *cc, const int32_t **d_head, const int32_t **d_slots, int64_t *cap_reads, int32_t *width);

/* An abundance accumulator that is not tied to one index: mnc_abundance_create with G = n_genomes and no index, for the
 * genomes of a whole database in part order.  mnc_engine_add_abundance answers MNC_ERR_ARG for it (it is for no index);
 * add_lists, add_carry, the read-outs and solve work on it.  MNC_ERR_ARG also for n_genomes < 0. */
int  mnc_abundance_create_global(int device, int32_t n_genomes, int64_t cap_cands, int32_t max_delta, int32_t scale_q, mnc_abundance **out);
/* The carry's rows first_read .. first_read + n_reads - 1, each treated exactly as mnc_engine_add_abundance treats a read: no
 * pair, nothing; one pair, unique[g] += 1; two or more, one stored row of (genome, best - score) in ascending genome id, or
 * -- when it does not fit -- counted in n_dropped.  MNC_ERR_ARG, nothing added: the carry's max_delta differs from the
 * accumulator's, the device differs, or the carry holds a genome id >= G (its largest id is read back first: the one host
 * wait, for the carry's merges).  MNC_ERR_RANGE: first_read + n_reads > cap_reads.  The add itself is asynchronous on the
 * accumulator's stream behind the carry's merges.  The carry is left as it is. */
int  mnc_abundance_add_carry(mnc_abundance *ab, mnc_carry *cc, int64_t first_read, int64_t n_reads);

/* ---------------------------------------------------------------- FASTQ batches and read routing
 * Replaces the per-record Biopython objects of the reference's loop:
 * SeqIO.parse(sample, 'fastq') + str(seq_record.seq) (monica/genomes/aligner.py:191-193,
 * 212-215) and SeqIO.write(seq_record, handle, 'fastq') into mapped/ unmapped/ ambiguous/
 * focus/ (aligner.py:232-243, 265).  Records follow Biopython's FASTQ rules (multi-line
 * sequence / quality, '+' caption check, length check); a malformed file gives
 * MNC_ERR_FORMAT with Biopython's message in mnc_last_error().  A reader owns one batch at a
 * time; pointers returned by the accessors stay valid until the next mnc_fastq_next/close. */
typedef struct mnc_fastq mnc_fastq;
int mnc_fastq_open(const char *path, mnc_fastq **out);
void mnc_fastq_close(mnc_fastq *fq);
/* parse the next batch: stops after max_reads records or once max_bases bases are held.
 * *n_reads = 0 at the end of the file. */
int mnc_fastq_next(mnc_fastq *fq, uint32_t max_reads, uint64_t max_bases, uint32_t *n_reads);
/* the current batch as a handle of its own (the reader goes on with fresh arrays): for a host loop that parses
 * batch k + 1 while batch k is classified and batch k - 1 is written out.  Accessors, mnc_fastq_route and
 * mnc_hitmap_update take it like the reader; mnc_fastq_close frees it. */
int mnc_fastq_detach_batch(mnc_fastq *fq, mnc_fastq **out);
/* bytes of the file no batch has taken yet (-1 for a pipe): a host loop that overlaps parsing, classification and
 * output makes its first and last batches small, so that the pipeline fills and drains quickly */
int mnc_fastq_remaining(const mnc_fastq *fq, int64_t *bytes);
const uint8_t *mnc_fastq_bases(const mnc_fastq *fq);     /* concatenated sequences (page-locked when a GPU is present) */
const int64_t *mnc_fastq_offsets(const mnc_fastq *fq);   /* n_reads + 1, starts at 0 */
const uint8_t *mnc_fastq_quals(const mnc_fastq *fq);     /* quality characters, same offsets */
/* title line of read r (without '@'); *id_len = length of its first word (seq_record.id) */
int mnc_fastq_title(const mnc_fastq *fq, uint32_t r, const char **title, uint32_t *len, uint32_t *id_len);
/* Append every record of the batch to the files its dest[r] bits name:
 *   MNC_TO_UNMAPPED / MNC_TO_AMBIGUOUS / MNC_TO_FOCUS: the record as read;
 *   MNC_TO_MAPPED: the record with its id replaced by labels[label[r]]
 *   (seq_record.id = tax_unit, aligner.py:242; Biopython then writes "<id> <old title>").
 * paths[4] = {unmapped, ambiguous, mapped, focus}; a NULL path must not be addressed. */
#define MNC_TO_UNMAPPED  1
#define MNC_TO_AMBIGUOUS 2
#define MNC_TO_MAPPED    4
#define MNC_TO_FOCUS     8
int mnc_fastq_route(const mnc_fastq *fq, const uint8_t *dest, const int32_t *label,
                    const char *const *labels, int n_labels, const char *const *paths);
/* Append one PAF line per alignment record of the batch (mnc_engine_fetch_alignments' arrays, host) to `path` -- what
 * `minimap2 -c` prints for the hits index.map() yields: read name (the title's first word), read length, qs, qe, + / -,
 * contig name, contig length, rs, re, mlen, blen, mapq, then tp:A:P|S cm:i:<cnt> s1:i:<score> NM:i: AS:i:<dp_score>
 * ms:i:<dp_max> nn:i:<n_ambi>, then cg:Z: / cs:Z: / MD:Z: for each of cigar / cs / md that is not NULL.
 * flags bit 0: primary records only.  MNC_ERR_IO when the file cannot be opened or written. */
#define MNC_PAF_PRIMARY_ONLY 1
int mnc_fastq_write_paf(const mnc_fastq *fq, const mnc_index *idx,
        const int64_t *aln_offsets, const mnc_aln_t *alns,
        const uint32_t *cigar, const char *cs, const char *md,
        int flags, const char *path);

/* ---------------------------------------------------------------- hits carried across index parts
 * Replaces the `sample_hits` dict and its <sample>_hits.pkl (aligner.py:184-188, 196-203,
 * 218-223, 267-273): per read id, the gated hits of all index parts seen so far.  best_hit
 * (aligner.py:328-339) only asks for the smallest NM/mlen and whether it is attained once,
 * so a read's list is held as {hits, nm, mlen, contig name, tied}; extending the list and
 * reducing it commute with this summary, exactly (int64 cross-products). */
typedef struct mnc_hitmap mnc_hitmap;
int mnc_hitmap_create(mnc_hitmap **out);
int mnc_hitmap_load(const char *path, mnc_hitmap **out);
int mnc_hitmap_save(const mnc_hitmap *hm, const char *path);
void mnc_hitmap_free(mnc_hitmap *hm);
int64_t mnc_hitmap_size(const mnc_hitmap *hm);           /* ids with at least one hit */
/* For every read of the batch, in order: sample_hits[id].extend(this part's gated hits),
 * given as the engine's outputs (nhits, best = minimal hit, assign == MNC_AMBIGUOUS: tied);
 * then out[r] = the state of sample_hits[id]: {hits, nm, mlen, name id, tied}
 * (hits == 0: the id is not in the dict).  Name ids index mnc_hitmap_name(). */
int mnc_hitmap_update(mnc_hitmap *hm, const mnc_fastq *fq, const mnc_index *idx,
                      const int32_t *assign, const mnc_hit_t *best, const int32_t *nhits,
                      int32_t *out /* n_reads x 5 */);
int mnc_hitmap_n_names(const mnc_hitmap *hm);
const char *mnc_hitmap_name(const mnc_hitmap *hm, int id);

/* ---------------------------------------------------------------- collectives (RCCL over xGMI)
 * The cross-process forms of monica's two merges, on a caller-supplied ncclComm_t and HIP stream
 * (librccl.so is opened on first use; the library does not link it):
 *   mnc_allreduce_counts     <- Counter.update in alignment_update (aligner.py:286-298) when the reads
 *                               of a batch are sharded over GPUs: int64 sum of the count table
 *                               (n = n_genomes * 3 for the table mnc_classify_device fills), in place
 *   mnc_allgather_summaries  <- the hits carried between index parts (aligner.py:91-103, 196-203,
 *                               218-223) when the parts live on different GPUs: every rank's per-read
 *                               summary block {hits, nm, mlen, contig, tied} (20 B per read), in rank
 *                               order; the merge itself is mnc_best_hit's rule per read
 * mnc_comm_* make / free a communicator through this ABI alone (ncclGetUniqueId on one rank, the
 * 128 bytes handed to the others by any means, ncclCommInitRank on all). */
int mnc_comm_unique_id(void *id128);
int mnc_comm_init_rank(const void *id128, int n_ranks, int rank, void **comm);
int mnc_comm_destroy(void *comm);
int mnc_comm_count(void *comm, int *n_ranks);   /* ncclCommCount: the ranks the communicator really spans */
int mnc_allreduce_counts(int64_t *d_counts, int n, void *comm, void *stream);
int mnc_allgather_summaries(const void *d_send, void *d_recv, size_t bytes_per_rank, void *comm, void *stream);

/* ---------------------------------------------------------------- C2: the merge over index parts, on the device
 * The reference carries a read's gated hits from index part to index part (sample_hits[read_id].extend(...),
 * aligner.py:196-203, 218-223; pickled between passes, aligner.py:184-188, 267-273) and lets best_hit
 * (aligner.py:328-339) decide over the union (aligner.py:219-233).  best_hit only asks for the smallest NM/mlen and
 * whether the last update of its running minimum was a tie, so one part's list is the 20-byte record
 * {hits, nm, mlen, global contig | -1, tied} per read (the same record mnc_hitmap_update carries on the host).
 *   mnc_shard_summary     writes a part's records [n][5] from mnc_classify_device's outputs of that part
 *                         (d_assign, d_best, d_nhits); rid_offset = the part's first contig in the global numbering
 *   mnc_merge_summaries   best_hit over the parts: d_parts = [n_parts][n][5] int32 in part order (= hit order: what
 *                         mnc_allgather_summaries leaves when rank order is part order); d_assign[n] = global contig |
 *                         MNC_UNMAPPED | MNC_AMBIGUOUS; d_nm / d_mlen / d_total (the minimal hit's NM and mlen, the
 *                         number of gated hits over all parts) may be NULL.  int64 cross-products: mnc_best_hit's rule.
 * All pointers are device pointers; both calls are asynchronous on `stream` (a hipStream_t, NULL = the default stream). */
int mnc_shard_summary(const int32_t *d_assign, const mnc_hit_t *d_best, const int32_t *d_nhits, int64_t n,
                      int32_t rid_offset, int32_t *d_out, void *stream);
int mnc_merge_summaries(const int32_t *d_parts, int n_parts, int64_t n, int32_t *d_assign, int32_t *d_nm, int32_t *d_mlen,
                        int32_t *d_total, void *stream);

/* how many sample files the host works on side by side -- monica's ThreadPool runs aligner() once per sample,
 * aligner.py:89-103: every FASTQ reader's parse and routing passes then take cores / n_workers threads (1, the
 * default: all of them, at most 16).  "cores" = what the process may keep busy: the hardware threads, less what its
 * CPU affinity and its control group's quota (cpu.max / cpu.cfs_quota_us) leave of them.  The passes' helper threads
 * belong to the calling thread, sleep between passes and end with it (csrc/team.h); like an OpenMP runtime's, they do
 * not survive fork(). */
int mnc_host_set_io_workers(int n_workers);
/* page-locked host memory for batch buffers (plain malloc when no GPU is present) */
void *mnc_host_alloc(size_t bytes);
void mnc_host_free(void *p);

/* ---------------------------------------------------------------- synthetic data (bench/tests)
 * Deterministic counter-based generator (SplitMix64), SURVEY.md section 8d. */
int mnc_synth_genome(uint64_t seed, int64_t len, char *out);
int mnc_synth_diverge(const char *src, int64_t len, uint64_t seed, int rate_ppm, char *out);
/* reads: ordinal r in [first, first+n) draws from stream (seed, r).  Rates in 1e-4 units.
 * random_frac_e4 of the reads are pure random sequence (truth = -1). */
int mnc_synth_reads(int n_genomes, const char *const *genomes, const int64_t *lens,
                    uint64_t seed, int64_t first, int n_reads, int read_len,
                    int sub_e4, int ins_e4, int del_e4, int random_frac_e4,
                    char *out_bases, int32_t *out_truth);

/* the same reads made on the device (one wave per read), byte for byte: d_genomes = the contigs
 * concatenated (ASCII), d_g_off[n_genomes + 1] their starts; all pointers are device pointers, the
 * launch is asynchronous on `stream` (a hipStream_t, NULL = the default stream).  BASELINE config 3's
 * 10 M reads are 50 GB: they are generated where they are classified. */
int mnc_synth_reads_device(int n_genomes, const uint8_t *d_genomes, const int64_t *d_g_off,
                           uint64_t seed, int64_t first, int n_reads, int read_len,
                           int sub_e4, int ins_e4, int del_e4, int random_frac_e4,
                           uint8_t *d_out_bases, int32_t *d_out_truth, void *stream);

const char *mnc_version(void);

#ifdef __cplusplus
}
#endif
#endif
