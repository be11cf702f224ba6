// Per-base pileup (include/monica_amd.h, "pileup"): what the reads say at each reference base -- allele counts, variants,
// consensus -- in an accumulator that lives across classify calls, added to from the last batch as it stands in HBM
// (regions, region CIGARs, the reads' bases, the contigs' 4-bit store).  The third consumer of that data after k_export.hip
// and k_coverage.hip, and made of their parts.  Runs only when asked for; nothing here is on the classification path.
//
// The planes.  Eight int32 words per reference base, each plane laid out as the coverage track is (base p of contig c is
// word off[c] + p):
//   track   [n_words]      depth DIFFERENCES of the M columns, exactly k_coverage.hip's track: two atomics per maximal run of
//                          M columns, the contig-end rule unchanged (cov_put)
//   alt     [7][n_words]   A C G T N DEL INS, channel-major.  Most columns match the reference, and a match costs nothing: an
//                          M column adds to its query base's channel only where it is not a reference match (a mismatch, a
//                          query N, any column over a reference N); a D adds to DEL for every base, an I to INS once, at the
//                          base on its left.  At 10 % errors that is a tenth of the atomics of one per column.
//   on read-out            count[b][p] = alt[b][p] + (ref[p] == b ? depth[p] - (alt[A] + alt[C] + alt[G] + alt[T] + alt[N])[p] : 0)
//
//   mnc_pile_add    one wave per READ, the records found and selected as mnc_cov_add_runs does.  A selected record's CIGAR
//                   is walked 64 operations at a time (prefix sums of the query and the reference lengths; the depth runs
//                   from two ballots as in k_coverage.hip), and the columns of a chunk 64 at a time with ONE LANE PER COLUMN:
//                   a lane finds its operation by bisecting the operations' inclusive column counts through cross-lane
//                   reads, as mnc_export_strings does -- except that an I operation counts as ONE column here, since its
//                   bases are not looked at.  An M lane fetches its two bases and, if they differ or the reference has an
//                   N, issues its one atomic.  What crosses a chunk border is scalar: the two offsets and "a run is open".
//   mnc_pile_scan   the read-outs, one pass over the tiles of scan.h with depth as a running sum (k_coverage.hip's summary:
//                   the plain sum G over the words minus G in front of the contig).  MODE 0 writes the eight planes, MODE 3
//                   the consensus; variants take MODE 1 (calls per tile), scan.h's exclusive scan over the tiles, and MODE 2
//                   (each tile places its records behind its offset by a prefix sum over its threads): compacted and in
//                   (contig, position, allele) order without a per-base offset array.
#include <hip/hip_runtime.h>
#include <new>
#include <vector>
#include "device.h"
#include "scan.h"
#include "cov_scan.h"
#include "accum.h"

using namespace mnc;

static_assert(sizeof(mnc_variant_t) == 20, "mnc_variant_t is 4 int32 and 4 bytes (monica_amd/_capi.py: VARIANT_DTYPE)");

constexpr int PILE_ALT = MNC_PILE_PLANES - 1;   // channels of `alt`: A C G T N DEL INS
constexpr int CH_N = 4, CH_DEL = 5, CH_INS = 6;

struct mnc_pileup : Accum {
	DeviceIndex *didx = nullptr;               // the index on this device: the reference bases of the read-outs
	int n_contigs = 0;
	int64_t n_words = 0;                       // = the index's total_len
	std::vector<int64_t> off;                  // n_contigs + 1
	int32_t *track = nullptr;                  // [n_words] depth differences
	int32_t *alt = nullptr;                    // [PILE_ALT][n_words]
	int64_t *d_off = nullptr;                  // [n_contigs + 1]
	long long *cbase = nullptr;                // [n_contigs] running sum of the track before the contig (scratch)
	int64_t *tile_sums = nullptr, *tile_cnt = nullptr, *tile_voff = nullptr;   // [n_words / SC_TILE + 2] each (scratch)
	int64_t *sums2 = nullptr;                  // the scan over tile_cnt's own tile sums (scratch)
};

namespace mnc {

__device__ __forceinline__ int pile_ref(const uint32_t *seq4, int64_t o)
{
	const int c = (int)(seq4[o >> 3] >> ((o & 7) * 4) & 15u);
	return c < 4 ? c : 4;
}

// one observation at base `pos` of a contig of `len` bases: nothing is ever written outside the contig's own words
__device__ __forceinline__ void pile_put(int32_t *plane, int64_t len, int64_t pos)
{
	if (pos >= 0 && pos < len) (void)__hip_atomic_fetch_add(plane + pos, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void mnc_pile_add(Batch B, int sel, const int64_t *off, int n_contigs, int64_t n_words, int32_t *track, int32_t *alt)
{
	const int lane = lane_id();
	const uint32_t rd = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (rd >= B.n_reads) return;                              // (whole waves; the kernel has no workgroup barrier)
	const int64_t read_off = B.offsets[rd];
	const int qlen = (int)(B.offsets[rd + 1] - read_off);
	if (qlen <= 0) return;
	const uint8_t *read = B.bases + read_off;
	cov_for_records(B, rd, sel, n_contigs, [&](const mnc_reg_t &r, int64_t slot) {
		const int n_c = r.n_cigar;
		if (n_c <= 0) return;
		const int64_t coff = off[r.rid], len = off[r.rid + 1] - coff;
		int32_t *w = track + coff, *a = alt + coff;            // channel ch of base p: a[ch * n_words + p]
		const uint32_t *src = B.cig_reg + B.regdp[slot].cig_off;
		auto Q = [&](int p) -> int {                            // column p of the query side, on the hit's strand (k_export.hip)
			int at = r.rev ? r.qe - 1 - p : r.qs + p;
			at = at < 0 ? 0 : at >= qlen ? qlen - 1 : at;
			const int c = base_nt4(read[at]);
			return r.rev ? (c < 4 ? 3 - c : 4) : c;
		};
		int64_t toff = r.rs;                                   // reference position before the chunk at hand
		int qoff = 0;                                          // query columns before it
		bool open = false;                                     // a run is open: the last M / D operation so far was an M
		for (int k0 = 0; k0 < n_c; k0 += 64) {
			const int k = k0 + lane;
			const uint32_t wd = k < n_c ? src[k] : 0u;
			const int op = (int)(wd & 0xfu);
			const int l = k < n_c && op <= 2 ? (int)(wd >> 4) : 0;
			const int dt = op != 1 ? l : 0, dq = op != 2 ? l : 0;
			const int cols = op == 1 ? (l > 0) : l;              // an insertion is one column: its bases are not looked at
			const int it = cov_incl_add(dt), iq = cov_incl_add(dq), ie = cov_incl_add(cols);
			const int my_t0 = it - dt, my_q0 = qoff + iq - dq;    // (the reference offset within the chunk: toff is 64 bits)
			// ---- depth: the runs of M columns
			cov_run_step(w, len, l > 0 && op == 0, l > 0 && op == 2, toff + my_t0, open);
			// ---- the columns, one lane each
			const int total = __shfl(ie, 63);
			for (int c0 = 0; c0 < total; c0 += 64) {
				const bool valid = c0 + lane < total;
				const int c = valid ? c0 + lane : total - 1;
				int o = 0;                                          // this column's operation: the first whose inclusive count exceeds c
				for (int step = 32; step > 0; step >>= 1) {
					const int e = __shfl(ie, o + step - 1);
					if (e <= c) o += step;
				}
				const int o_end = __shfl(ie, o), o_cols = __shfl(cols, o), o_op = __shfl(op, o);
				const int q0 = __shfl(my_q0, o), t0 = __shfl(my_t0, o);
				const int x = c - (o_end - o_cols);                  // column within the operation
				const int64_t p = toff + t0 + x;
				if (!valid) continue;
				if (o_op == 0) {
					if (p >= 0 && p < len) {
						const int qc = Q(q0 + x), tc = pile_ref(B.seq4, coff + p);
						if (tc == 4 || qc != tc) pile_put(a + (int64_t)qc * n_words, len, p);
					}
				} else if (o_op == 2) pile_put(a + (int64_t)CH_DEL * n_words, len, p);
				else if (p > r.rs) pile_put(a + (int64_t)CH_INS * n_words, len, p - 1);   // a reference column of this record lies on its left
			}
			toff += __shfl(it, 63), qoff += __shfl(iq, 63);
		}
		cov_run_close(w, len, toff, open);
	});
}

// ---------------------------------------------------------------- read-outs
struct PileView {
	const int32_t *track, *alt;
	int64_t n_words;
	const uint32_t *seq4;
	const int64_t *off;
	int n_contigs;
};
struct PileThr { int min_depth, min_count, min_permille; };

// the full counts of one base: A C G T N DEL INS
struct PileBase {
	int cnt[PILE_ALT], depth, ref;
	__device__ __forceinline__ int span() const { return depth + cnt[CH_DEL]; }
	__device__ __forceinline__ int allele(int a) const { return a < 4 ? cnt[a] : cnt[a + 1]; }   // a: A C G T DEL INS
};

__device__ __forceinline__ PileBase pile_load(const PileView &P, int64_t g, int depth)
{
	PileBase b;
	for (int ch = 0; ch < PILE_ALT; ++ch) b.cnt[ch] = P.alt[(int64_t)ch * P.n_words + g];
	b.depth = depth, b.ref = pile_ref(P.seq4, g);
	if (b.ref < 4) b.cnt[b.ref] += depth - (b.cnt[0] + b.cnt[1] + b.cnt[2] + b.cnt[3] + b.cnt[CH_N]);
	return b;
}

// bit a: allele a (A C G T DEL INS) is called
__device__ __forceinline__ int pile_calls(const PileBase &b, const PileThr &t)
{
	const int span = b.span();
	if (b.ref >= 4 || span < t.min_depth) return 0;
	int m = 0;
	for (int a = 0; a < 6; ++a) {
		const int c = b.allele(a);
		if (a != b.ref && c >= t.min_count && (long long)c * 1000 >= (long long)t.min_permille * span) m |= 1 << a;
	}
	return m;
}

__device__ __forceinline__ char pile_consensus(const PileBase &b, int min_depth)
{
	if (b.span() < min_depth) return 'N';
	int mx = b.cnt[CH_DEL];
	for (int a = 0; a < 4; ++a) mx = b.cnt[a] > mx ? b.cnt[a] : mx;
	if (b.ref < 4 && b.cnt[b.ref] == mx) return "ACGT"[b.ref];
	for (int a = 0; a < 4; ++a) if (b.cnt[a] == mx) return "ACGT"[a];
	return '-';
}

// The words [w0, w0 + n) of the track, the sum starting at w0; the bases from `start` (relative to w0) on are read out.
// cbase == nullptr: the words are the first n of contig `rid`.  Otherwise they are the whole track, and a base's depth is the
// running sum minus cbase[its contig].
// MODE 0: o_counts[8][n - start]   1: tile_cnt[tile] = variants called in the tile   2: o_var, a tile's records from
// tile_voff[tile] on   3: o_cons[n - start]
template <int MODE>
__global__ __launch_bounds__(SC_THREADS) void mnc_pile_scan(PileView P, int64_t w0, int64_t n, const int64_t *tile_pre, const long long *cbase, int rid,
                                                            int64_t start, PileThr thr, int32_t *o_counts, int64_t *tile_cnt, const int64_t *tile_voff,
                                                            mnc_variant_t *o_var, int64_t var_cap, char *o_cons)
{
	__shared__ long long s[SC_THREADS / 64];
	__shared__ int s_n[SC_THREADS / 64];
	const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
	const int64_t base = (int64_t)blockIdx.x * SC_TILE + (int64_t)threadIdx.x * SC_ITEMS, m = n - start;
	int v[SC_ITEMS];
	long long x = 0;
	for (int k = 0; k < SC_ITEMS; ++k) { v[k] = base + k < n ? P.track[w0 + base + k] : 0; x += v[k]; }
	long long inc = x;
	for (int d = 1; d < 64; d <<= 1) {
		const long long o = __shfl_up(inc, d);
		if (lane >= d) inc += o;
	}
	if (lane == 63) s[wave] = inc;
	__syncthreads();
	long long pre = tile_pre[blockIdx.x] + inc - x;
	for (int w = 0; w < wave; ++w) pre += s[w];
	int c = rid;
	long long cb = 0;
	if (cbase && base < n) {                                  // the contig of this thread's first word: the last c with off[c] <= it
		int lo = 0, hi = P.n_contigs;
		while (hi - lo > 1) {
			const int mid = lo + (hi - lo) / 2;
			if (P.off[mid] <= w0 + base) lo = mid; else hi = mid;
		}
		c = lo, cb = cbase[c];
	}
	int mask[SC_ITEMS], dep[SC_ITEMS], ctg[SC_ITEMS], n_call = 0;
	for (int k = 0; k < SC_ITEMS; ++k) {
		const int64_t i = base + k;
		pre += v[k];
		mask[k] = 0, dep[k] = 0, ctg[k] = c;
		if (i >= n) continue;
		if (cbase) while (c + 1 < P.n_contigs && w0 + i >= P.off[c + 1]) { ++c; cb = cbase[c]; }
		dep[k] = (int)(pre - cb), ctg[k] = c;
		if (i < start) continue;
		const PileBase b = pile_load(P, w0 + i, dep[k]);
		if (MODE == 0) {
			o_counts[i - start] = b.depth;
			for (int ch = 0; ch < PILE_ALT; ++ch) o_counts[(int64_t)(ch + 1) * m + (i - start)] = b.cnt[ch];
		} else if (MODE == 3) o_cons[i - start] = pile_consensus(b, thr.min_depth);
		else mask[k] = pile_calls(b, thr), n_call += __popc((unsigned)mask[k]);
	}
	if (MODE == 1 || MODE == 2) {
		int inc_n = n_call;
		for (int d = 1; d < 64; d <<= 1) {
			const int o = __shfl_up(inc_n, d);
			if (lane >= d) inc_n += o;
		}
		if (lane == 63) s_n[wave] = inc_n;
		__syncthreads();
		if (MODE == 1) {
			if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (int64_t)s_n[0] + s_n[1] + s_n[2] + s_n[3];
		} else {
			int64_t at = tile_voff[blockIdx.x] + inc_n - n_call;
			for (int w = 0; w < wave; ++w) at += s_n[w];
			for (int k = 0; k < SC_ITEMS; ++k) {
				if (!mask[k]) continue;
				const int64_t g = w0 + base + k;
				const PileBase b = pile_load(P, g, dep[k]);
				for (int a = 0; a < 6; ++a) {
					if (!(mask[k] >> a & 1)) continue;
					if (at < var_cap) {
						mnc_variant_t r;
						r.rid = ctg[k], r.pos = (int32_t)(g - P.off[ctg[k]]), r.span = b.span(), r.count = b.allele(a);
						r.ref = (uint8_t)"ACGT"[b.ref], r.alt = (uint8_t)"ACGT-+"[a], r.pad[0] = r.pad[1] = 0;
						o_var[at] = r;
					}
					++at;
				}
			}
		}
	}
}

// tile sums of the words [w0, w0 + n) (exclusive, in place) and, for the whole track, the sum in front of every contig
static void pile_tile_sums(mnc_pileup *pu, int64_t w0, int64_t n, bool all)
{
	cov_tile_sums(pu->track + w0, n, pu->tile_sums, pu->d_off, pu->n_contigs, all ? pu->cbase : nullptr, pu->st);
}

template <int MODE>
static void pile_launch(mnc_pileup *pu, int64_t w0, int64_t n, bool all, int rid, int64_t start, PileThr thr, int32_t *o_counts, mnc_variant_t *o_var,
                        int64_t var_cap, char *o_cons)
{
	const PileView P{pu->track, pu->alt, pu->n_words, pu->didx->seq4, pu->d_off, pu->n_contigs};
	hipLaunchKernelGGL(mnc_pile_scan<MODE>, dim3((unsigned)((n + SC_TILE - 1) / SC_TILE)), dim3(SC_THREADS), 0, pu->st, P, w0, n, pu->tile_sums,
	                   all ? pu->cbase : nullptr, rid, start, thr, o_counts, pu->tile_cnt, pu->tile_voff, o_var, var_cap, o_cons);
}

// ---------------------------------------------------------------- the engine's side (mnc_engine_add_pileup, engine.hip)
const Accum *as_accum(const mnc_pileup *pu) { return pu; }

// the batch B, as it stands in HBM, on the engine's stream `st`; nothing waits on the host
int pileup_add(mnc_pileup *pu, const Batch &B, int sel, hipStream_t st)
{
	if (B.n_reads == 0 || pu->n_words == 0) return MNC_OK;
	return pu->add(st, [&] {
		hipLaunchKernelGGL(mnc_pile_add, dim3((B.n_reads + 3) / 4), dim3(256), 0, st, B, sel, pu->d_off, pu->n_contigs, pu->n_words, pu->track, pu->alt);
	});
}

} // namespace mnc

// ---------------------------------------------------------------- C-ABI
extern "C" void mnc_pileup_free(mnc_pileup *pu)
{
	if (!pu) return;
	pu->release();
	delete pu;
}

extern "C" int mnc_pileup_create(mnc_index *idx, int device, mnc_pileup **out)
{
	if (!idx || !out) return MNC_ERR_ARG;
	*out = nullptr;
	if (int rc = check_device(device)) return rc;
	if (idx->seq_off.size() != idx->contig_len.size() + 1) { set_error("the index holds no contig bases"); return MNC_ERR_ARG; }
	mnc_pileup *pu = new (std::nothrow) mnc_pileup;
	if (!pu) return MNC_ERR_NOMEM;
	pu->n_contigs = (int)idx->contig_len.size();
	try {
		pu->off.assign(idx->seq_off.begin(), idx->seq_off.end());   // the planes' layout is the 4-bit store's
	} catch (const std::bad_alloc &) { delete pu; return MNC_ERR_NOMEM; }
	pu->n_words = pu->off[pu->n_contigs];
	if (int rc = index_upload(idx, device, &pu->didx)) { delete pu; return rc; }
	const size_t nc = (size_t)pu->n_contigs, nw = (size_t)pu->n_words, nt = nw / SC_TILE + 2;
	hipError_t he = pu->begin(idx, device);
	pu->alloc(he, (void**)&pu->track, nw * 4);
	pu->alloc(he, (void**)&pu->alt, nw * 4 * PILE_ALT);
	pu->alloc(he, (void**)&pu->d_off, (nc + 1) * 8);
	pu->alloc(he, (void**)&pu->cbase, nc * 8);
	pu->alloc(he, (void**)&pu->tile_sums, nt * 8);
	pu->alloc(he, (void**)&pu->tile_cnt, nt * 8);
	pu->alloc(he, (void**)&pu->tile_voff, nt * 8);
	pu->alloc(he, (void**)&pu->sums2, (nt / SC_TILE + 2) * 8);
	pu->streams(he);
	if (he == hipSuccess) he = hipMemcpy(pu->d_off, pu->off.data(), (nc + 1) * 8, hipMemcpyHostToDevice);
	if (he != hipSuccess) {
		set_error("pileup accumulator of %lld bases (32 bytes each): %s", (long long)pu->n_words, hipGetErrorString(he));
		const int rc = Accum::failed(he);
		mnc_pileup_free(pu);
		return rc;
	}
	if (int rc = mnc_pileup_reset(pu)) { mnc_pileup_free(pu); return rc; }
	*out = pu;
	return MNC_OK;
}

extern "C" int mnc_pileup_reset(mnc_pileup *pu)
{
	if (!pu) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(pu->device));
	std::lock_guard<std::mutex> lk(pu->mu);
	if (pu->n_words) {
		HIP_TRY(hipMemsetAsync(pu->track, 0, (size_t)pu->n_words * 4, pu->st));
		HIP_TRY(hipMemsetAsync(pu->alt, 0, (size_t)pu->n_words * 4 * PILE_ALT, pu->st));
	}
	HIP_TRY(pu->own_done());
	return MNC_OK;
}

extern "C" int mnc_pileup_device_bytes(const mnc_pileup *pu, int64_t *bytes) { return accum_device_bytes(pu, bytes); }

extern "C" int mnc_pileup_device(mnc_pileup *pu, const int32_t **d_depth, const int32_t **d_alt, int64_t *n_words)
{
	if (!pu) return MNC_ERR_ARG;
	if (d_depth) *d_depth = pu->n_words ? pu->track : nullptr;
	if (d_alt) *d_alt = pu->n_words ? pu->alt : nullptr;
	if (n_words) *n_words = pu->n_words;
	return MNC_OK;
}

extern "C" int mnc_pileup_fetch_counts(mnc_pileup *pu, int rid, int64_t start, int64_t end, int32_t *out)
{
	if (!pu) return MNC_ERR_ARG;
	if (int rc = accum_interval(pu->off, rid, start, end)) return rc;
	if (end == start) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(pu->device));
	const size_t bytes = (size_t)(end - start) * 4 * MNC_PILE_PLANES;
	int32_t *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, bytes));
	pile_tile_sums(pu, pu->off[rid], end, false);               // the contig's words up to `end`: the sum starts at the contig
	pile_launch<0>(pu, pu->off[rid], end, false, rid, start, PileThr{0, 0, 0}, tmp, nullptr, 0, nullptr);
	return pu->finish(hipSuccess, tmp, {out, tmp, bytes}, {}, "pileup counts");
}

extern "C" int mnc_pileup_consensus(mnc_pileup *pu, int rid, int64_t start, int64_t end, int32_t min_depth, char *out)
{
	if (!pu) return MNC_ERR_ARG;
	if (int rc = accum_interval(pu->off, rid, start, end)) return rc;
	if (end == start) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(pu->device));
	char *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, (size_t)(end - start)));
	pile_tile_sums(pu, pu->off[rid], end, false);
	pile_launch<3>(pu, pu->off[rid], end, false, rid, start, PileThr{min_depth, 0, 0}, nullptr, nullptr, 0, tmp);
	return pu->finish(hipSuccess, tmp, {out, tmp, (size_t)(end - start)}, {}, "pileup consensus");
}

extern "C" int mnc_pileup_call_variants(mnc_pileup *pu, int rid, int32_t min_depth, int32_t min_count, int32_t min_permille, mnc_variant_t *out, int64_t cap, int64_t *n)
{
	if (!pu || !n) return MNC_ERR_ARG;
	*n = 0;
	if (rid < -1 || rid >= pu->n_contigs) { set_error("contig %d out of range", rid); return MNC_ERR_ARG; }
	const bool all = rid < 0;
	const int64_t w0 = all ? 0 : pu->off[rid], len = all ? pu->n_words : pu->off[rid + 1] - w0;
	if (len == 0) return MNC_OK;
	HIP_TRY(hipSetDevice(pu->device));
	const PileThr thr{min_depth, min_count, min_permille};
	const int64_t nb = (len + SC_TILE - 1) / SC_TILE;
	// ---- count, scan
	pile_tile_sums(pu, w0, len, all);
	pile_launch<1>(pu, w0, len, all, rid, 0, thr, nullptr, nullptr, 0, nullptr);
	exclusive_scan(ScanInPlain<int64_t>{pu->tile_cnt}, nb, pu->tile_voff, pu->sums2, pu->st);
	HIP_TRY(hipGetLastError());
	int64_t total = 0;
	HIP_TRY(hipMemcpyAsync(&total, pu->tile_voff + nb, 8, hipMemcpyDeviceToHost, pu->st));
	HIP_TRY(hipStreamSynchronize(pu->st));
	*n = total;
	if (cap < total) { set_error("%lld variants, room for %lld", (long long)total, (long long)cap); return MNC_ERR_RANGE; }
	if (total == 0) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	// ---- write (read-outs are for one thread at a time; should an add slip in between the passes all the same, no tile
	// writes beyond `total`)
	mnc_variant_t *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, (size_t)total * sizeof(mnc_variant_t)));
	pile_launch<2>(pu, w0, len, all, rid, 0, thr, nullptr, tmp, total, nullptr);
	return pu->finish(hipSuccess, tmp, {out, tmp, (size_t)total * sizeof(mnc_variant_t)}, {}, "pileup variants");
}
