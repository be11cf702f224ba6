// Depth and breadth of coverage per contig (include/monica_amd.h, "coverage"): an accumulator that lives across classify
// calls, added to from the last batch as it stands in HBM (regions, region CIGARs).  Runs only when asked for; nothing here
// is on the classification path.
//
// The track.  One int32 per reference base of the index, the contigs back to back without padding: base p of contig c
// is word off[c] + p, off = the prefix sums of the contig lengths.  It holds DIFFERENCES of depth: a covered run [s, e)
// adds +1 at s and -1 at e, so a run costs two atomics whatever its length and tracks of several ranks add up word by word.
// Depth of base p is the sum of the contig's words 0 .. p.
//   THE CONTIG-END RULE.  A run that ends on the last base of its contig has its -1 one past the contig -- on the first
//   base of the next one, where it would take one off that contig's depth.  That -1 is DROPPED (cov_put), not stored in a
//   slot of its own: depth is defined as a sum that starts anew at every contig, so nothing ever reads what lies beyond a
//   contig's last word, and the track stays at exactly 4 bytes per base in the layout a caller's collective expects.
//   Consequence: the words of a contig do not sum to zero, and the summary must not let one contig's sum run into the next.
//
//   mnc_cov_add_runs   one wave per READ (not per record: a read has a handful of records, cov_for_records).  Every lane
//                      walks the read's records -- the selection is decided on the way, for MNC_COV_ASSIGNED by best_hit's
//                      int64 cross-products over the gated records -- and the wave walks a selected record's CIGAR 64
//                      operations at a time: reference offsets by a prefix sum of the reference-consuming lengths, the
//                      covered runs by cov_run_step (cov_common.h).
//   mnc_cov_add_span   one lane per read: +1 at rs, -1 at re of every selected record (MNC_COV_SPAN)
//   mnc_cov_scan       the summary.  Restarting the sum at every contig needs no segmented operator: with G the plain
//                      running sum of the whole track, depth(c, p) = G(off[c] + p) - G(off[c] - 1), so scan.h's tile sums
//                      serve as they are, mnc_cov_contig_base finds every contig's G(off[c] - 1), and the pass over the
//                      tiles subtracts it.  The reductions (covered bases, depth sum, maximum; per bin for one contig's
//                      profile) are taken in that pass from registers: per-base depth is never stored, the track is only
//                      read.  A tile inside one contig -- all but a few -- reduces across its workgroup and issues three
//                      atomics; a tile that spans a contig border lets every lane flush its own.
#include <hip/hip_runtime.h>
#include <new>
#include <vector>
#include "device.h"
#include "scan.h"
#include "cov_scan.h"                          // with cov_common.h: the selectors, the record walk, the runs, the tile sums: shared with k_pileup.hip
#include "accum.h"

using namespace mnc;

struct mnc_coverage : Accum {
	int bin_bases = 0, n_contigs = 0;
	int64_t n_words = 0;                       // = the index's total_len
	std::vector<int64_t> off;                  // n_contigs + 1
	int32_t *track = nullptr;                  // [n_words] depth differences
	unsigned long long *n_aln = nullptr;       // [n_contigs] records added
	int64_t *d_off = nullptr;                  // [n_contigs + 1]
	int64_t *tile_sums = nullptr;              // [n_words / SC_TILE + 2] scratch of the summary
	long long *cbase = nullptr;                // [n_contigs] running sum of the track before the contig (scratch)
	unsigned long long *c_cov = nullptr, *c_sum = nullptr;   // [n_contigs] each: the summary's results
	int32_t *c_max = nullptr;
};

namespace mnc {

__global__ __launch_bounds__(256) void mnc_cov_add_runs(Batch B, int sel, const int64_t *off, int n_contigs, int32_t *track, unsigned long long *n_aln)
{
	const int lane = lane_id();
	const uint32_t rd = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (rd >= B.n_reads) return;                              // (whole waves; the kernel has no workgroup barrier)
	cov_for_records(B, rd, sel, n_contigs, [&](const mnc_reg_t &r, int64_t slot) {
		const int64_t len = off[r.rid + 1] - off[r.rid];
		int32_t *w = track + off[r.rid];
		if (lane == 0) (void)__hip_atomic_fetch_add(n_aln + r.rid, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		const int n_c = r.n_cigar;
		if (n_c <= 0) return;
		const uint32_t *src = B.cig_reg + B.regdp[slot].cig_off;
		int64_t toff = r.rs;                                   // reference position before the chunk at hand
		bool open = false;                                     // a run is open: the last M / D operation so far was an M
		for (int k0 = 0; k0 < n_c; k0 += 64) {
			const int k = k0 + lane;
			const uint32_t wd = k < n_c ? src[k] : 0u;
			const int op = (int)(wd & 0xfu);
			const int l = k < n_c && op <= 2 ? (int)(wd >> 4) : 0;
			const int dt = op != 1 ? l : 0;
			const int it = cov_incl_add(dt);
			cov_run_step(w, len, l > 0 && op == 0, l > 0 && op == 2, toff + it - dt, open);
			toff += __shfl(it, 63);
		}
		cov_run_close(w, len, toff, open);
	});
}

__global__ __launch_bounds__(256) void mnc_cov_add_span(Batch B, int sel, const int64_t *off, int n_contigs, int32_t *track, unsigned long long *n_aln)
{
	const uint32_t rd = blockIdx.x * blockDim.x + threadIdx.x;
	if (rd >= B.n_reads) return;
	cov_for_records(B, rd, sel, n_contigs, [&](const mnc_reg_t &r, int64_t) {
		const int64_t len = off[r.rid + 1] - off[r.rid];
		int32_t *w = track + off[r.rid];
		(void)__hip_atomic_fetch_add(n_aln + r.rid, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (r.re > r.rs) cov_put(w, len, r.rs, 1), cov_put(w, len, r.re, -1);
	});
}

struct CovAcc {
	int cov = 0, mx = 0, cnt = 0;
	long long sum = 0;
	__device__ __forceinline__ void add(int d) { cov += d > 0, sum += d, mx = d > mx ? d : mx, ++cnt; }
};

// MODE 0: the whole track, per-contig reductions.  MODE 1: the words of ONE contig (track points at its first), per-bin
// reductions.  MODE 2: the first n words of one contig, depth of the words from `start` on written out.
template <int MODE>
__global__ __launch_bounds__(SC_THREADS) void mnc_cov_scan(const int32_t *track, int64_t n, const int64_t *tile_pre, const int64_t *off, int n_contigs,
                                                           const long long *cbase, unsigned long long *o_cov, unsigned long long *o_sum, int32_t *o_max,
                                                           int bin_bases, int32_t *b_cov, int64_t start, int32_t *depth)
{
	__shared__ long long s[SC_THREADS / 64];
	__shared__ int s_c0;
	__shared__ long long s_sum[SC_THREADS / 64];
	__shared__ int s_cov[SC_THREADS / 64], s_max[SC_THREADS / 64];
	const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
	const int64_t tile0 = (int64_t)blockIdx.x * SC_TILE, base = tile0 + (int64_t)threadIdx.x * SC_ITEMS;
	const int64_t tile_end = tile0 + SC_TILE < n ? tile0 + SC_TILE : n;
	int v[SC_ITEMS];
	long long x = 0;
	for (int k = 0; k < SC_ITEMS; ++k) { v[k] = base + k < n ? track[base + k] : 0; x += v[k]; }
	long long inc = x;
	for (int d = 1; d < 64; d <<= 1) {
		const long long o = __shfl_up(inc, d);
		if (lane >= d) inc += o;
	}
	if (lane == 63) s[wave] = inc;
	if (MODE == 0 && threadIdx.x == 0) {                       // the contig of the tile's first word: the last c with off[c] <= tile0
		int lo = 0, hi = n_contigs;
		while (hi - lo > 1) {
			const int mid = lo + (hi - lo) / 2;
			if (off[mid] <= tile0) lo = mid; else hi = mid;
		}
		s_c0 = lo;
	}
	__syncthreads();
	long long pre = tile_pre[blockIdx.x] + inc - x;
	for (int w = 0; w < wave; ++w) pre += s[w];
	if (MODE == 0) {
		const int c0 = s_c0;
		if (tile_end <= off[c0 + 1]) {                            // (the same for the whole workgroup) the tile lies in one contig
			const long long cb = cbase[c0];
			CovAcc a;
			for (int k = 0; k < SC_ITEMS; ++k) { pre += v[k]; if (base + k < n) a.add((int)(pre - cb)); }
			for (int d = 32; d > 0; d >>= 1) {
				a.cov += __shfl_xor(a.cov, d), a.sum += __shfl_xor(a.sum, d);
				const int m = __shfl_xor(a.mx, d);
				a.mx = m > a.mx ? m : a.mx;
			}
			if (lane == 0) s_cov[wave] = a.cov, s_sum[wave] = a.sum, s_max[wave] = a.mx;
			__syncthreads();
			if (threadIdx.x == 0) {
				int cov = 0, mx = 0;
				long long sum = 0;
				for (int w = 0; w < SC_THREADS / 64; ++w) cov += s_cov[w], sum += s_sum[w], mx = s_max[w] > mx ? s_max[w] : mx;
				if (cov) (void)atomicAdd(o_cov + c0, (unsigned long long)cov);
				if (sum) (void)atomicAdd(o_sum + c0, (unsigned long long)sum);
				if (mx > 0) (void)atomicMax(o_max + c0, mx);
			}
		} else if (base < n) {                                    // a contig border inside the tile: every lane for itself
			int lo = 0, hi = n_contigs;
			while (hi - lo > 1) {
				const int mid = lo + (hi - lo) / 2;
				if (off[mid] <= base) lo = mid; else hi = mid;
			}
			int c = lo;
			CovAcc a;
			auto flush = [&]() {
				if (a.cov) (void)atomicAdd(o_cov + c, (unsigned long long)a.cov);
				if (a.sum) (void)atomicAdd(o_sum + c, (unsigned long long)a.sum);
				if (a.mx > 0) (void)atomicMax(o_max + c, a.mx);
				a = CovAcc();
			};
			long long cb = cbase[c];
			for (int k = 0; k < SC_ITEMS && base + k < n; ++k) {
				while (c + 1 < n_contigs && base + k >= off[c + 1]) { flush(); ++c; cb = cbase[c]; }
				pre += v[k];
				a.add((int)(pre - cb));
			}
			flush();
		}
	} else if (MODE == 1) {
		// a wave whose 256 words lie in one bin -- most, at the usual widths -- reduces first
		const int64_t w_first = tile0 + (int64_t)wave * 64 * SC_ITEMS, w_last = (w_first + 64 * SC_ITEMS < n ? w_first + 64 * SC_ITEMS : n) - 1;
		if (w_first < n && w_first / bin_bases == w_last / bin_bases) {
			CovAcc a;
			for (int k = 0; k < SC_ITEMS; ++k) { pre += v[k]; if (base + k < n) a.add((int)pre); }
			for (int d = 32; d > 0; d >>= 1) a.cov += __shfl_xor(a.cov, d), a.sum += __shfl_xor(a.sum, d);
			if (lane == 0) {
				const int64_t b = w_first / bin_bases;
				if (a.cov) (void)atomicAdd(b_cov + b, a.cov);
				if (a.sum) (void)atomicAdd(o_sum + b, (unsigned long long)a.sum);
			}
		} else if (base < n) {
			int64_t b = base / bin_bases;
			CovAcc a;
			for (int k = 0; k < SC_ITEMS && base + k < n; ++k) {
				const int64_t bk = (base + k) / bin_bases;
				if (bk != b) {
					if (a.cov) (void)atomicAdd(b_cov + b, a.cov);
					if (a.sum) (void)atomicAdd(o_sum + b, (unsigned long long)a.sum);
					a = CovAcc(), b = bk;
				}
				pre += v[k];
				a.add((int)pre);
			}
			if (a.cov) (void)atomicAdd(b_cov + b, a.cov);
			if (a.sum) (void)atomicAdd(o_sum + b, (unsigned long long)a.sum);
		}
	} else {
		for (int k = 0; k < SC_ITEMS; ++k) {
			pre += v[k];
			if (base + k < n && base + k >= start) depth[base + k - start] = (int32_t)pre;
		}
	}
}

// tile sums of track[0 .. n) (exclusive, in place), then the pass of MODE over the tiles
template <int MODE>
static void cov_launch_scan(mnc_coverage *cv, const int32_t *track, int64_t n, int32_t *b_cov, unsigned long long *b_sum, int64_t start, int32_t *depth)
{
	cov_tile_sums(track, n, cv->tile_sums, cv->d_off, cv->n_contigs, MODE == 0 ? cv->cbase : nullptr, cv->st);
	hipLaunchKernelGGL(mnc_cov_scan<MODE>, dim3((unsigned)((n + SC_TILE - 1) / SC_TILE)), dim3(SC_THREADS), 0, cv->st, track, n, cv->tile_sums, cv->d_off, cv->n_contigs, cv->cbase,
	                   MODE == 0 ? cv->c_cov : nullptr, MODE == 0 ? cv->c_sum : b_sum, MODE == 0 ? cv->c_max : nullptr, cv->bin_bases, b_cov, start, depth);
}

// ---------------------------------------------------------------- the engine's side (mnc_engine_add_coverage, engine.hip)
const Accum *as_accum(const mnc_coverage *cv) { return cv; }

// the batch B, as it stands in HBM, on the engine's stream `st`; nothing waits on the host
int coverage_add(mnc_coverage *cv, const Batch &B, int sel, bool span, hipStream_t st)
{
	if (B.n_reads == 0 || cv->n_words == 0) return MNC_OK;
	return cv->add(st, [&] {
		if (span) hipLaunchKernelGGL(mnc_cov_add_span, dim3((B.n_reads + 255) / 256), dim3(256), 0, st, B, sel, cv->d_off, cv->n_contigs, cv->track, cv->n_aln);
		else hipLaunchKernelGGL(mnc_cov_add_runs, dim3((B.n_reads + 3) / 4), dim3(256), 0, st, B, sel, cv->d_off, cv->n_contigs, cv->track, cv->n_aln);
	});
}

} // namespace mnc

// ---------------------------------------------------------------- C-ABI
extern "C" void mnc_coverage_free(mnc_coverage *cv)
{
	if (!cv) return;
	cv->release();
	delete cv;
}

extern "C" int mnc_coverage_create(mnc_index *idx, int device, int bin_bases, mnc_coverage **out)
{
	if (!idx || !out) return MNC_ERR_ARG;
	*out = nullptr;
	if (bin_bases < 1) { set_error("bin_bases must be 1 or more"); return MNC_ERR_ARG; }
	if (int rc = check_device(device)) return rc;
	mnc_coverage *cv = new (std::nothrow) mnc_coverage;
	if (!cv) return MNC_ERR_NOMEM;
	cv->bin_bases = bin_bases, cv->n_contigs = (int)idx->contig_len.size();
	try {
		cv->off.assign((size_t)cv->n_contigs + 1, 0);
	} catch (const std::bad_alloc &) { delete cv; return MNC_ERR_NOMEM; }
	for (int c = 0; c < cv->n_contigs; ++c) cv->off[c + 1] = cv->off[c] + idx->contig_len[c];
	cv->n_words = cv->off[cv->n_contigs];
	const size_t nc = (size_t)cv->n_contigs, nw = (size_t)cv->n_words;
	hipError_t he = cv->begin(idx, device);
	cv->alloc(he, (void**)&cv->track, nw * 4);
	cv->alloc(he, (void**)&cv->n_aln, nc * 8);
	cv->alloc(he, (void**)&cv->d_off, (nc + 1) * 8);
	cv->alloc(he, (void**)&cv->tile_sums, (nw / SC_TILE + 2) * 8);
	cv->alloc(he, (void**)&cv->cbase, nc * 8);
	cv->alloc(he, (void**)&cv->c_cov, nc * 8);
	cv->alloc(he, (void**)&cv->c_sum, nc * 8);
	cv->alloc(he, (void**)&cv->c_max, nc * 4);
	cv->streams(he);
	if (he == hipSuccess) he = hipMemcpy(cv->d_off, cv->off.data(), (nc + 1) * 8, hipMemcpyHostToDevice);
	if (he != hipSuccess) {
		set_error("coverage accumulator of %lld bases: %s", (long long)cv->n_words, hipGetErrorString(he));
		const int rc = Accum::failed(he);
		mnc_coverage_free(cv);
		return rc;
	}
	if (int rc = mnc_coverage_reset(cv)) { mnc_coverage_free(cv); return rc; }
	*out = cv;
	return MNC_OK;
}

extern "C" int mnc_coverage_reset(mnc_coverage *cv)
{
	if (!cv) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(cv->device));
	std::lock_guard<std::mutex> lk(cv->mu);
	if (cv->n_words) HIP_TRY(hipMemsetAsync(cv->track, 0, (size_t)cv->n_words * 4, cv->st));
	if (cv->n_contigs) HIP_TRY(hipMemsetAsync(cv->n_aln, 0, (size_t)cv->n_contigs * 8, cv->st));
	HIP_TRY(cv->own_done());
	return MNC_OK;
}

extern "C" int mnc_coverage_device_bytes(const mnc_coverage *cv, int64_t *bytes) { return accum_device_bytes(cv, bytes); }

extern "C" int mnc_coverage_summary(mnc_coverage *cv, int64_t *covered, int64_t *depth_sum, int32_t *max_depth, int64_t *n_aln)
{
	if (!cv) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(cv->device));
	const size_t nc = (size_t)cv->n_contigs;
	hipStream_t st = cv->st;
	if (nc && (covered || depth_sum || max_depth)) {
		HIP_TRY(hipMemsetAsync(cv->c_cov, 0, nc * 8, st));
		HIP_TRY(hipMemsetAsync(cv->c_sum, 0, nc * 8, st));
		HIP_TRY(hipMemsetAsync(cv->c_max, 0, nc * 4, st));
		if (cv->n_words) cov_launch_scan<0>(cv, cv->track, cv->n_words, nullptr, nullptr, 0, nullptr);
		HIP_TRY(hipGetLastError());
		if (covered) HIP_TRY(hipMemcpyAsync(covered, cv->c_cov, nc * 8, hipMemcpyDeviceToHost, st));
		if (depth_sum) HIP_TRY(hipMemcpyAsync(depth_sum, cv->c_sum, nc * 8, hipMemcpyDeviceToHost, st));
		if (max_depth) HIP_TRY(hipMemcpyAsync(max_depth, cv->c_max, nc * 4, hipMemcpyDeviceToHost, st));
	}
	if (nc && n_aln) HIP_TRY(hipMemcpyAsync(n_aln, cv->n_aln, nc * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return MNC_OK;
}

extern "C" int mnc_coverage_fetch_bins(mnc_coverage *cv, int rid, int32_t *bin_covered, int64_t *bin_depth_sum, int64_t cap, int64_t *n_bins)
{
	if (!cv || !n_bins) return MNC_ERR_ARG;
	if (rid < 0 || rid >= cv->n_contigs) { set_error("contig %d out of range", rid); return MNC_ERR_ARG; }
	const int64_t len = cv->off[rid + 1] - cv->off[rid], nb = (len + cv->bin_bases - 1) / cv->bin_bases;
	*n_bins = nb;
	if (cap < nb) { set_error("contig %d has %lld bins of %d bases", rid, (long long)nb, cv->bin_bases); return MNC_ERR_RANGE; }
	if (nb == 0) return MNC_OK;
	HIP_TRY(hipSetDevice(cv->device));
	char *tmp = nullptr;                                        // [nb] depth sums, then [nb] covered bases
	HIP_TRY(hipMalloc((void**)&tmp, (size_t)nb * 12));
	const hipError_t he = hipMemsetAsync(tmp, 0, (size_t)nb * 12, cv->st);
	if (he == hipSuccess) cov_launch_scan<1>(cv, cv->track + cv->off[rid], len, (int32_t*)(tmp + (size_t)nb * 8), (unsigned long long*)tmp, 0, nullptr);
	return cv->finish(he, tmp, {bin_depth_sum, tmp, (size_t)nb * 8}, {bin_covered, tmp + (size_t)nb * 8, (size_t)nb * 4}, "bins of contig %d", rid);
}

extern "C" int mnc_coverage_fetch_depth(mnc_coverage *cv, int rid, int64_t start, int64_t end, int32_t *depth)
{
	if (!cv) return MNC_ERR_ARG;
	if (int rc = accum_interval(cv->off, rid, start, end)) return rc;
	if (end == start) return MNC_OK;
	if (!depth) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(cv->device));
	int32_t *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, (size_t)(end - start) * 4));
	cov_launch_scan<2>(cv, cv->track + cv->off[rid], end, nullptr, nullptr, start, tmp);   // the contig's words up to `end`: the sum starts at the contig
	return cv->finish(hipSuccess, tmp, {depth, tmp, (size_t)(end - start) * 4}, {}, "depth of contig %d", rid);
}

extern "C" int mnc_coverage_device(mnc_coverage *cv, const int32_t **d_track, int64_t *n_words)
{
	if (!cv) return MNC_ERR_ARG;
	if (d_track) *d_track = cv->n_words ? cv->track : nullptr;
	if (n_words) *n_words = cv->n_words;
	return MNC_OK;
}
