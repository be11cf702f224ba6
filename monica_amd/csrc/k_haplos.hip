// Local haplotypes (include/monica_amd.h, "haplos"): how often the reads spell each of the 2^k allele patterns over k
// CONSECUTIVE sites of a caller's list -- hap[n_sites][2^k], row i the window of sites i .. i + k - 1.  Two strains leave two
// frequent patterns in every window, three strains three wherever their differences interleave; the pair tables of
// k_linkage.hip cannot count them.  A sibling of k_linkage.hip: an accumulator of accum.h over the site list of linkage.h,
// the sixth consumer of a batch as it stands in HBM; runs only when asked for.
//
//   mnc_haplos_add  one wave per READ, four per workgroup, no workgroup barrier, no LDS, no scratch.  The walk is linkage.h's
//                   link_walk: the lanes hold SITES, 64 at a time, and two ballots make their statements two masks, REF and
//                   ALT.  Each lane owns the window that ENDS at its site: with the masks of the 64 sites before it shifts the
//                   128 bits so that its own site is bit 63 and the site t in front of it bit 63 - t -- a window that straddles
//                   a 64-site border of a record costs nothing extra, the carried state is the two masks.  "All k have a
//                   statement" is one compare of the top k bits of REF | ALT; the pattern (first site first) is the bit-reverse
//                   of ALT under the k-bit mask.  A lane acts only when its window starts inside the record's range of sites.
//   the words       one atomic per (record, window) would mostly land on the all-REF cell.  That cell is DERIVED, as the
//                   linkage derives REF / REF: the windows inside a record's range of sites are a run of i, +1 / -1 in a
//                   difference track[n_sites] (two atomics a record, by one lane), and a window of the run costs its one atomic
//                   only where it is not all-REF: on word 0 of its row ("missing") where a site has no statement, else on
//                   word p.  So at most ONE atomic per lane and chunk, against up to `window` in mnc_link_add.  On read-out
//                   hap[i][0] = (track[0] + .. + track[i]) - (the sum of row i).  Every word stays additive.
//   read-outs       scan.h's exclusive scan over the track (a single column), then the lanes of a wave lie on (window,
//                   pattern): 64 >> k windows per wave, each a group of 2^k neighbouring lanes, so a wave reads 64 consecutive
//                   words.  The row's sum is a butterfly of k shuffles inside the group.
//     mnc_haplos_table  fetch: cell 0 from the running sum and the butterfly, the others as stored.
//     mnc_haplos_call_k a workgroup takes HC_TILE = 1024 cells in four sweeps.  total = running sum - missing; "called" is
//                   one ballot, n_haps a popcount under the group's mask.  Count (MODE 1: n_haps, total, the histogram, the
//                   tile's number of records), scan.h over the tiles, place (MODE 2: a wave's records go behind those of the
//                   waves and sweeps before it, a lane's behind the called lanes below it -- (window, pattern) order), as
//                   mnc_pileup_call_variants does; only the answer travels.  The histogram: a contig's windows are contiguous,
//                   so a workgroup counts the windows of its first window's contig in eight LDS words and adds the non-zero
//                   ones at its end -- at most eight global atomics a workgroup, plus one per window of a further contig that
//                   begins inside the tile.
// Integer arithmetic throughout.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <new>
#include "linkage.h"

using namespace mnc;

struct mnc_haplos : mnc::Accum {
	int64_t n_sites = 0;
	int k = 0, n_contigs = 0;
	LinkSitesDev list;                         // the sites' positions and alleles, the contigs' first sites and first bases (linkage.h)
	int32_t *d_rid = nullptr;                  // [n_sites] the sites' contigs
	int32_t *row = nullptr;                    // [n_sites][1 << k]: missing, then the patterns 1 ..; behind them track[n_sites]
	int32_t *track = nullptr;
	int64_t words() const { return n_sites * ((1ll << k) + 1); }   // of `row` and `track` together
	// scratch of the read-outs
	int64_t *runs = nullptr;                   // [n_sites + 1] the scan of the track
	int64_t *sums = nullptr;                   // the scans' tile sums
	int64_t *tile_cnt = nullptr, *tile_voff = nullptr;   // [tiles + 1] each: the records per tile of the call, and where they go
	unsigned long long *hist = nullptr;        // [n_contigs][8]
	int32_t *o_total = nullptr;                // [n_sites]
	uint8_t *o_nhaps = nullptr;                // [n_sites]
};

namespace mnc {

constexpr int HC_THREADS = 256, HC_SWEEPS = 4, HC_TILE = HC_THREADS * HC_SWEEPS;   // mnc_haplos_call_k: cells per workgroup

struct HaplosView {
	LinkSites list;
	int k;
	int32_t *row, *track;
};

// the walk is linkage.h's; here, what is done with the 64 statements it hands over
__global__ __launch_bounds__(256) void mnc_haplos_add(Batch B, int sel, HaplosView H)
{
	const int lane = lane_id(), K = H.k;
	const uint32_t rd = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (rd >= B.n_reads) return;                              // (whole waves; the kernel has no workgroup barrier)
	const unsigned long long full = ~0ull << (64 - K);        // the window of a lane: the top K bits
	int s_lo = 0;
	unsigned long long p_ref = 0, p_alt = 0;                  // the statements of the 64 sites before
	link_walk(B, rd, sel, H.list, [&](int lo, int s_hi) {
		s_lo = lo, p_ref = p_alt = 0;
		// ---- the windows inside the record's range: the run of i is [s_lo, s_hi - K + 1), and s_hi - K + 1 <= n_sites - 1
		if (lane == 0 && s_hi - lo >= K) {
			link_put(H.track + lo, 1);
			link_put(H.track + (s_hi - K + 1), -1);
		}
	}, [&](int, int s, bool valid, int stmt) {
		const unsigned long long c_ref = __ballot(stmt == 1), c_alt = __ballot(stmt == 2);
		if (valid && s - s_lo >= K - 1) {                        // the window that ends here starts inside the record's range
			// sites s - 63 .. s as bits 0 .. 63: site s - t is bit 63 - t
			const unsigned long long v_ref = lane < 63 ? (p_ref >> (lane + 1)) | (c_ref << (63 - lane)) : c_ref;
			const unsigned long long v_alt = lane < 63 ? (p_alt >> (lane + 1)) | (c_alt << (63 - lane)) : c_alt;
			const int p = (int)(__brevll(v_alt & full));           // first site first: site s - K + 1 is bit K - 1
			int32_t *w = H.row + ((int64_t)(s - K + 1) << K);
			if (((v_ref | v_alt) & full) != full) link_put(w, 1);  // missing
			else if (p) link_put(w + p, 1);                        // (all-REF is derived)
		}
		p_ref = c_ref, p_alt = c_alt;
	});
}

// ---------------------------------------------------------------- read-outs
// runs: the exclusive scan over the track, so the running sum up to and with window i is runs[i + 1].
// The n_cells cells from first_cell on (a multiple of 2^k), one thread each; a group of 2^k lanes holds one row.
__global__ __launch_bounds__(256) void mnc_haplos_table(const int32_t *row, const int64_t *runs, int k, int64_t first_cell, int64_t n_cells, int32_t *out)
{
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int G = 1 << k, p = lane_id() & (G - 1);
	const bool in = t < n_cells;
	const int w = in ? row[first_cell + t] : 0;
	long long sum = w;
	for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
	if (in) out[t] = p ? w : (int32_t)(runs[((first_cell + t) >> k) + 1] - sum);
}

struct HaplosCall {
	const int32_t *row, *rid;
	const int64_t *runs;
	int64_t n_sites;
	int k, min_total, min_count, min_permille;
};

// MODE 1: n_haps[], total[], hist[][8] and tile_cnt[tile] = the records of the tile.  MODE 2: the records, a tile's from
// tile_voff[tile] on, none at or beyond `cap`.
template <int MODE>
__global__ __launch_bounds__(HC_THREADS) void mnc_haplos_call_k(HaplosCall H, uint8_t *n_haps, int32_t *total, unsigned long long *hist, int64_t *tile_cnt,
                                                                const int64_t *tile_voff, mnc_haplo_t *out, int64_t cap)
{
	__shared__ int s_n[HC_THREADS / 64];
	__shared__ int s_hist[8];
	const int lane = lane_id(), wave = (int)(threadIdx.x >> 6), G = 1 << H.k, p = lane & (G - 1);
	const unsigned long long gm = G == 64 ? ~0ull : ((1ull << G) - 1ull) << (lane - p);   // the lanes of this lane's window
	const int64_t cells = H.n_sites << H.k, base = (int64_t)blockIdx.x * HC_TILE;          // (base < cells: the grid is the tiles)
	const int c0 = H.rid[base >> H.k];
	if (MODE == 1) {
		if (threadIdx.x < 8) s_hist[threadIdx.x] = 0;
		__syncthreads();
	}
	int64_t at = MODE == 2 ? tile_voff[blockIdx.x] : 0;
	int n_wave = 0;
	for (int sw = 0; sw < HC_SWEEPS; ++sw) {                    // (every thread runs every sweep: the barriers are the workgroup's)
		const int64_t t = base + sw * HC_THREADS + threadIdx.x, i = t >> H.k;
		const bool in = t < cells;
		const int w = in ? H.row[t] : 0;
		long long sum = w;
		for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
		const long long run = in ? H.runs[i + 1] : 0, tot = run - __shfl(w, lane - p);   // all that spelled it: the run less the missing
		const long long cnt = p ? w : run - sum;
		const bool judged = in && tot >= H.min_total && tot > 0;
		const bool called = judged && cnt >= H.min_count && cnt * 1000 >= (long long)H.min_permille * tot;
		const unsigned long long cm = __ballot(called);
		if (MODE == 1) {
			n_wave += __popcll(cm);
			if (in && p == 0) {
				const int h = __popcll(cm & gm), c = H.rid[i];
				n_haps[i] = (uint8_t)h, total[i] = (int32_t)tot;
				if (judged && c == c0) atomicAdd(&s_hist[h < 7 ? h : 7], 1);
				else if (judged) atomicAdd(hist + (int64_t)c * 8 + (h < 7 ? h : 7), 1ull);
			}
		} else {
			if (lane == 0) s_n[wave] = __popcll(cm);
			__syncthreads();
			int64_t my = at + __popcll(cm & ((1ull << lane) - 1ull));
			for (int x = 0; x < wave; ++x) my += s_n[x];
			if (called && my < cap) out[my] = mnc_haplo_t{(int32_t)i, p, (int32_t)cnt, (int32_t)tot};
			at += s_n[0] + s_n[1] + s_n[2] + s_n[3];
			__syncthreads();
		}
	}
	if (MODE == 1) {
		if (lane == 0) s_n[wave] = n_wave;
		__syncthreads();
		if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (int64_t)s_n[0] + s_n[1] + s_n[2] + s_n[3];
		if (threadIdx.x < 8 && s_hist[threadIdx.x]) atomicAdd(hist + (int64_t)c0 * 8 + threadIdx.x, (unsigned long long)s_hist[threadIdx.x]);
	}
}

// ---------------------------------------------------------------- the engine's side (mnc_engine_add_haplos, engine.hip)
const Accum *as_accum(const mnc_haplos *hp) { return hp; }

int haplos_add(mnc_haplos *hp, const Batch &B, int sel, hipStream_t st)
{
	if (B.n_reads == 0 || hp->n_sites == 0) return MNC_OK;
	const HaplosView H{hp->list.view(hp->n_contigs), hp->k, hp->row, hp->track};
	return hp->add(st, [&] { hipLaunchKernelGGL(mnc_haplos_add, dim3((B.n_reads + 3) / 4), dim3(256), 0, st, B, sel, H); });
}

} // namespace mnc

// ---------------------------------------------------------------- C-ABI
extern "C" void mnc_haplos_free(mnc_haplos *hp)
{
	if (!hp) return;
	hp->release();
	delete hp;
}

extern "C" int mnc_haplos_create(mnc_index *idx, int device, const mnc_variant_t *sites, int64_t n_sites, int32_t k, mnc_haplos **out)
{
	if (!idx || !out) return MNC_ERR_ARG;
	*out = nullptr;
	if (n_sites < 0 || (n_sites && !sites)) return MNC_ERR_ARG;
	if (k < 2 || k > MNC_HAPLOS_MAX_K) { set_error("k %d outside 2 .. %d", (int)k, MNC_HAPLOS_MAX_K); return MNC_ERR_ARG; }
	LinkSitesHost H;
	if (int rc = link_sites_check(idx, sites, n_sites, H)) return rc;
	mnc_haplos *hp = new (std::nothrow) mnc_haplos;
	if (!hp) return MNC_ERR_NOMEM;
	if (int rc = check_device(device)) { delete hp; return rc; }
	hp->n_sites = n_sites, hp->k = k, hp->n_contigs = H.n_contigs;
	const size_t ns = (size_t)n_sites, nw = (size_t)hp->words(), tiles = ((ns << k) + HC_TILE - 1) / HC_TILE;
	hipError_t he = hp->begin(idx, device);
	hp->list.alloc(*hp, he, H);
	hp->alloc(he, (void**)&hp->d_rid, ns * 4);
	hp->alloc(he, (void**)&hp->row, nw * 4);
	hp->alloc(he, (void**)&hp->runs, (ns + 1) * 8);
	hp->alloc(he, (void**)&hp->sums, (ns / SC_TILE + 2) * 8);    // (the tiles of the call are fewer than the sites)
	hp->alloc(he, (void**)&hp->tile_cnt, (tiles + 1) * 8);
	hp->alloc(he, (void**)&hp->tile_voff, (tiles + 1) * 8);
	hp->alloc(he, (void**)&hp->hist, (size_t)H.n_contigs * 64);
	hp->alloc(he, (void**)&hp->o_total, ns * 4);
	hp->alloc(he, (void**)&hp->o_nhaps, ns);
	hp->streams(he);
	if (he == hipSuccess) hp->track = hp->row + (ns << k);
	hp->list.fill(he, H);
	if (he == hipSuccess && ns) he = hipMemcpy(hp->d_rid, H.rid.data(), ns * 4, hipMemcpyHostToDevice);
	if (he != hipSuccess) {
		set_error("haplos accumulator of %lld sites, k %d (%d bytes a site): %s", (long long)n_sites, (int)k, 4 * (1 << k) + 27, hipGetErrorString(he));
		const int rc = Accum::failed(he);
		mnc_haplos_free(hp);
		return rc;
	}
	if (int rc = mnc_haplos_reset(hp)) { mnc_haplos_free(hp); return rc; }
	*out = hp;
	return MNC_OK;
}

extern "C" int mnc_haplos_reset(mnc_haplos *hp)
{
	if (!hp) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(hp->device));
	std::lock_guard<std::mutex> g(hp->mu);
	if (hp->n_sites) HIP_TRY(hipMemsetAsync(hp->row, 0, (size_t)hp->words() * 4, hp->st));
	HIP_TRY(hp->own_done());
	return MNC_OK;
}

extern "C" int mnc_haplos_device_bytes(const mnc_haplos *hp, int64_t *bytes) { return accum_device_bytes(hp, bytes); }

extern "C" int mnc_haplos_device(mnc_haplos *hp, const int32_t **d_words)
{
	if (!hp) return MNC_ERR_ARG;
	if (d_words) *d_words = hp->n_sites ? hp->row : nullptr;
	return MNC_OK;
}

extern "C" int mnc_haplos_fetch(mnc_haplos *hp, int64_t first, int64_t n, int32_t *out)
{
	if (!hp) return MNC_ERR_ARG;
	if (first < 0 || n < 0 || first > hp->n_sites || n > hp->n_sites - first) {
		set_error("windows [%lld, %lld) outside the list of %lld", (long long)first, (long long)(first + n), (long long)hp->n_sites);
		return MNC_ERR_ARG;
	}
	if (n == 0) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(hp->device));
	const int64_t n_cells = n << hp->k;
	int32_t *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, (size_t)n_cells * 4));
	exclusive_scan(ScanInPlain<int32_t>{hp->track}, hp->n_sites, hp->runs, hp->sums, hp->st);
	hipLaunchKernelGGL(mnc_haplos_table, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, hp->st, hp->row, hp->runs, hp->k, first << hp->k, n_cells, tmp);
	return hp->finish(hipSuccess, tmp, {out, tmp, (size_t)n_cells * 4}, {}, "haplotype table");
}

extern "C" int mnc_haplos_call(mnc_haplos *hp, int32_t min_total, int32_t min_count, int32_t min_permille, uint8_t *n_haps, int32_t *total, int64_t *hist,
                               mnc_haplo_t *out, int64_t cap, int64_t *n)
{
	if (!hp) return MNC_ERR_ARG;
	if (n) *n = 0;
	const int64_t ns = hp->n_sites;
	const size_t b_hist = (size_t)hp->n_contigs * 64;
	if (ns == 0) {
		if (hist) std::fill(hist, hist + (size_t)hp->n_contigs * 8, (int64_t)0);
		return MNC_OK;
	}
	HIP_TRY(hipSetDevice(hp->device));
	const unsigned tiles = (unsigned)(((ns << hp->k) + HC_TILE - 1) / HC_TILE);
	const HaplosCall H{hp->row, hp->d_rid, hp->runs, ns, hp->k, min_total, min_count, min_permille};
	// ---- count, scan
	exclusive_scan(ScanInPlain<int32_t>{hp->track}, ns, hp->runs, hp->sums, hp->st);
	HIP_TRY(hipMemsetAsync(hp->hist, 0, b_hist, hp->st));
	hipLaunchKernelGGL(mnc_haplos_call_k<1>, dim3(tiles), dim3(HC_THREADS), 0, hp->st, H, hp->o_nhaps, hp->o_total, hp->hist, hp->tile_cnt, hp->tile_voff, nullptr, 0);
	exclusive_scan(ScanInPlain<int64_t>{hp->tile_cnt}, tiles, hp->tile_voff, hp->sums, hp->st);
	HIP_TRY(hipGetLastError());
	int64_t found = 0;
	HIP_TRY(hipMemcpyAsync(&found, hp->tile_voff + tiles, 8, hipMemcpyDeviceToHost, hp->st));
	HIP_TRY(hipStreamSynchronize(hp->st));
	if (n) *n = found;
	if ((out || n) && cap < found) { set_error("%lld haplotype records, room for %lld", (long long)found, (long long)cap); return MNC_ERR_RANGE; }
	// ---- place (read-outs are for one thread at a time; should an add slip in between the passes all the same, no tile
	// writes beyond `found`)
	mnc_haplo_t *tmp = nullptr;
	if (out && found) {
		HIP_TRY(hipMalloc((void**)&tmp, (size_t)found * sizeof(mnc_haplo_t)));
		hipLaunchKernelGGL(mnc_haplos_call_k<2>, dim3(tiles), dim3(HC_THREADS), 0, hp->st, H, nullptr, nullptr, nullptr, nullptr, hp->tile_voff, tmp, found);
	}
	hipError_t e = hipGetLastError();
	if (e == hipSuccess && n_haps) e = hipMemcpyAsync(n_haps, hp->o_nhaps, (size_t)ns, hipMemcpyDeviceToHost, hp->st);
	if (e == hipSuccess && total) e = hipMemcpyAsync(total, hp->o_total, (size_t)ns * 4, hipMemcpyDeviceToHost, hp->st);
	return hp->finish(e, tmp, {hist, hp->hist, b_hist}, {tmp ? out : nullptr, tmp, (size_t)found * sizeof(mnc_haplo_t)}, "haplotype calls");
}
