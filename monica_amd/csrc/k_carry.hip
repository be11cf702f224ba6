// The candidate carry (include/monica_amd.h, "candidate carry"): read identity across the parts of a database, for the
// abundance accumulator.  One row per read of a sample, addressed by the read's ordinal in the sample: the largest score any
// part has given the read, and up to `width` (global genome id, score) pairs.  Every part's batches are merged into the rows
// as they stand in HBM; after the last part mnc_abundance_add_carry (k_abundance.hip) takes each row as one read.  Runs only
// when asked for; nothing here is on the classification path.
//
//   mnc_carry_merge_k  one wave per READ, whole waves, no workgroup barrier.  The row lives in registers, one slot per lane
//                      (so width <= 64).  What comes in -- <SRC_BATCH> the read's genomes out of the batch, in ascending id by
//                      ab_next's wave-minimum rounds (ab_common.h, shared with mnc_ab_collect); <SRC_CSR> a row of a device
//                      CSR staged by mnc_carry_add_lists; <SRC_CARRY> the same row of another carry -- goes through one body:
//                        best := max(best, the incoming scores), known BEFORE any pair is placed: the batch gives it by
//                        ab_best, a CSR row by a wave maximum, a carry by its head;
//                        the row is cut at best - max_delta, which frees lanes; incoming pairs beyond the cut are passed over;
//                        per incoming pair: a ballot on equal genome, then a max; else the first free lane; else the
//                        lowest-ranked lane is replaced if the newcomer ranks above it, and the row is marked truncated --
//                        every pair in play is within the cut by now, so a pair leaves for room only when the header's rule
//                        says so;
//                        one coalesced write of the row (8 * width bytes) and lane 0's of the head.
//                      Rank: score descending, ties to the smaller genome id -- the key (score biased << 32 | INT32_MAX - id).
//                      Two merges never run at the same time (Accum::serial), so a row is read and written without atomics.
//   mnc_carry_sort_k   one wave per read, for mnc_carry_fetch: a pair's place is the number of the row's pairs with a smaller
//                      genome id (width shuffles); unused places are written -1 / 0.
//   mnc_carry_stat_k   rows used, pairs, truncated rows and the largest genome id: a wave per read, grid-stride, summed per
//                      wave and added once per wave with 64-bit atomics.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <new>
#include <vector>
#include "ab_common.h"

using namespace mnc;

constexpr int64_t CARRY_MAX_READS = 1LL << 32;   // one wave per read, four to a workgroup: the grid stays below 2^31
constexpr int CARRY_STAT_WG = 2048;
enum { SRC_BATCH = 0, SRC_CSR = 1, SRC_CARRY = 2 };

namespace mnc {

// ---------------------------------------------------------------- the row in registers
struct CarryRow {
	int g, s;                                  // this lane's slot: genome (-1: free) and score
	int best, flags;                           // wave-uniform
	int width, max_delta;

	__device__ __forceinline__ void load(const int2 *head, const int2 *slots, int64_t r, int w, int md)
	{
		width = w, max_delta = md;
		const int2 h = head[r];
		best = h.x, flags = h.y;
		const int2 p = lane_id() < w ? slots[r * w + lane_id()] : make_int2(-1, 0);
		g = (flags & CARRY_USED) ? p.x : -1, s = g >= 0 ? p.y : 0;
	}
	// best := max(best, nb), and every pair beyond the cut leaves
	__device__ __forceinline__ void raise(int nb)
	{
		best = (flags & CARRY_USED) && best > nb ? best : nb;
		flags |= CARRY_USED;
		if (g >= 0 && (long long)best - s > max_delta) g = -1, s = 0;
	}
	__device__ __forceinline__ bool within(int S) const { return (long long)best - S <= max_delta; }
	static __device__ __forceinline__ unsigned long long rank_key(int G, int S)
	{
		return (unsigned long long)((uint32_t)S ^ 0x80000000u) << 32 | (uint32_t)(INT32_MAX - G);
	}
	// one incoming pair, the same in every lane, within the cut
	__device__ __forceinline__ void offer(int G, int S)
	{
		const int lane = lane_id();
		if (__ballot(g == G)) {
			if (g == G && S > s) s = S;
			return;
		}
		const unsigned long long free_lanes = __ballot(lane < width && g < 0);
		if (free_lanes) {
			if (lane == __ffsll((long long)free_lanes) - 1) g = G, s = S;
			return;
		}
		const unsigned long long mine = lane < width ? rank_key(g, s) : ~0ull;
		const unsigned long long low = ab_wave_min(mine);
		if (rank_key(G, S) > low && mine == low) g = G, s = S;
		flags |= CARRY_TRUNCATED;
	}
	__device__ __forceinline__ void store(int2 *head, int2 *slots, int64_t r) const
	{
		if (lane_id() < width) slots[r * width + lane_id()] = make_int2(g, s);
		if (lane_id() == 0) head[r] = make_int2(best, flags);
	}
};

// what a merge takes its pairs from (one of the three is set)
struct CarrySrc {
	int n_contigs, n_genomes, genome_offset;   // SRC_BATCH
	const int64_t *offsets;                    // SRC_CSR: row r = (genome, score)[offsets[r] .. offsets[r + 1])
	const int32_t *genome, *score;
	const int2 *head, *slots;                  // SRC_CARRY: same width and max_delta
};

template <int SRC>
__global__ __launch_bounds__(256) void mnc_carry_merge_k(Batch B, CarrySrc src, int64_t n, int64_t first_read, int width, int max_delta, int2 *head, int2 *slots)
{
	const int lane = lane_id();
	const int64_t rd = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (rd >= n) return;                                      // (whole waves; the kernel has no workgroup barrier)
	const int64_t r = first_read + rd;                        // (the host has checked first_read + n <= the rows there are)
	CarryRow row;
	if (SRC == SRC_BATCH) {
		const int nr = B.n_reg[rd];
		if (nr <= 0) return;
		const int64_t slot0 = reg_slot(B, (uint32_t)rd);
		int nb;
		if (!ab_best(B, slot0, nr, src.n_contigs, src.n_genomes, nb)) return;   // a read with no record leaves its row as it is
		row.load(head, slots, r, width, max_delta);
		row.raise(nb);
		for (int last = -1;;) {
			const unsigned long long key = ab_next(B, slot0, nr, src.n_contigs, src.n_genomes, last);
			if (key == ~0ull) break;
			last = (int)(key >> 32);
			const int S = ab_key_score(key);
			if (row.within(S)) row.offer(last + src.genome_offset, S);
		}
	} else if (SRC == SRC_CSR) {
		const int64_t a = src.offsets[rd], b = src.offsets[rd + 1];   // (b > a: checked on the host)
		int nb = INT32_MIN;
		for (int64_t j = a + lane; j < b; j += 64) nb = src.score[j] > nb ? src.score[j] : nb;
		for (int d = 32; d > 0; d >>= 1) {
			const int o = __shfl_xor(nb, d);
			nb = o > nb ? o : nb;
		}
		row.load(head, slots, r, width, max_delta);
		row.raise(nb);
		for (int64_t j = a; j < b; ++j) {
			const int G = src.genome[j], S = src.score[j];
			if (row.within(S)) row.offer(G, S);
		}
	} else {
		const int2 h = src.head[r];
		if (!(h.y & CARRY_USED)) return;
		const int2 p = lane < width ? src.slots[r * width + lane] : make_int2(-1, 0);
		row.load(head, slots, r, width, max_delta);
		row.raise(h.x);
		row.flags |= h.y & CARRY_TRUNCATED;
		for (int i = 0; i < width; ++i) {
			const int G = __shfl(p.x, i), S = __shfl(p.y, i);
			if (G >= 0 && row.within(S)) row.offer(G, S);
		}
	}
	row.store(head, slots, r);
}

// rows [r0, r1): empty
__global__ __launch_bounds__(256) void mnc_carry_clear_k(int2 *head, int2 *slots, int64_t r0, int64_t r1, int width)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	for (int64_t i = r0 + i0; i < r1; i += stride) head[i] = make_int2(0, 0);
	for (int64_t i = r0 * width + i0; i < r1 * width; i += stride) slots[i] = make_int2(-1, 0);
}

__global__ __launch_bounds__(256) void mnc_carry_sort_k(const int2 *head, const int2 *slots, int64_t first_read, int64_t n, int width, int32_t *count, int32_t *best,
                                                        int32_t *genome, int32_t *score)
{
	const int lane = lane_id();
	const int64_t rd = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (rd >= n) return;
	const int2 h = head[first_read + rd];
	const bool used = (h.y & CARRY_USED) != 0;
	const int2 p = used && lane < width ? slots[(first_read + rd) * width + lane] : make_int2(-1, 0);
	const int k = __popcll(__ballot(p.x >= 0));
	int rank = 0;
	for (int i = 0; i < width; ++i) {
		const int gi = __shfl(p.x, i);
		rank += gi >= 0 && gi < p.x;
	}
	if (lane < width && lane >= k) genome[rd * width + lane] = -1, score[rd * width + lane] = 0;
	if (p.x >= 0) genome[rd * width + rank] = p.x, score[rd * width + rank] = p.y;
	if (lane == 0) count[rd] = k, best[rd] = used ? h.x : 0;
}

__global__ __launch_bounds__(256) void mnc_carry_stat_k(const int2 *head, const int2 *slots, int64_t n, int width, unsigned long long *stat)
{
	const int lane = lane_id();
	unsigned long long rows = 0, pairs = 0, trunc = 0;
	int top = -1;
	for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * (blockDim.x >> 6)) {
		const int2 h = head[r];
		if (!(h.y & CARRY_USED)) continue;
		const int2 p = lane < width ? slots[r * width + lane] : make_int2(-1, 0);
		rows += 1, trunc += (h.y & CARRY_TRUNCATED) != 0;
		pairs += (unsigned long long)__popcll(__ballot(p.x >= 0));
		top = p.x > top ? p.x : top;
	}
	for (int d = 32; d > 0; d >>= 1) {
		const int o = __shfl_xor(top, d);
		top = o > top ? o : top;
	}
	if (lane != 0 || rows == 0) return;
	(void)__hip_atomic_fetch_add(stat + 0, rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	(void)__hip_atomic_fetch_add(stat + 1, pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	(void)__hip_atomic_fetch_add(stat + 2, trunc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	(void)__hip_atomic_fetch_max(stat + 3, (unsigned long long)(top + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- host side
static unsigned merge_grid(int64_t n) { return (unsigned)((n + 3) / 4); }
static unsigned clear_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (items + 255) / 256)); }

const Accum *as_accum(const mnc_carry *cc) { return cc; }

// The batch B of an engine, as it stands in HBM, on the engine's stream `st`; nothing waits on the host.  The range check
// is made under the carry's lock, against the rows there are at that moment.
int carry_add(mnc_carry *cc, const Batch &B, int n_contigs, int n_genomes, int64_t first_read, int32_t genome_offset, hipStream_t st)
{
	int rc = MNC_OK;
	const int q = cc->add(st, [&] {
		if ((int64_t)B.n_reads > cc->cap || first_read > cc->cap - (int64_t)B.n_reads) {
			set_error("reads [%lld, %lld) do not fit a carry of %lld rows: mnc_carry_reserve first", (long long)first_read, (long long)(first_read + B.n_reads), (long long)cc->cap);
			rc = MNC_ERR_RANGE;
			return;
		}
		CarrySrc src = {};
		src.n_contigs = n_contigs, src.n_genomes = n_genomes, src.genome_offset = genome_offset;
		hipLaunchKernelGGL(mnc_carry_merge_k<SRC_BATCH>, dim3(merge_grid(B.n_reads)), dim3(256), 0, st, B, src, (int64_t)B.n_reads, first_read, (int)cc->width,
		                   (int)cc->max_delta, cc->head, cc->slots);
	});
	return rc ? rc : q;
}

int carry_read_begin(mnc_carry *cc, hipStream_t on)
{
	std::lock_guard<std::mutex> lk(cc->mu);
	HIP_TRY(hipStreamWaitEvent(on, cc->ev_add, 0));
	HIP_TRY(hipStreamWaitEvent(on, cc->ev_own, 0));
	return MNC_OK;
}

int carry_read_end(mnc_carry *cc, hipEvent_t done)
{
	std::lock_guard<std::mutex> lk(cc->mu);
	HIP_TRY(hipStreamWaitEvent(cc->st, done, 0));
	HIP_TRY(cc->own_done());
	return MNC_OK;
}

int carry_stats(mnc_carry *cc, unsigned long long *s)
{
	HIP_TRY(hipSetDevice(cc->device));
	std::lock_guard<std::mutex> lk(cc->mu);
	HIP_TRY(hipMemsetAsync(cc->stat, 0, 32, cc->st));
	if (cc->cap) {
		const unsigned wg = (unsigned)std::max<int64_t>(1, std::min<int64_t>(CARRY_STAT_WG, (cc->cap + 3) / 4));
		hipLaunchKernelGGL(mnc_carry_stat_k, dim3(wg), dim3(256), 0, cc->st, cc->head, cc->slots, cc->cap, (int)cc->width, cc->stat);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipMemcpyAsync(s, cc->stat, 32, hipMemcpyDeviceToHost, cc->st));
	HIP_TRY(hipStreamSynchronize(cc->st));
	return MNC_OK;
}

} // namespace mnc

// rows [r0, r1) empty, on the carry's stream (the caller holds `mu`)
static hipError_t carry_clear(mnc_carry *cc, int64_t r0, int64_t r1)
{
	if (r1 <= r0) return hipSuccess;
	hipLaunchKernelGGL(mnc_carry_clear_k, dim3(clear_grid((r1 - r0) * cc->width)), dim3(256), 0, cc->st, cc->head, cc->slots, r0, r1, (int)cc->width);
	return hipGetLastError();
}

// ---------------------------------------------------------------- C-ABI
extern "C" void mnc_carry_free(mnc_carry *cc)
{
	if (!cc) return;
	cc->release();
	delete cc;
}

extern "C" int mnc_carry_create(int device, int64_t cap_reads, int32_t width, int32_t max_delta, mnc_carry **out)
{
	if (!out) return MNC_ERR_ARG;
	*out = nullptr;
	if (cap_reads < 0 || cap_reads > CARRY_MAX_READS) { set_error("cap_reads %lld outside 0 .. 2^32", (long long)cap_reads); return MNC_ERR_ARG; }
	if (width < 1 || width > CARRY_MAX_WIDTH) { set_error("width %d outside 1 .. %d (a row lives in one wave, one pair per lane)", width, CARRY_MAX_WIDTH); return MNC_ERR_ARG; }
	if (max_delta < 0) { set_error("max_delta %d: max_delta >= 0 is required", max_delta); return MNC_ERR_ARG; }
	if (int rc = check_device(device)) return rc;
	mnc_carry *cc = new (std::nothrow) mnc_carry;
	if (!cc) return MNC_ERR_NOMEM;
	cc->cap = cap_reads, cc->width = width, cc->max_delta = max_delta, cc->serial = true;
	hipError_t he = cc->begin(nullptr, device);
	cc->alloc(he, (void**)&cc->head, (size_t)cap_reads * 8);
	cc->alloc(he, (void**)&cc->slots, (size_t)cap_reads * width * 8);
	cc->alloc(he, (void**)&cc->stat, 32);
	cc->streams(he);
	if (he != hipSuccess) {
		set_error("candidate carry of %lld reads (%d bytes each): %s", (long long)cap_reads, 8 * width + 8, hipGetErrorString(he));
		const int rc = Accum::failed(he);
		mnc_carry_free(cc);
		return rc;
	}
	if (int rc = mnc_carry_reset(cc)) { mnc_carry_free(cc); return rc; }
	*out = cc;
	return MNC_OK;
}

extern "C" int mnc_carry_reset(mnc_carry *cc)
{
	if (!cc) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(cc->device));
	std::lock_guard<std::mutex> lk(cc->mu);
	HIP_TRY(carry_clear(cc, 0, cc->cap));
	HIP_TRY(cc->own_done());
	return MNC_OK;
}

extern "C" int mnc_carry_reserve(mnc_carry *cc, int64_t n_reads)
{
	if (!cc) return MNC_ERR_ARG;
	if (n_reads < 0 || n_reads > CARRY_MAX_READS) { set_error("n_reads %lld outside 0 .. 2^32", (long long)n_reads); return MNC_ERR_ARG; }
	HIP_TRY(hipSetDevice(cc->device));
	std::lock_guard<std::mutex> lk(cc->mu);                     // (an engine's carry reads the pointers under it)
	if (n_reads <= cc->cap) return MNC_OK;
	const int64_t cap = std::min<int64_t>(CARRY_MAX_READS, std::max<int64_t>(n_reads, cc->cap + cc->cap / 2));
	int2 *head = nullptr, *slots = nullptr;
	hipError_t he = hipMalloc((void**)&head, (size_t)cap * 8);
	if (he == hipSuccess) he = hipMalloc((void**)&slots, (size_t)cap * cc->width * 8);
	// what is there is copied behind every merge queued so far (`st` waits for each add's event), then the old rows go
	if (he == hipSuccess && cc->cap) he = hipMemcpyAsync(head, cc->head, (size_t)cc->cap * 8, hipMemcpyDeviceToDevice, cc->st);
	if (he == hipSuccess && cc->cap) he = hipMemcpyAsync(slots, cc->slots, (size_t)cc->cap * cc->width * 8, hipMemcpyDeviceToDevice, cc->st);
	if (he == hipSuccess) he = hipStreamSynchronize(cc->st);
	if (he != hipSuccess) {
		set_error("candidate carry of %lld reads (%d bytes each): %s", (long long)cap, 8 * cc->width + 8, hipGetErrorString(he));
		(void)hipFree(head), (void)hipFree(slots);
		return Accum::failed(he);
	}
	for (void *&p : cc->bufs) p = p == (void*)cc->head ? (void*)head : p == (void*)cc->slots ? (void*)slots : p;
	(void)hipFree(cc->head), (void)hipFree(cc->slots);
	cc->bytes += (cap - cc->cap) * (8 * (int64_t)cc->width + 8) - (cc->cap ? 0 : 16);   // (an empty buffer was 8 bytes)
	const int64_t old = cc->cap;
	cc->head = head, cc->slots = slots, cc->cap = cap;
	HIP_TRY(carry_clear(cc, old, cap));
	HIP_TRY(cc->own_done());
	return MNC_OK;
}

extern "C" int mnc_carry_device_bytes(const mnc_carry *cc, int64_t *bytes) { return accum_device_bytes(cc, bytes); }

extern "C" int mnc_carry_add_lists(mnc_carry *cc, int64_t first_read, int64_t n_reads, const int64_t *offsets, const int32_t *genome, const int32_t *score)
{
	if (!cc || n_reads < 0 || (n_reads && !offsets)) return MNC_ERR_ARG;
	if (first_read < 0) { set_error("first_read %lld: a read's ordinal", (long long)first_read); return MNC_ERR_ARG; }
	// ---- every check on the host, before anything is touched
	if (n_reads && (offsets[0] < 0 || !genome || !score)) return MNC_ERR_ARG;
	for (int64_t r = 0; r < n_reads; ++r) {
		const int64_t a = offsets[r], b = offsets[r + 1];
		if (b <= a) { set_error("row %lld is empty (offsets %lld, %lld)", (long long)r, (long long)a, (long long)b); return MNC_ERR_ARG; }
		for (int64_t j = a; j < b; ++j)
			if (genome[j] < 0 || (j > a && genome[j] <= genome[j - 1])) {
				set_error("row %lld: genome ids must be >= 0 and ascend strictly", (long long)r);
				return MNC_ERR_ARG;
			}
	}
	HIP_TRY(hipSetDevice(cc->device));
	std::lock_guard<std::mutex> lk(cc->mu);
	if (n_reads > cc->cap || first_read > cc->cap - n_reads) {
		set_error("reads [%lld, %lld) do not fit a carry of %lld rows: mnc_carry_reserve first", (long long)first_read, (long long)(first_read + n_reads), (long long)cc->cap);
		return MNC_ERR_RANGE;
	}
	if (n_reads == 0) return MNC_OK;
	const int64_t a0 = offsets[0], n_pairs = offsets[n_reads] - a0;
	std::vector<int64_t> off;
	try {
		off.resize((size_t)n_reads + 1);
	} catch (const std::bad_alloc &) { return MNC_ERR_NOMEM; }
	for (int64_t r = 0; r <= n_reads; ++r) off[(size_t)r] = offsets[r] - a0;
	char *tmp = nullptr;                                       // offsets, genome, score behind one another
	const size_t b_off = ((size_t)n_reads + 1) * 8, b_col = (size_t)n_pairs * 4;
	HIP_TRY(hipMalloc((void**)&tmp, b_off + 2 * b_col));
	hipError_t he = hipMemcpyAsync(tmp, off.data(), b_off, hipMemcpyHostToDevice, cc->st);
	if (he == hipSuccess) he = hipMemcpyAsync(tmp + b_off, genome + a0, b_col, hipMemcpyHostToDevice, cc->st);
	if (he == hipSuccess) he = hipMemcpyAsync(tmp + b_off + b_col, score + a0, b_col, hipMemcpyHostToDevice, cc->st);
	if (he == hipSuccess) {
		CarrySrc src = {};
		src.offsets = (const int64_t*)tmp, src.genome = (const int32_t*)(tmp + b_off), src.score = (const int32_t*)(tmp + b_off + b_col);
		hipLaunchKernelGGL(mnc_carry_merge_k<SRC_CSR>, dim3(merge_grid(n_reads)), dim3(256), 0, cc->st, Batch{}, src, n_reads, first_read, (int)cc->width,
		                   (int)cc->max_delta, cc->head, cc->slots);
		he = hipGetLastError();
	}
	if (he == hipSuccess) he = cc->own_done();                   // an engine's carry comes behind it
	const hipError_t hs = hipStreamSynchronize(cc->st);          // the host arrays above are read until here
	if (he == hipSuccess) he = hs;
	(void)hipFree(tmp);
	if (he != hipSuccess) { set_error("carry add_lists: %s", hipGetErrorString(he)); return MNC_ERR_HIP; }
	return MNC_OK;
}

extern "C" int mnc_carry_merge(mnc_carry *dst, mnc_carry *src)
{
	if (!dst || !src || dst == src) return MNC_ERR_ARG;
	if (dst->device != src->device || dst->width != src->width || dst->max_delta != src->max_delta) {
		set_error("two carries are merged on one device, with one width and one max_delta");
		return MNC_ERR_ARG;
	}
	HIP_TRY(hipSetDevice(dst->device));
	{
		std::lock_guard<std::mutex> lk(dst->mu);
		if (src->cap > dst->cap) { set_error("a carry of %lld rows into one of %lld: mnc_carry_reserve first", (long long)src->cap, (long long)dst->cap); return MNC_ERR_RANGE; }
		if (src->cap == 0) return MNC_OK;
		if (int rc = carry_read_begin(src, dst->st)) return rc;
		CarrySrc from = {};
		from.head = src->head, from.slots = src->slots;
		hipLaunchKernelGGL(mnc_carry_merge_k<SRC_CARRY>, dim3(merge_grid(src->cap)), dim3(256), 0, dst->st, Batch{}, from, src->cap, (int64_t)0, (int)dst->width,
		                   (int)dst->max_delta, dst->head, dst->slots);
		HIP_TRY(hipGetLastError());
		HIP_TRY(dst->own_done());                                // an engine's carry into dst comes behind it
	}
	return carry_read_end(src, dst->ev_own);
}

extern "C" int mnc_carry_info(mnc_carry *cc, int64_t *cap_reads, int64_t *n_rows_used, int64_t *n_cands, int64_t *n_truncated_reads)
{
	if (!cc) return MNC_ERR_ARG;
	unsigned long long s[4];
	if (int rc = carry_stats(cc, s)) return rc;
	if (cap_reads) *cap_reads = cc->cap;
	if (n_rows_used) *n_rows_used = (int64_t)s[0];
	if (n_cands) *n_cands = (int64_t)s[1];
	if (n_truncated_reads) *n_truncated_reads = (int64_t)s[2];
	return MNC_OK;
}

extern "C" int mnc_carry_fetch(mnc_carry *cc, int64_t first_read, int64_t n_reads, int32_t *count, int32_t *best, int32_t *genome, int32_t *score)
{
	if (!cc || n_reads < 0) return MNC_ERR_ARG;
	if (first_read < 0) { set_error("first_read %lld: a read's ordinal", (long long)first_read); return MNC_ERR_ARG; }
	HIP_TRY(hipSetDevice(cc->device));
	std::lock_guard<std::mutex> lk(cc->mu);
	if (n_reads > cc->cap || first_read > cc->cap - n_reads) {
		set_error("reads [%lld, %lld) of a carry of %lld rows", (long long)first_read, (long long)(first_read + n_reads), (long long)cc->cap);
		return MNC_ERR_RANGE;
	}
	if (n_reads == 0) return MNC_OK;
	const size_t b_row = (size_t)n_reads * 4, b_col = b_row * (size_t)cc->width;
	char *tmp = nullptr;                                       // count, best, genome, score behind one another
	HIP_TRY(hipMalloc((void**)&tmp, 2 * b_row + 2 * b_col));
	int32_t *d_count = (int32_t*)tmp, *d_best = (int32_t*)(tmp + b_row), *d_genome = (int32_t*)(tmp + 2 * b_row), *d_score = (int32_t*)(tmp + 2 * b_row + b_col);
	hipLaunchKernelGGL(mnc_carry_sort_k, dim3(merge_grid(n_reads)), dim3(256), 0, cc->st, cc->head, cc->slots, first_read, n_reads, (int)cc->width, d_count, d_best,
	                   d_genome, d_score);
	hipError_t he = hipGetLastError();
	if (he == hipSuccess && count) he = hipMemcpyAsync(count, d_count, b_row, hipMemcpyDeviceToHost, cc->st);
	if (he == hipSuccess && best) he = hipMemcpyAsync(best, d_best, b_row, hipMemcpyDeviceToHost, cc->st);
	return cc->finish(he, tmp, { genome, d_genome, b_col }, { score, d_score, b_col }, "carry fetch of %lld rows", (long long)n_reads);
}

extern "C" int mnc_carry_device(mnc_carry *cc, const int32_t **d_head, const int32_t **d_slots, int64_t *cap_reads, int32_t *width)
{
	if (!cc) return MNC_ERR_ARG;
	std::lock_guard<std::mutex> lk(cc->mu);
	if (d_head) *d_head = cc->cap ? (const int32_t*)cc->head : nullptr;
	if (d_slots) *d_slots = cc->cap ? (const int32_t*)cc->slots : nullptr;
	if (cap_reads) *cap_reads = cc->cap;
	if (width) *width = cc->width;
	return MNC_OK;
}
