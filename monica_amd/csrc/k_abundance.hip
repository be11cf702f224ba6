// Abundance by expectation-maximisation over every candidate genome (include/monica_amd.h, "abundance"): the fourth consumer
// of a batch as it stands in HBM, after k_export.hip, k_coverage.hip and k_pileup.hip.  An accumulator that lives across
// classify calls collects, per read, the genomes whose best base-level score lies within max_delta of the read's best; a
// read with one such genome is counted at once, a read with several is kept as one row of a CSR of (genome, delta) pairs.
// mnc_abundance_solve then runs the EM over the rows.  Runs only when asked for; nothing here is on the classification path.
//
//   mnc_ab_collect   one wave per READ, the records found as mnc_pile_add finds them and selected as MNC_COV_ALL selects
//                    (cov_common.h), a CIGAR required.  The candidates come out in ascending genome id by extraction: each
//                    round takes the wave minimum of the key (genome << 32 | inverted score) over the records whose genome
//                    lies above the last one taken -- the smallest such genome and, within it, its largest dp_max.  A read
//                    has a few tens of records at most, so a round is one or two loads per lane.  The rounds run twice: once
//                    to count the candidates, once -- behind the reservation -- to write them, so that no bound on the number
//                    of genomes of a read is built in.
//                    The reservation: rows and candidate slots are handed out TOGETHER from one 64-bit word (rows << 33 |
//                    slots) by a compare-and-swap loop of lane 0, so row r starts where row r - 1 ends -- offsets is a true
//                    CSR whatever order the waves arrive in -- and a row that does not fit takes nothing: it is counted in
//                    n_dropped and the word stays as it was.  No host wait.
//   mnc_ab_collect_carry  the same treatment for the rows of a candidate carry (k_carry.hip; mnc_abundance_add_carry, for a
//                    database of several index parts): one wave per row, a pair per lane, ascending genome id by rank, the
//                    same reservation.
//   mnc_ab_pass      one EM iteration's E and M step in one pass over the CSR, one thread per ROW (rows hold 2-6 pairs: 8
//                    bytes per candidate, 8 per row offset, and the theta gathers).  Every product, sum and quotient is one
//                    IEEE double operation rounded to nearest (__dmul_rn / __dadd_rn / __ddiv_rn; no fused multiply-add);
//                    what a row gives a genome is floor(p * 2^32) as uint64, and the sums are integer sums: the result does
//                    not depend on row order, launch shape or batch cut, and no floating-point atomic appears anywhere.
//                    While G <= AB_LDS_G = 2 048 genomes, theta (8 bytes) and a private uint64 acc (8 bytes) per genome sit
//                    in LDS -- 32 KiB a workgroup -- and a workgroup flushes its non-zero entries with 64-bit global atomics
//                    at the end; above the cut-off theta is gathered from HBM / L2 and every add is a 64-bit global atomic.
//   mnc_ab_finish    the small pass behind it, one workgroup: total, the new theta, the integer convergence test, the next
//                    iteration's acc set to unique << 32 (the two acc buffers swap by the iteration's parity).
//   Host round trips: the form built is the device-side "done" word.  mnc_abundance_solve queues init and then pass + finish
//                    per iteration without reading anything back; once the test is met (or rows were dropped, or nothing was
//                    added) the word is set and the remaining launches return at once.  One wait at the end.  Only a
//                    max_iter above AB_LAUNCH_BLOCK = 256 iterations is queued in blocks of that many, the word read
//                    between blocks.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <new>
#include <vector>
#include "ab_common.h"                         // (the records that count and the extraction rounds: shared with k_carry.hip)

using namespace mnc;

constexpr int AB_LDS_G = 2048;                 // genomes whose theta and private acc fit a workgroup's LDS (16 bytes each)
constexpr int AB_LAUNCH_BLOCK = 256;           // iterations queued before the "done" word is looked at
constexpr int AB_PASS_WG = 2048;               // workgroups of a pass at most (grid-stride over the rows)
constexpr int AB_SLOT_BITS = 33;               // the reservation word: rows << 33 | candidate slots
constexpr int64_t AB_MAX_CANDS = 1LL << 32;    // so cap_cands (and with it twice the rows) stays below either field's range
constexpr unsigned long long AB_SLOT_MASK = (1ull << AB_SLOT_BITS) - 1ull;
// counters (uint64 words of `ctr`)
constexpr int ABC_PACK = 0, ABC_READS = 1, ABC_DROPPED = 2, ABC_N = 4;
// solver state (uint64 words of `state`)
constexpr int ABS_DONE = 0, ABS_ITERS = 1, ABS_LAST = 2, ABS_N = 4;

struct mnc_abundance : Accum {                 // (ev_own: the last reset or add_lists)
	int n_contigs = 0, G = 0;
	int64_t cap_cands = 0, cap_rows = 0;
	int32_t max_delta = 0, scale_q = 0;
	int64_t *unique = nullptr;                 // [G]
	int64_t *offsets = nullptr;                // [cap_rows + 1]
	int32_t *genome = nullptr, *delta = nullptr;   // [cap_cands] each
	unsigned long long *ctr = nullptr;         // [ABC_N]
	double *theta = nullptr;                   // [G]
	unsigned long long *acc = nullptr;         // [2][G]
	unsigned long long *state = nullptr;       // [ABS_N]
};

namespace mnc {

// ---------------------------------------------------------------- collect
// (ab_best, ab_next and the key they share: ab_common.h)

// Lane 0 of a wave reserves one row and its k candidate slots together, or drops the row: the word as it stood before the
// reservation (rows << 33 | slots: the row's number and its first slot), ~0 for a row that does not fit.  Counted in
// n_reads or in n_dropped either way.
__device__ __forceinline__ unsigned long long ab_reserve(unsigned long long *ctr, int k, int64_t cap_cands, int64_t cap_rows)
{
	unsigned long long got = ~0ull;
	unsigned long long cur = __hip_atomic_load(ctr + ABC_PACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	for (;;) {
		const int64_t rows = (int64_t)(cur >> AB_SLOT_BITS), slots = (int64_t)(cur & AB_SLOT_MASK);
		if (slots + k > cap_cands || rows + 1 > cap_rows) break;
		const unsigned long long want = cur + (1ull << AB_SLOT_BITS) + (unsigned long long)k;
		if (__hip_atomic_compare_exchange_strong(ctr + ABC_PACK, &cur, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { got = cur; break; }
	}
	(void)__hip_atomic_fetch_add(ctr + (got == ~0ull ? ABC_DROPPED : ABC_READS), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	return got;
}

__global__ __launch_bounds__(256) void mnc_ab_collect(Batch B, int n_contigs, int n_genomes, int max_delta, int64_t cap_cands, int64_t cap_rows,
                                                      int64_t *unique, int64_t *offsets, int32_t *genome, int32_t *delta, unsigned long long *ctr)
{
	const int lane = lane_id();
	const uint32_t rd = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (rd >= B.n_reads) return;                              // (whole waves; the kernel has no workgroup barrier)
	const int n = B.n_reg[rd];
	if (n <= 0) return;
	const int64_t slot0 = reg_slot(B, rd);
	// ---- best: the largest dp_max of the records that count
	int best;
	if (!ab_best(B, slot0, n, n_contigs, n_genomes, best)) return;   // a read with no record adds nothing
	// ---- count the candidates
	int k = 0, only = -1;
	for (int last = -1;;) {
		const unsigned long long key = ab_next(B, slot0, n, n_contigs, n_genomes, last);
		if (key == ~0ull) break;
		last = (int)(key >> 32);
		if ((long long)best - ab_key_score(key) <= max_delta) ++k, only = last;
	}
	if (k == 1) {
		if (lane == 0) {
			(void)__hip_atomic_fetch_add(unique + only, (int64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			(void)__hip_atomic_fetch_add(ctr + ABC_READS, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		return;
	}
	// ---- reserve row and slots together, or drop the row
	unsigned long long got = ~0ull;
	if (lane == 0) got = ab_reserve(ctr, k, cap_cands, cap_rows);
	got = __shfl(got, 0);
	if (got == ~0ull) return;
	const int64_t row = (int64_t)(got >> AB_SLOT_BITS), start = (int64_t)(got & AB_SLOT_MASK);
	// ---- write them: the same rounds again (start + k <= cap_cands and row < cap_rows were checked by the reservation)
	int j = 0;
	for (int last = -1; j < k;) {
		const unsigned long long key = ab_next(B, slot0, n, n_contigs, n_genomes, last);
		if (key == ~0ull) break;
		last = (int)(key >> 32);
		const long long dl = (long long)best - ab_key_score(key);
		if (dl > max_delta) continue;
		if (lane == 0) genome[start + j] = last, delta[start + j] = (int32_t)dl;
		++j;
	}
	if (lane == 0) offsets[row] = start, offsets[row + 1] = start + k;   // (row r + 1 writes the same value into its own first word)
}

// A carry's rows [first, first + n) (k_carry.hip), each treated as mnc_ab_collect treats a read: one wave per row, the
// row's pairs one per lane.  Ascending genome id by rank: a pair's place is the number of the row's pairs with a smaller id.
// The host has checked that the carry holds no id >= n_genomes.
__global__ __launch_bounds__(256) void mnc_ab_collect_carry(const int2 *head, const int2 *slots, int width, int64_t first, int64_t n, int n_genomes,
                                                            int64_t cap_cands, int64_t cap_rows, int64_t *unique, int64_t *offsets, int32_t *genome,
                                                            int32_t *delta, unsigned long long *ctr)
{
	const int lane = lane_id();
	const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (r >= n) return;                                       // (whole waves; no workgroup barrier)
	const int2 h = head[first + r];
	if (!(h.y & CARRY_USED)) return;
	const int2 p = lane < width ? slots[(first + r) * width + lane] : make_int2(-1, 0);
	const bool valid = p.x >= 0 && p.x < n_genomes;
	const int k = __popcll(__ballot(valid));
	if (k == 0) return;
	if (k == 1) {
		if (valid) {
			(void)__hip_atomic_fetch_add(unique + p.x, (int64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			(void)__hip_atomic_fetch_add(ctr + ABC_READS, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		return;
	}
	int rank = 0;
	for (int i = 0; i < width; ++i) {
		const int gi = __shfl(p.x, i);
		rank += gi >= 0 && gi < p.x;
	}
	unsigned long long got = ~0ull;
	if (lane == 0) got = ab_reserve(ctr, k, cap_cands, cap_rows);
	got = __shfl(got, 0);
	if (got == ~0ull) return;
	const int64_t row = (int64_t)(got >> AB_SLOT_BITS), start = (int64_t)(got & AB_SLOT_MASK);
	if (valid) genome[start + rank] = p.x, delta[start + rank] = (int32_t)((long long)h.x - p.y);   // (rank < k: start + k <= cap_cands)
	if (lane == 0) offsets[row] = start, offsets[row + 1] = start + k;
}

// ---------------------------------------------------------------- solve
// 2^(-f/4), f = 0 .. 3, as the header's exact doubles
__constant__ unsigned long long AB_T[4] = { 0x3ff0000000000000ull, 0x3feae89f995ad3adull, 0x3fe6a09e667f3bcdull, 0x3fe306fe0a31b715ull };

// ldexp(T[x & 3], -(x >> 2)): x <= 4000, so the result is a normal double and the exponent field can be lowered in place
__device__ __forceinline__ double ab_weight(int dl, int scale_q)
{
	const int x = dl * scale_q;
	return __longlong_as_double((long long)(AB_T[x & 3] - ((unsigned long long)(x >> 2) << 52)));
}

__global__ __launch_bounds__(1024) void mnc_ab_init(int G, const int64_t *unique, const unsigned long long *ctr, double *theta, unsigned long long *acc,
                                                    unsigned long long *state)
{
	const double t0 = G > 0 ? __ddiv_rn(1.0, (double)G) : 0.0;
	for (int g = threadIdx.x; g < G; g += blockDim.x) {
		theta[g] = t0;
		acc[g] = (unsigned long long)unique[g] << 32;           // iteration 1 adds into buffer 0 ...
		acc[(size_t)G + g] = 0;                                 // ... and is compared with zeros
	}
	if (threadIdx.x == 0) {
		state[ABS_DONE] = ctr[ABC_READS] == 0 || ctr[ABC_DROPPED] != 0;
		state[ABS_ITERS] = 0, state[ABS_LAST] = 1;
	}
}

template <bool LDS>
__global__ __launch_bounds__(256) void mnc_ab_pass(int G, int scale_q, const int64_t *offsets, const int32_t *genome, const int32_t *delta,
                                                   const unsigned long long *ctr, const double *theta, unsigned long long *acc, const unsigned long long *state)
{
	__shared__ double s_theta[LDS ? AB_LDS_G : 1];
	__shared__ unsigned long long s_acc[LDS ? AB_LDS_G : 1];
	if (state[ABS_DONE]) return;
	const int64_t n_rows = (int64_t)(ctr[ABC_PACK] >> AB_SLOT_BITS);
	if ((int64_t)blockIdx.x * blockDim.x >= n_rows) return;    // (uniform over the workgroup: before any barrier)
	if (LDS) {
		for (int g = threadIdx.x; g < G; g += blockDim.x) s_theta[g] = theta[g], s_acc[g] = 0;
		__syncthreads();
	}
	const double *th = LDS ? s_theta : theta;
	for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
		const int64_t a = offsets[r], b = offsets[r + 1];
		double z = 0.0;
		for (int64_t j = a; j < b; ++j) z = __dadd_rn(z, __dmul_rn(ab_weight(delta[j], scale_q), th[genome[j]]));
		if (!(z > 0.0)) continue;
		for (int64_t j = a; j < b; ++j) {                         // (the same products again: the row's lines are in L1 by now)
			const int g = genome[j];
			const double p = __ddiv_rn(__dmul_rn(ab_weight(delta[j], scale_q), th[g]), z);
			const unsigned long long v = (unsigned long long)__dmul_rn(p, 4294967296.0);   // floor: p >= 0
			if (!v) continue;
			if (LDS) (void)atomicAdd(&s_acc[g], v);
			else (void)__hip_atomic_fetch_add(acc + g, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
	if (LDS) {
		__syncthreads();
		for (int g = threadIdx.x; g < G; g += blockDim.x)
			if (s_acc[g]) (void)__hip_atomic_fetch_add(acc + g, s_acc[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// acc: this iteration's sums; prev: the last iteration's, which become the next iteration's buffer
__global__ __launch_bounds__(1024) void mnc_ab_finish(int G, unsigned long long tol, int which, const int64_t *unique, double *theta, unsigned long long *acc_all,
                                                      unsigned long long *state)
{
	__shared__ unsigned long long s_sum[16], s_max[16];
	if (state[ABS_DONE]) return;
	unsigned long long *acc = acc_all + (size_t)which * G, *prev = acc_all + (size_t)(which ^ 1) * G;
	unsigned long long sum = 0, mx = 0;
	for (int g = threadIdx.x; g < G; g += blockDim.x) {
		const unsigned long long x = acc[g], y = prev[g], d = x > y ? x - y : y - x;
		sum += x, mx = d > mx ? d : mx;
	}
	for (int d = 32; d > 0; d >>= 1) {
		sum += __shfl_xor(sum, d);
		const unsigned long long o = __shfl_xor(mx, d);
		mx = o > mx ? o : mx;
	}
	if (lane_id() == 0) s_sum[threadIdx.x >> 6] = sum, s_max[threadIdx.x >> 6] = mx;
	__syncthreads();
	sum = 0, mx = 0;
	for (int w = 0; w < (int)(blockDim.x >> 6); ++w) sum += s_sum[w], mx = s_max[w] > mx ? s_max[w] : mx;
	const double total = (double)sum;
	for (int g = threadIdx.x; g < G; g += blockDim.x) {
		theta[g] = sum ? __ddiv_rn((double)acc[g], total) : 0.0;
		prev[g] = (unsigned long long)unique[g] << 32;           // the next iteration adds into it
	}
	if (threadIdx.x == 0) {
		state[ABS_ITERS] += 1, state[ABS_LAST] = (unsigned long long)which;
		if (mx <= tol) state[ABS_DONE] = 1;
	}
}

// rows made by the caller (mnc_abundance_add_lists), already checked and laid behind the rows that are there
__global__ __launch_bounds__(256) void mnc_ab_append(int G, const int64_t *uniq_inc, int64_t *unique, unsigned long long *ctr, unsigned long long pack, unsigned long long n_reads)
{
	for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x)
		if (uniq_inc[g]) (void)__hip_atomic_fetch_add(unique + g, uniq_inc[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		ctr[ABC_PACK] = pack;
		(void)__hip_atomic_fetch_add(ctr + ABC_READS, n_reads, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// ---------------------------------------------------------------- the engine's side (mnc_engine_add_abundance, engine.hip)
const Accum *as_accum(const mnc_abundance *ab) { return ab; }

// the batch B, as it stands in HBM, on the engine's stream `st`; nothing waits on the host
int abundance_add(mnc_abundance *ab, const Batch &B, hipStream_t st)
{
	if (B.n_reads == 0 || ab->G == 0) return MNC_OK;
	return ab->add(st, [&] {
		hipLaunchKernelGGL(mnc_ab_collect, dim3((B.n_reads + 3) / 4), dim3(256), 0, st, B, ab->n_contigs, ab->G, (int)ab->max_delta, ab->cap_cands, ab->cap_rows,
		                   ab->unique, ab->offsets, ab->genome, ab->delta, ab->ctr);
	});
}

} // namespace mnc

// the counters as they stand behind everything queued so far
static int ab_counters(mnc_abundance *ab, unsigned long long *c)
{
	HIP_TRY(hipSetDevice(ab->device));
	HIP_TRY(hipMemcpyAsync(c, ab->ctr, ABC_N * 8, hipMemcpyDeviceToHost, ab->st));
	HIP_TRY(hipStreamSynchronize(ab->st));
	return MNC_OK;
}

// ---------------------------------------------------------------- C-ABI
extern "C" void mnc_abundance_free(mnc_abundance *ab)
{
	if (!ab) return;
	ab->release();
	delete ab;
}

// for the genomes of `idx`, or -- idx = NULL -- for n_genomes genomes of no index (mnc_abundance_create_global)
static int ab_create(mnc_index *idx, int32_t n_genomes, int device, int64_t cap_cands, int32_t max_delta, int32_t scale_q, mnc_abundance **out)
{
	*out = nullptr;
	if (cap_cands < 0 || cap_cands >= AB_MAX_CANDS) { set_error("cap_cands %lld outside 0 .. 2^32 - 1", (long long)cap_cands); return MNC_ERR_ARG; }
	if (max_delta < 0 || scale_q < 1 || (int64_t)max_delta * scale_q > 4000) {
		set_error("max_delta %d, scale_q %d: max_delta >= 0, scale_q >= 1 and max_delta * scale_q <= 4000 are required", max_delta, scale_q);
		return MNC_ERR_ARG;
	}
	if (int rc = check_device(device)) return rc;
	mnc_abundance *ab = new (std::nothrow) mnc_abundance;
	if (!ab) return MNC_ERR_NOMEM;
	ab->n_contigs = idx ? (int)idx->contig_len.size() : 0, ab->G = idx ? (int)idx->genome_name.size() : (int)n_genomes;
	ab->cap_cands = cap_cands, ab->cap_rows = cap_cands / 2, ab->max_delta = max_delta, ab->scale_q = scale_q;
	const size_t G = (size_t)ab->G;
	hipError_t he = ab->begin(idx, device);
	ab->alloc(he, (void**)&ab->unique, G * 8);
	ab->alloc(he, (void**)&ab->offsets, ((size_t)ab->cap_rows + 1) * 8);
	ab->alloc(he, (void**)&ab->genome, (size_t)cap_cands * 4);
	ab->alloc(he, (void**)&ab->delta, (size_t)cap_cands * 4);
	ab->alloc(he, (void**)&ab->ctr, ABC_N * 8);
	ab->alloc(he, (void**)&ab->theta, G * 8);
	ab->alloc(he, (void**)&ab->acc, G * 16);
	ab->alloc(he, (void**)&ab->state, ABS_N * 8);
	ab->streams(he);
	if (he != hipSuccess) {
		set_error("abundance accumulator of %lld candidate slots (12 bytes each): %s", (long long)cap_cands, hipGetErrorString(he));
		const int rc = Accum::failed(he);
		mnc_abundance_free(ab);
		return rc;
	}
	if (int rc = mnc_abundance_reset(ab)) { mnc_abundance_free(ab); return rc; }
	*out = ab;
	return MNC_OK;
}

extern "C" int mnc_abundance_create(mnc_index *idx, int device, int64_t cap_cands, int32_t max_delta, int32_t scale_q, mnc_abundance **out)
{
	if (!idx || !out) return MNC_ERR_ARG;
	return ab_create(idx, 0, device, cap_cands, max_delta, scale_q, out);
}

extern "C" int mnc_abundance_create_global(int device, int32_t n_genomes, int64_t cap_cands, int32_t max_delta, int32_t scale_q, mnc_abundance **out)
{
	if (!out) return MNC_ERR_ARG;
	*out = nullptr;
	if (n_genomes < 0) { set_error("n_genomes %d: a number of genomes", n_genomes); return MNC_ERR_ARG; }
	return ab_create(nullptr, n_genomes, device, cap_cands, max_delta, scale_q, out);
}

// The rows [first_read, first_read + n_reads) of a carry, each as one read.  The one wait is for the carry's largest genome
// id (every check comes before anything is added); the add itself is queued on the accumulator's stream.
extern "C" int mnc_abundance_add_carry(mnc_abundance *ab, mnc_carry *cc, int64_t first_read, int64_t n_reads)
{
	if (!ab || !cc) return MNC_ERR_ARG;
	if (first_read < 0 || n_reads < 0) { set_error("rows [%lld, + %lld): a range of reads", (long long)first_read, (long long)n_reads); return MNC_ERR_ARG; }
	if (cc->device != ab->device) { set_error("the carry is on device %d, the accumulator on device %d", cc->device, ab->device); return MNC_ERR_ARG; }
	if (cc->max_delta != ab->max_delta) { set_error("the carry was cut at max_delta %d, the accumulator's is %d", cc->max_delta, ab->max_delta); return MNC_ERR_ARG; }
	if (n_reads > cc->cap || first_read > cc->cap - n_reads) {
		set_error("rows [%lld, %lld) of a carry of %lld", (long long)first_read, (long long)(first_read + n_reads), (long long)cc->cap);
		return MNC_ERR_RANGE;
	}
	unsigned long long s[4];
	if (int rc = carry_stats(cc, s)) return rc;
	if ((int64_t)s[3] > ab->G) { set_error("the carry holds genome id %lld, the accumulator has %d genomes", (long long)s[3] - 1, ab->G); return MNC_ERR_ARG; }
	if (n_reads == 0 || ab->G == 0) return MNC_OK;
	HIP_TRY(hipSetDevice(ab->device));
	std::lock_guard<std::mutex> lk(ab->mu);
	if (int rc = carry_read_begin(cc, ab->st)) return rc;
	hipLaunchKernelGGL(mnc_ab_collect_carry, dim3((unsigned)((n_reads + 3) / 4)), dim3(256), 0, ab->st, cc->head, cc->slots, (int)cc->width, first_read, n_reads, ab->G,
	                   ab->cap_cands, ab->cap_rows, ab->unique, ab->offsets, ab->genome, ab->delta, ab->ctr);
	HIP_TRY(hipGetLastError());
	HIP_TRY(ab->own_done());                                   // an engine's add, and whatever changes the carry, comes behind it
	return carry_read_end(cc, ab->ev_own);
}

extern "C" int mnc_abundance_reset(mnc_abundance *ab)
{
	if (!ab) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(ab->device));
	std::lock_guard<std::mutex> lk(ab->mu);
	HIP_TRY(hipMemsetAsync(ab->unique, 0, ab->G ? (size_t)ab->G * 8 : 8, ab->st));
	HIP_TRY(hipMemsetAsync(ab->offsets, 0, 8, ab->st));        // offsets[0]: the CSR of no rows
	HIP_TRY(hipMemsetAsync(ab->ctr, 0, ABC_N * 8, ab->st));
	HIP_TRY(ab->own_done());
	return MNC_OK;
}

extern "C" int mnc_abundance_device_bytes(const mnc_abundance *ab, int64_t *bytes) { return accum_device_bytes(ab, bytes); }

extern "C" int mnc_abundance_device(mnc_abundance *ab, const int64_t **d_unique, const int64_t **d_offsets, const int32_t **d_genome, const int32_t **d_delta)
{
	if (!ab) return MNC_ERR_ARG;
	if (d_unique) *d_unique = ab->G ? ab->unique : nullptr;
	if (d_offsets) *d_offsets = ab->offsets;
	if (d_genome) *d_genome = ab->cap_cands ? ab->genome : nullptr;
	if (d_delta) *d_delta = ab->cap_cands ? ab->delta : nullptr;
	return MNC_OK;
}

extern "C" int mnc_abundance_info(mnc_abundance *ab, int64_t *n_reads, int64_t *n_stored_reads, int64_t *n_cands, int64_t *n_dropped)
{
	if (!ab) return MNC_ERR_ARG;
	unsigned long long c[ABC_N];
	if (int rc = ab_counters(ab, c)) return rc;
	if (n_reads) *n_reads = (int64_t)c[ABC_READS];
	if (n_stored_reads) *n_stored_reads = (int64_t)(c[ABC_PACK] >> AB_SLOT_BITS);
	if (n_cands) *n_cands = (int64_t)(c[ABC_PACK] & AB_SLOT_MASK);
	if (n_dropped) *n_dropped = (int64_t)c[ABC_DROPPED];
	return MNC_OK;
}

extern "C" int mnc_abundance_fetch_unique(mnc_abundance *ab, int64_t *unique)
{
	if (!ab || (!unique && ab->G)) return MNC_ERR_ARG;
	if (!ab->G) return MNC_OK;
	HIP_TRY(hipSetDevice(ab->device));
	HIP_TRY(hipMemcpyAsync(unique, ab->unique, (size_t)ab->G * 8, hipMemcpyDeviceToHost, ab->st));
	HIP_TRY(hipStreamSynchronize(ab->st));
	return MNC_OK;
}

// the stored rows on the host, as they stand: offsets[n_rows + 1], genome / delta [n_cands]
static int ab_rows_to_host(mnc_abundance *ab, std::vector<int64_t> &off, std::vector<int32_t> &gen, std::vector<int32_t> &del)
{
	unsigned long long c[ABC_N];
	if (int rc = ab_counters(ab, c)) return rc;
	const size_t n_rows = (size_t)(c[ABC_PACK] >> AB_SLOT_BITS), n_cands = (size_t)(c[ABC_PACK] & AB_SLOT_MASK);
	try {
		off.assign(n_rows + 1, 0), gen.assign(n_cands, 0), del.assign(n_cands, 0);
	} catch (const std::bad_alloc &) { return MNC_ERR_NOMEM; }
	HIP_TRY(hipMemcpyAsync(off.data(), ab->offsets, (n_rows + 1) * 8, hipMemcpyDeviceToHost, ab->st));
	if (n_cands) {
		HIP_TRY(hipMemcpyAsync(gen.data(), ab->genome, n_cands * 4, hipMemcpyDeviceToHost, ab->st));
		HIP_TRY(hipMemcpyAsync(del.data(), ab->delta, n_cands * 4, hipMemcpyDeviceToHost, ab->st));
	}
	HIP_TRY(hipStreamSynchronize(ab->st));
	return MNC_OK;
}

extern "C" int mnc_abundance_fetch_lists(mnc_abundance *ab, int64_t *offsets, int32_t *genome, int32_t *delta, int64_t cap_reads, int64_t cap_cands)
{
	if (!ab || !offsets || cap_reads < 0 || cap_cands < 0) return MNC_ERR_ARG;
	std::vector<int64_t> off;
	std::vector<int32_t> gen, del;
	if (int rc = ab_rows_to_host(ab, off, gen, del)) return rc;
	const int64_t n_rows = (int64_t)off.size() - 1, n_cands = (int64_t)gen.size();
	if (cap_reads < n_rows || cap_cands < n_cands) {
		set_error("%lld rows of %lld candidates, room for %lld and %lld", (long long)n_rows, (long long)n_cands, (long long)cap_reads, (long long)cap_cands);
		return MNC_ERR_RANGE;
	}
	if (n_cands && (!genome || !delta)) return MNC_ERR_ARG;
	// lexicographic by the row's (genome, delta) sequence; a row that is a prefix of another comes first
	std::vector<int64_t> order;
	try {
		order.resize((size_t)n_rows);
	} catch (const std::bad_alloc &) { return MNC_ERR_NOMEM; }
	for (int64_t r = 0; r < n_rows; ++r) order[(size_t)r] = r;
	std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
		const int64_t ax = off[(size_t)x], nx = off[(size_t)x + 1] - ax, ay = off[(size_t)y], ny = off[(size_t)y + 1] - ay;
		for (int64_t j = 0; j < nx && j < ny; ++j) {
			if (gen[(size_t)(ax + j)] != gen[(size_t)(ay + j)]) return gen[(size_t)(ax + j)] < gen[(size_t)(ay + j)];
			if (del[(size_t)(ax + j)] != del[(size_t)(ay + j)]) return del[(size_t)(ax + j)] < del[(size_t)(ay + j)];
		}
		return nx < ny;
	});
	int64_t at = 0;
	offsets[0] = 0;
	for (int64_t i = 0; i < n_rows; ++i) {
		const int64_t a = off[(size_t)order[(size_t)i]], n = off[(size_t)order[(size_t)i] + 1] - a;
		for (int64_t j = 0; j < n; ++j) genome[at + j] = gen[(size_t)(a + j)], delta[at + j] = del[(size_t)(a + j)];
		at += n, offsets[i + 1] = at;
	}
	return MNC_OK;
}

extern "C" int mnc_abundance_add_lists(mnc_abundance *ab, int64_t n_reads, const int64_t *offsets, const int32_t *genome, const int32_t *delta)
{
	if (!ab || n_reads < 0 || (n_reads && !offsets)) return MNC_ERR_ARG;
	if (n_reads == 0) return MNC_OK;
	// ---- every check on the host, before anything is touched
	if (offsets[0] < 0 || (offsets[n_reads] > offsets[0] && (!genome || !delta))) return MNC_ERR_ARG;
	std::vector<int64_t> uniq, off;
	std::vector<int32_t> gen, del;
	try {
		uniq.assign((size_t)ab->G + 1, 0);
		off.push_back(0);
		for (int64_t r = 0; r < n_reads; ++r) {
			const int64_t a = offsets[r], b = offsets[r + 1];
			if (b <= a) { set_error("row %lld is empty (offsets %lld, %lld)", (long long)r, (long long)a, (long long)b); return MNC_ERR_ARG; }
			for (int64_t j = a; j < b; ++j) {
				if (genome[j] < 0 || genome[j] >= ab->G || (j > a && genome[j] <= genome[j - 1])) {
					set_error("row %lld: genome ids must ascend strictly within 0 .. %d", (long long)r, ab->G - 1);
					return MNC_ERR_ARG;
				}
				if (delta[j] < 0 || delta[j] > ab->max_delta) { set_error("row %lld: delta %d outside 0 .. %d", (long long)r, delta[j], ab->max_delta); return MNC_ERR_ARG; }
			}
			if (b - a == 1) { ++uniq[(size_t)genome[a]]; continue; }
			gen.insert(gen.end(), genome + a, genome + b), del.insert(del.end(), delta + a, delta + b);
			off.push_back((int64_t)gen.size());
		}
	} catch (const std::bad_alloc &) { return MNC_ERR_NOMEM; }
	unsigned long long c[ABC_N];
	if (int rc = ab_counters(ab, c)) return rc;                // (waits for the adds queued so far)
	const int64_t rows0 = (int64_t)(c[ABC_PACK] >> AB_SLOT_BITS), slots0 = (int64_t)(c[ABC_PACK] & AB_SLOT_MASK);
	const int64_t n_rows = (int64_t)off.size() - 1, n_slots = (int64_t)gen.size();
	if (slots0 + n_slots > ab->cap_cands || rows0 + n_rows > ab->cap_rows) {
		set_error("%lld candidates in %lld rows do not fit: %lld of %lld slots are taken", (long long)n_slots, (long long)n_rows, (long long)slots0, (long long)ab->cap_cands);
		return MNC_ERR_RANGE;
	}
	for (int64_t &o : off) o += slots0;
	int64_t *d_inc = nullptr;
	HIP_TRY(hipMalloc((void**)&d_inc, uniq.size() * 8));
	std::lock_guard<std::mutex> lk(ab->mu);
	hipError_t he = hipMemcpyAsync(d_inc, uniq.data(), uniq.size() * 8, hipMemcpyHostToDevice, ab->st);
	if (he == hipSuccess && n_rows) he = hipMemcpyAsync(ab->offsets + rows0, off.data(), (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, ab->st);
	if (he == hipSuccess && n_slots) he = hipMemcpyAsync(ab->genome + slots0, gen.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, ab->st);
	if (he == hipSuccess && n_slots) he = hipMemcpyAsync(ab->delta + slots0, del.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, ab->st);
	if (he == hipSuccess) {
		const unsigned long long pack = (unsigned long long)(rows0 + n_rows) << AB_SLOT_BITS | (unsigned long long)(slots0 + n_slots);
		hipLaunchKernelGGL(mnc_ab_append, dim3((unsigned)std::min<int64_t>(((int64_t)ab->G + 255) / 256 + 1, 256)), dim3(256), 0, ab->st, ab->G, d_inc, ab->unique, ab->ctr,
		                   pack, (unsigned long long)n_reads);
		he = hipGetLastError();
	}
	if (he == hipSuccess) he = ab->own_done();                   // an engine's add comes behind it
	const hipError_t hs = hipStreamSynchronize(ab->st);          // the host arrays above are read until here
	if (he == hipSuccess) he = hs;
	(void)hipFree(d_inc);
	if (he != hipSuccess) { set_error("abundance add_lists: %s", hipGetErrorString(he)); return MNC_ERR_HIP; }
	return MNC_OK;
}

extern "C" int mnc_abundance_solve(mnc_abundance *ab, int32_t max_iter, uint64_t tol_q32, double *theta, double *expected, int32_t *iters)
{
	if (!ab || !iters || ((!theta || !expected) && ab->G)) return MNC_ERR_ARG;
	if (max_iter < 1) { set_error("max_iter %d: at least one iteration", max_iter); return MNC_ERR_ARG; }
	*iters = 0;
	HIP_TRY(hipSetDevice(ab->device));
	const int G = ab->G;
	const bool lds = G <= AB_LDS_G;
	const int wg = (int)std::max<int64_t>(1, std::min<int64_t>(AB_PASS_WG, (ab->cap_rows + 255) / 256));
	unsigned long long c[ABC_N] = {0, 0, 0, 0}, s[ABS_N] = {0, 0, 0, 0};
	std::vector<unsigned long long> acc;                        // both buffers: which one holds the last iteration is in the state
	std::vector<double> th;
	try {
		acc.resize((size_t)G * 2 + 1), th.resize((size_t)G + 1);
	} catch (const std::bad_alloc &) { return MNC_ERR_NOMEM; }
	hipLaunchKernelGGL(mnc_ab_init, dim3(1), dim3(1024), 0, ab->st, G, ab->unique, ab->ctr, ab->theta, ab->acc, ab->state);
	for (int k = 0; k < max_iter;) {
		for (const int end = (int)std::min<int64_t>(max_iter, (int64_t)k + AB_LAUNCH_BLOCK); k < end; ++k) {
			const int which = k & 1;
			unsigned long long *into = ab->acc + (size_t)which * G;
			if (lds) hipLaunchKernelGGL(mnc_ab_pass<true>, dim3(wg), dim3(256), 0, ab->st, G, (int)ab->scale_q, ab->offsets, ab->genome, ab->delta, ab->ctr, ab->theta, into, ab->state);
			else hipLaunchKernelGGL(mnc_ab_pass<false>, dim3(wg), dim3(256), 0, ab->st, G, (int)ab->scale_q, ab->offsets, ab->genome, ab->delta, ab->ctr, ab->theta, into, ab->state);
			hipLaunchKernelGGL(mnc_ab_finish, dim3(1), dim3(1024), 0, ab->st, G, (unsigned long long)tol_q32, which, ab->unique, ab->theta, ab->acc, ab->state);
		}
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(s, ab->state, ABS_N * 8, hipMemcpyDeviceToHost, ab->st));
		HIP_TRY(hipMemcpyAsync(c, ab->ctr, ABC_N * 8, hipMemcpyDeviceToHost, ab->st));
		if (G) {
			HIP_TRY(hipMemcpyAsync(th.data(), ab->theta, (size_t)G * 8, hipMemcpyDeviceToHost, ab->st));
			HIP_TRY(hipMemcpyAsync(acc.data(), ab->acc, (size_t)G * 16, hipMemcpyDeviceToHost, ab->st));
		}
		HIP_TRY(hipStreamSynchronize(ab->st));                    // the one wait (one per AB_LAUNCH_BLOCK iterations)
		if (s[ABS_DONE]) break;
	}
	if (c[ABC_DROPPED]) {
		set_error("%llu rows were dropped for lack of candidate slots (cap_cands %lld): reset and collect again into a larger accumulator", c[ABC_DROPPED], (long long)ab->cap_cands);
		return MNC_ERR_RANGE;
	}
	for (int g = 0; g < G; ++g) theta[g] = expected[g] = 0.0;
	if (c[ABC_READS] == 0 || G == 0) return MNC_OK;
	*iters = (int32_t)s[ABS_ITERS];
	for (int g = 0; g < G; ++g) theta[g] = th[(size_t)g], expected[g] = (double)acc[(size_t)s[ABS_LAST] * G + g] / 4294967296.0;
	return MNC_OK;
}
