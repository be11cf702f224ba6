// What k_abundance.hip and k_carry.hip share: how one wave finds a read's candidate genomes among the records of a batch as
// it stands in HBM -- the records that count, the read's best score, and the genomes in ascending id by extraction -- and
// the candidate carry's handle, which both files and engine.hip see.
#pragma once

#include <hip/hip_runtime.h>
#include "device.h"
#pragma clang diagnostic push                  // (the header's scan kernels are for the two accumulators over the reference bases)
#pragma clang diagnostic ignored "-Wunused-function"
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "cov_common.h"
#pragma clang diagnostic pop
#include "accum.h"

namespace mnc {

__device__ __forceinline__ unsigned long long ab_wave_min(unsigned long long x)
{
	for (int d = 32; d > 0; d >>= 1) {
		const unsigned long long o = __shfl_xor(x, d);
		x = o < x ? o : x;
	}
	return x;
}

// the key of one record: genome in the high word, the score inverted in the low one (order-preserving for any int32), so
// that the minimum is the smallest genome and within it the largest score
__device__ __forceinline__ unsigned long long ab_key(int g, int s) { return (unsigned long long)(uint32_t)g << 32 | (uint32_t)~((uint32_t)s ^ 0x80000000u); }
__device__ __forceinline__ int ab_key_score(unsigned long long k) { return (int)(~(uint32_t)k ^ 0x80000000u); }

// a record that counts: selected as MNC_COV_ALL selects, on a contig of the index, with a CIGAR
__device__ __forceinline__ bool ab_counted(const Batch &B, const mnc_reg_t &r, int n_contigs)
{
	return cov_selected(r, MNC_COV_ALL, B.min_mapq) && r.rid >= 0 && r.rid < n_contigs && r.n_cigar > 0;
}

// the largest dp_max of the read's records that count, over the whole wave; false when there is none
__device__ __forceinline__ bool ab_best(const Batch &B, int64_t slot0, int n, int n_contigs, int n_genomes, int &best)
{
	bool any = false;
	best = INT32_MIN;
	for (int i = lane_id(); i < n; i += 64) {
		const mnc_reg_t &r = B.regs[slot0 + i];
		if (!ab_counted(B, r, n_contigs)) continue;
		const int g = B.contig_genome[r.rid];
		if (g < 0 || g >= n_genomes) continue;
		any = true, best = r.dp_max > best ? r.dp_max : best;
	}
	if (!__ballot(any)) return false;
	for (int d = 32; d > 0; d >>= 1) {
		const int o = __shfl_xor(best, d);
		best = o > best ? o : best;
	}
	return true;
}

// the smallest key above genome `last` among the read's records that count; ~0 when there is none
__device__ __forceinline__ unsigned long long ab_next(const Batch &B, int64_t slot0, int n, int n_contigs, int n_genomes, int last)
{
	unsigned long long k = ~0ull;
	for (int i = lane_id(); i < n; i += 64) {
		const mnc_reg_t &r = B.regs[slot0 + i];
		if (!ab_counted(B, r, n_contigs)) continue;
		const int g = B.contig_genome[r.rid];
		if (g <= last || g >= n_genomes) continue;
		const unsigned long long x = ab_key(g, r.dp_max);
		k = x < k ? x : k;
	}
	return ab_wave_min(k);
}

// ---------------------------------------------------------------- the candidate carry (k_carry.hip)
constexpr int CARRY_MAX_WIDTH = 64;            // a row lives in one wave's registers, one slot per lane
constexpr int CARRY_USED = 1, CARRY_TRUNCATED = 2;   // head[r].y

} // namespace mnc

// One row per read of a sample: head[r] = (best, CARRY_* flags), slots[r * width + i] = (global genome id, score), a free
// slot (-1, 0), in no particular order.  ev_add: the last merge (merges wait for one another: `serial`); ev_own: the last
// reset, add_lists, merge as dst or as the source of somebody's read.
struct mnc_carry : mnc::Accum {
	int64_t cap = 0;
	int32_t width = 0, max_delta = 0;
	int2 *head = nullptr;                      // [cap]
	int2 *slots = nullptr;                     // [cap][width]
	unsigned long long *stat = nullptr;        // [4]: rows used, pairs, truncated rows, the largest genome id + 1
};

namespace mnc {

// the rows of `cc` are read by work queued on `on` (another accumulator's stream): it comes behind the merges queued so far
int carry_read_begin(mnc_carry *cc, hipStream_t on);
// ... and whatever changes `cc` later comes behind that work, which `done` (recorded on `on`) marks
int carry_read_end(mnc_carry *cc, hipEvent_t done);
// rows used, pairs, truncated rows, the largest genome id + 1, as they stand behind everything queued so far (waits)
int carry_stats(mnc_carry *cc, unsigned long long *s);

} // namespace mnc
