// What the two accumulators over the reference bases share (k_coverage.hip, k_pileup.hip): which records of a read a call
// adds (the selectors of include/monica_amd.h, "coverage"), one end of a run in a depth-difference track under the
// contig-end rule, and the running sum in front of every contig that their scans subtract.
#pragma once

#include <hip/hip_runtime.h>
#include "device.h"
#include "scan.h"

namespace mnc {

__device__ __forceinline__ int cov_incl_add(int x)
{
	const int lane = lane_id();
	for (int d = 1; d < 64; d <<= 1) {
		const int o = __shfl_up(x, d);
		if (lane >= d) x += o;
	}
	return x;
}

// one end of a run at base `pos` of a contig of `len` bases whose first word is `w`: without a return value.  An end
// at `len` is the -1 of a run that reaches the contig's last base -- dropped (the contig-end rule, k_coverage.hip); nothing is
// ever written outside the contig's own words.
__device__ __forceinline__ void cov_put(int32_t *w, int64_t len, int64_t pos, int v)
{
	if (pos >= 0 && pos < len) (void)__hip_atomic_fetch_add(w + pos, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool cov_selected(const mnc_reg_t &r, int sel, int min_mapq)
{
	const bool primary = r.id == r.parent;
	return sel == MNC_COV_ALL || (sel == MNC_COV_PRIMARY && primary) || (primary && r.mapq >= min_mapq);   // GATED, and ASSIGNED's candidates
}

// MNC_COV_ASSIGNED: the record best_hit chose among the gated ones of a read whose decision is a contig -- the running
// minimum of NM / mlen by int64 cross-products, as gate_and_decide (k_post.hip) and mnc_best_hit keep it; -1: none
__device__ __forceinline__ int cov_pick(const Batch &B, uint32_t rd, int64_t slot0, int n)
{
	if (B.assign[rd] < 0) return -1;
	int pick = -1;
	long long b_nm = 0, b_mlen = 1;
	for (int i = 0; i < n; ++i) {
		const mnc_reg_t &x = B.regs[slot0 + i];
		if (x.id != x.parent || x.mapq < B.min_mapq) continue;
		const long long nm = x.blen - x.mlen + x.n_ambi, mlen = x.mlen;
		if (pick < 0 || nm * b_mlen <= b_nm * mlen) pick = i, b_nm = nm, b_mlen = mlen;
	}
	return pick;
}

// G(off[c] - 1) of every contig: the exclusive tile sum of the tile that holds the contig's first word plus the words
// of that tile in front of it (one wave per contig)
static __global__ __launch_bounds__(256) void mnc_cov_contig_base(const int32_t *track, const int64_t *off, int n_contigs, const int64_t *tile_pre, long long *cbase)
{
	const int c = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
	if (c >= n_contigs) return;
	const int64_t s = off[c];
	long long x = 0;
	if (off[c + 1] > s) {                                      // (an empty contig has no word, and no tile, of its own)
		const int64_t t = s / SC_TILE;
		for (int64_t i = t * SC_TILE + lane_id(); i < s; i += 64) x += track[i];
		for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
		x += tile_pre[t];
	}
	if (lane_id() == 0) cbase[c] = x;
}

} // namespace mnc
