// What the two accumulators over the reference bases share (k_coverage.hip, k_pileup.hip): which records of a read a call
// adds (the selectors of include/monica_amd.h, "coverage"), the walk over them, the runs of M columns of a CIGAR in a
// depth-difference track under the contig-end rule, and the running sum in front of every contig that their scans subtract.
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

// The records of read `rd` that a call with selector `sel` adds: f(record, its region slot) for each one that is selected
// and lies on a contig of the accumulator, in slot order.  A read's live region slots are reg_slot(rd) .. + n_reg[rd], as
// k_export.hip finds them: no scan over the batch, no record list, no host wait.
template <class F>
__device__ __forceinline__ void cov_for_records(const Batch &B, uint32_t rd, int sel, int n_contigs, F f)
{
	const int n = B.n_reg[rd];
	if (n <= 0) return;
	const int64_t slot0 = reg_slot(B, rd);
	const int pick = sel == MNC_COV_ASSIGNED ? cov_pick(B, rd, slot0, n) : -1;
	if (sel == MNC_COV_ASSIGNED && pick < 0) return;
	for (int i = pick < 0 ? 0 : pick; i < (pick < 0 ? n : pick + 1); ++i) {
		const mnc_reg_t r = B.regs[slot0 + i];
		if (cov_selected(r, sel, B.min_mapq) && r.rid >= 0 && r.rid < n_contigs) f(r, slot0 + i);
	}
}

// The depth runs of one chunk of 64 CIGAR operations, one operation per lane of a whole wave: this lane's is an M (is_M)
// or a D (is_D) of at least one base that starts at base t0 of the contig, or neither.  A covered run is a maximal stretch
// of M columns without a D (insertions consume no reference and do not break it): the M lane whose nearest M / D neighbour
// below is a D (or none, with no run carried in) opens it, the D lane whose nearest neighbour below is an M closes it at its
// own start.  `open` -- the last M / D operation so far was an M -- is all that crosses a chunk border; cov_run_close, after
// the last chunk with the reference position behind the record, lets lane 0 close the last run.
__device__ __forceinline__ void cov_run_step(int32_t *w, int64_t len, bool is_M, bool is_D, int64_t t0, bool &open)
{
	const unsigned long long m_M = __ballot(is_M), m_D = __ballot(is_D);
	const unsigned long long below = (m_M | m_D) & ((1ull << lane_id()) - 1ull);
	const bool prev_M = below ? (m_M >> (63 - __clzll((long long)below)) & 1ull) != 0 : open;
	if (is_M && !prev_M) cov_put(w, len, t0, 1);
	if (is_D && prev_M) cov_put(w, len, t0, -1);
	const unsigned long long any = m_M | m_D;
	if (any) open = (m_M >> (63 - __clzll((long long)any)) & 1ull) != 0;
}

__device__ __forceinline__ void cov_run_close(int32_t *w, int64_t len, int64_t t_end, bool open)
{
	if (open && lane_id() == 0) cov_put(w, len, t_end, -1);
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
