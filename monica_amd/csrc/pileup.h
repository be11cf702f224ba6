// What the two units of the pileup share (k_pileup.hip: the planes, their add kernel and read-outs; k_pile_ins.hip: the
// insertion store's kernels and read-outs): the accumulator's struct, the walk of one read's records with one lane per
// column (pile_add_read; <true> also hands every I operation to the store), and the read-outs' pass over the tiles
// (mnc_pile_scan).  k_pileup.hip's header comment describes them.  A third unit, k_pile_strand.hip, holds the opt-in strand
// store: the same walk with the forward records' own planes and a base-quality mask, and the read-outs by strand.
#pragma once

#include <hip/hip_runtime.h>
#include <vector>
#include "device.h"
#include "scan.h"
#include "cov_scan.h"
#include "accum.h"
#include "pile_ins.h"

static_assert(sizeof(mnc_variant_t) == 20, "mnc_variant_t is 4 int32 and 4 bytes (monica_amd/_capi.py: VARIANT_DTYPE)");

constexpr int PILE_ALT = MNC_PILE_PLANES - 1;   // channels of `alt`: A C G T N DEL INS
constexpr int CH_N = 4, CH_DEL = 5, CH_INS = 6;

struct mnc_pileup : mnc::Accum {
	mnc::DeviceIndex *didx = nullptr;               // the index on this device: the reference bases of the read-outs
	int n_contigs = 0;
	int64_t n_words = 0;                       // = the index's total_len
	std::vector<int64_t> off;                  // n_contigs + 1
	int32_t *track = nullptr;                  // [n_words] depth differences
	int32_t *alt = nullptr;                    // [PILE_ALT][n_words]
	int64_t *d_off = nullptr;                  // [n_contigs + 1]
	long long *cbase = nullptr;                // [n_contigs] running sum of the track before the contig (scratch)
	int64_t *tile_sums = nullptr, *tile_cnt = nullptr, *tile_voff = nullptr;   // [n_words / SC_TILE + 2] each (scratch)
	int64_t *sums2 = nullptr;                  // the scan over tile_cnt's own tile sums (scratch)
	bool ins_on = false;                       // mnc_pileup_store_insertions was called: `ins` is the allele table (pile_ins.h)
	bool added = false;                        // something has been added since creation (under `mu`)
	mnc::InsTable ins{};
	// ---- the strand store (mnc_pileup_store_strands, k_pile_strand.hip): 40 more bytes per reference base
	bool strands_on = false;
	int min_qual = 0;                          // an M column whose read base has a Phred below it is masked; 0: no mask
	int32_t *track_f = nullptr;                // [n_words] depth differences of the forward records
	int32_t *alt_f = nullptr;                  // [PILE_ALT][n_words] ... and their channels
	int32_t *lowq = nullptr;                   // [2][n_words] masked M columns: of both strands, of the forward records
	long long *cbase_f = nullptr;              // cbase and tile_sums once more, for track_f (scratch)
	int64_t *tile_sums_f = nullptr;
	// what the read-outs of both strands subtract from the depth: nothing without a mask (today's code)
	const int32_t *lowq_view() const { return min_qual > 0 ? lowq : nullptr; }
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

// the strand store's side of the add (k_pile_strand.hip): its planes, and the batch's quality characters (Phred + 33, laid
// out as the bases are) with the floor below which an M column is masked
struct PileStrands {
	int32_t *track_f, *alt_f, *lowq;
	const uint8_t *quals;
	int min_qual;
};

// INS: the insertion store is on -- the lane of an I column hands its operation to ins_wave_add (pile_ins.h), and that is
// all the difference: the planes get what they get without it.
// STR: the strand store is on -- a forward record (wave-uniform: a wave holds one read, and `rev` is the record's) repeats
// its depth runs in track_f and every atomic it issues on `alt` in alt_f.  QUAL: an M lane also loads the quality byte of
// its read base; below the floor it issues no `alt` atomic, match or not, and counts the column in lowq (and lowq's forward
// half).  The depth runs are NOT broken at a masked column: the read-outs subtract lowq.  Without STR and QUAL nothing of
// this is instantiated.
template <bool INS, bool STR = false, bool QUAL = false>
__device__ __forceinline__ void pile_add_read(const Batch &B, int sel, const int64_t *off, int n_contigs, int64_t n_words, int32_t *track, int32_t *alt, const InsTable &T,
                                              const PileStrands &S = PileStrands{})
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
		const bool fwd = STR && !r.rev;
		int32_t *wf = STR ? S.track_f + coff : nullptr, *af = STR ? S.alt_f + coff : nullptr, *lq = QUAL ? S.lowq + coff : nullptr;
		const uint32_t *src = B.cig_reg + B.regdp[slot].cig_off;
		auto At = [&](int p) -> int {                           // the read base of column p of the query side
			const int at = r.rev ? r.qe - 1 - p : r.qs + p;
			return at < 0 ? 0 : at >= qlen ? qlen - 1 : at;
		};
		auto Q = [&](int p) -> int {                            // column p of the query side, on the hit's strand (k_export.hip)
			const int c = base_nt4(read[At(p)]);
			return r.rev ? (c < 4 ? 3 - c : 4) : c;
		};
		// one observation of channel ch at base p; a forward record's goes to its own planes as well
		auto put = [&](int ch, int64_t p) {
			pile_put(a + (int64_t)ch * n_words, len, p);
			if (fwd) pile_put(af + (int64_t)ch * n_words, len, p);
		};
		int64_t toff = r.rs;                                   // reference position before the chunk at hand
		int qoff = 0;                                          // query columns before it
		bool open = false;                                     // a run is open: the last M / D operation so far was an M
		bool open_f = false;                                   // STR: the same for the forward track
		int claims = 0;                                        // INS: the alleles this wave has claimed in this record (pile_ins.h)
		for (int k0 = 0; k0 < n_c; k0 += 64) {
			const bool full = INS && ins_full(T);
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
			if (fwd) cov_run_step(wf, len, l > 0 && op == 0, l > 0 && op == 2, toff + my_t0, open_f);
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
				const int o_l = INS ? __shfl(l, o) : 0;
				const int x = c - (o_end - o_cols);                  // column within the operation
				const int64_t p = toff + t0 + x;
				bool stored = false;                                // an I that the INS plane counts: its bases go to the store
				if (valid) {
					if (o_op == 0) {
						if (p >= 0 && p < len) {
							bool masked = false;
							if (QUAL) {
								const int phred = (int)S.quals[read_off + At(q0 + x)] - 33;   // (below '!': Phred 0)
								masked = phred < S.min_qual;
							}
							if (masked) {
								pile_put(lq, len, p);
								if (fwd) pile_put(lq + n_words, len, p);
							} else {
								const int qc = Q(q0 + x), tc = pile_ref(B.seq4, coff + p);
								if (tc == 4 || qc != tc) put(qc, p);
							}
						}
					} else if (o_op == 2) put(CH_DEL, p);
					else if (p > r.rs) {                                 // a reference column of this record lies on its left
						put(CH_INS, p - 1);
						stored = p - 1 >= 0 && p - 1 < len;
					}
				}
				// (every lane of the wave is here: the trip count is the wave's, and nothing above leaves the loop)
				if (INS) ins_wave_add(T, stored, coff + p - 1, o_l, 1, (long long)q0, [&](long long s, int j) { return Q((int)s + j); }, full, claims);
			}
			toff += __shfl(it, 63), qoff += __shfl(iq, 63);
		}
		cov_run_close(w, len, toff, open);
		if (fwd) cov_run_close(wf, len, toff, open_f);
		if (INS) ins_flush(T, claims);
	});
}

// ---------------------------------------------------------------- read-outs
struct PileView {
	const int32_t *track, *alt;
	int64_t n_words;
	const uint32_t *seq4;
	const int64_t *off;
	int n_contigs;
	const int32_t *lowq = nullptr;            // the masked M columns of a pileup that masks by quality: taken off the depth
};
struct PileThr {
	int min_depth, min_count, min_permille;
	bool any_ref = false;                     // MODE 4: a reference N is no obstacle (the consensus with insertions)
};

// the full counts of one base: A C G T N DEL INS
struct PileBase {
	int cnt[PILE_ALT], depth, ref;
	__device__ __forceinline__ int span() const { return depth + cnt[CH_DEL]; }
	__device__ __forceinline__ int allele(int a) const { return a < 4 ? cnt[a] : cnt[a + 1]; }   // a: A C G T DEL INS
};

__device__ __forceinline__ PileBase pile_load(const PileView &P, int64_t g, int depth)
{
	PileBase b;
	if (P.lowq) depth -= P.lowq[g];
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
// tile_voff[tile] on   3: o_cons[n - start]   4: o_counts[n - start] = the span of a base an insertion allele may be called at
// (span >= min_depth; the reference base not N, unless thr.any_ref: the consensus asks no such thing), else -1
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
		else if (MODE == 4) o_counts[i - start] = b.span() >= thr.min_depth && (thr.any_ref || b.ref < 4) ? b.span() : -1;
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
static inline void pile_tile_sums(mnc_pileup *pu, int64_t w0, int64_t n, bool all)
{
	cov_tile_sums(pu->track + w0, n, pu->tile_sums, pu->d_off, pu->n_contigs, all ? pu->cbase : nullptr, pu->st);
}

template <int MODE>
static inline void pile_launch(mnc_pileup *pu, int64_t w0, int64_t n, bool all, int rid, int64_t start, PileThr thr, int32_t *o_counts, mnc_variant_t *o_var,
                        int64_t var_cap, char *o_cons)
{
	const PileView P{pu->track, pu->alt, pu->n_words, pu->didx->seq4, pu->d_off, pu->n_contigs, pu->lowq_view()};
	hipLaunchKernelGGL(mnc_pile_scan<MODE>, dim3((unsigned)((n + SC_TILE - 1) / SC_TILE)), dim3(SC_THREADS), 0, pu->st, P, w0, n, pu->tile_sums,
	                   all ? pu->cbase : nullptr, rid, start, thr, o_counts, pu->tile_cnt, pu->tile_voff, o_var, var_cap, o_cons);
}

// k_pile_ins.hip: the add with the store on (under the accumulator's `add`, as mnc_pile_add is launched), and the clearing of
// the table on the accumulator's own stream
void pileup_add_ins_launch(mnc_pileup *pu, const Batch &B, int sel, hipStream_t st);
hipError_t ins_clear(mnc_pileup *pu);
// k_pile_strand.hip: the add of a pileup with the strand store (d_quals: the batch's quality characters on the device, or
// nullptr where there is no mask), the clearing of its planes on the accumulator's own stream, and what an add checks first
void pileup_add_strands_launch(mnc_pileup *pu, const Batch &B, int sel, hipStream_t st, const uint8_t *d_quals);
hipError_t strands_clear(mnc_pileup *pu);

} // namespace mnc
