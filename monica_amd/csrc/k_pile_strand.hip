// The strand store of a pileup (include/monica_amd.h, "pileup": strands and base qualities): which strand an observation
// came from and whether its base was good enough to count -- the two standard filters against false variant calls on
// nanopore reads (an allele must be seen on both strands; a base below a quality floor is no evidence).  Opt-in per
// accumulator (mnc_pileup_store_strands); a pileup without it runs k_pileup.hip's and k_pile_ins.hip's kernels as ever.
//
// The planes, beside the eight words of k_pileup.hip, ten more per reference base (72 bytes in all), laid out alike:
//   track_f [n_words]      depth differences of the FORWARD records (rev == 0) only: a second cov_run_step / cov_run_close
//                          under a wave-uniform branch -- a wave holds one read, and `rev` is the record's
//   alt_f   [7][n_words]   the forward records' channels: one more atomic wherever a forward record issues one on `alt`
//   lowq    [2][n_words]   masked M columns, of both strands and of the forward records
// A reference match still costs no atomic.  What is new is the mask: an M lane loads the quality byte of its read base (at
// the index its base comes from, reversed for a reverse record); below the floor it issues no `alt` atomic and counts the
// column in lowq -- one atomic, two for a forward record, for a reference match as well.  The depth runs are not broken at
// a masked column: every read-out subtracts lowq from the depth (PileView::lowq), so one accumulator has one meaning and
// the existing read-outs report the masked pileup through the depth and the spans they already compute.
//
//   mnc_pile_add_str        pileup.h's walk with the store on, by (insertion store, qualities)
//   mnc_pile_scan_strands   the read-outs by strand: ONE pass over the tiles of scan.h with TWO running sums, the depth of
//                           both strands and of the forward records (a second set of tile sums and of sums in front of the
//                           contigs, for track_f).  Per strand the reference's counts are reconstructed as pile_load does;
//                           reverse is total minus forward, word for word, because every plane is additive.  MODE 0 writes
//                           the 18 planes; the variants take MODE 1 (calls per tile), scan.h's exclusive scan and MODE 2
//                           (place), the scheme of mnc_pile_scan: compacted and in (contig, position, allele) order.
#include <hip/hip_runtime.h>
#include <new>
#include "pileup.h"

using namespace mnc;

static_assert(sizeof(mnc_variant_strand_t) == 28, "mnc_variant_strand_t is mnc_variant_t and 2 int32 (monica_amd/_capi.py: VARIANT_STRAND_DTYPE)");
static_assert(MNC_PILE_FWD == MNC_PILE_PLANES && MNC_PILE_LOWQ == 2 * MNC_PILE_PLANES && MNC_PILE_STRAND_PLANES == MNC_PILE_LOWQ_FWD + 1, "the 18 planes");

namespace mnc {

template <bool INS, bool QUAL>
__global__ __launch_bounds__(256) void mnc_pile_add_str(Batch B, int sel, const int64_t *off, int n_contigs, int64_t n_words, int32_t *track, int32_t *alt, InsTable T,
                                                        PileStrands S)
{
	pile_add_read<INS, true, QUAL>(B, sel, off, n_contigs, n_words, track, alt, T, S);
}

// (under the accumulator's `add`, as mnc_pile_add is launched; the store is on)
void pileup_add_strands_launch(mnc_pileup *pu, const Batch &B, int sel, hipStream_t st, const uint8_t *d_quals)
{
	const PileStrands S{pu->track_f, pu->alt_f, pu->lowq, d_quals, pu->min_qual};
	const dim3 grid((B.n_reads + 3) / 4), block(256);
	const bool qual = pu->min_qual > 0;                        // (pileup_quals_check: the qualities are there then)
#define MNC_ADD_STR(I, Q) hipLaunchKernelGGL((mnc_pile_add_str<I, Q>), grid, block, 0, st, B, sel, pu->d_off, pu->n_contigs, pu->n_words, pu->track, pu->alt, pu->ins, S)
	if (pu->ins_on) { if (qual) MNC_ADD_STR(true, true); else MNC_ADD_STR(true, false); }
	else { if (qual) MNC_ADD_STR(false, true); else MNC_ADD_STR(false, false); }
#undef MNC_ADD_STR
}

// what an engine's add checks before it touches anything: qualities go to a strand store, and a store that masks needs them
int pileup_quals_check(const mnc_pileup *pu, bool with_quals)
{
	if (with_quals && !pu->strands_on) { set_error("the pileup has no strand store (mnc_pileup_store_strands was not called)"); return MNC_ERR_ARG; }
	if (!with_quals && pu->min_qual > 0) { set_error("this pileup masks by quality: add with qualities (mnc_engine_add_pileup_quals)"); return MNC_ERR_ARG; }
	return MNC_OK;
}
int pileup_min_qual(const mnc_pileup *pu) { return pu->min_qual; }

hipError_t strands_clear(mnc_pileup *pu)
{
	if (!pu->n_words) return hipSuccess;
	const size_t nw = (size_t)pu->n_words;
	hipError_t he = hipMemsetAsync(pu->track_f, 0, nw * 4, pu->st);
	if (he == hipSuccess) he = hipMemsetAsync(pu->alt_f, 0, nw * 4 * PILE_ALT, pu->st);
	if (he == hipSuccess) he = hipMemsetAsync(pu->lowq, 0, nw * 4 * 2, pu->st);
	return he;
}

// ---------------------------------------------------------------- read-outs by strand
struct StrandThr { int min_count, min_permille; };

// the alleles of `m` (pile_calls of both strands' counts) that each strand passes on its own: count_s >= min_count and
// count_s * 1000 >= min_permille * span_s, s = forward (f) and reverse (b - f)
__device__ __forceinline__ int strand_calls(const PileBase &b, const PileBase &f, int m, const StrandThr &t)
{
	const long long sf = f.span(), sr = b.span() - f.span();
	int out = 0;
	for (int a = 0; a < 6; ++a) {
		if (!(m >> a & 1)) continue;
		const long long cf = f.allele(a), cr = b.allele(a) - f.allele(a);
		if (cf >= t.min_count && cr >= t.min_count && cf * 1000 >= (long long)t.min_permille * sf && cr * 1000 >= (long long)t.min_permille * sr) out |= 1 << a;
	}
	return out;
}

// mnc_pile_scan's arguments, and beside them: F, the forward records' view; tile_pre_f / cbase_f, track_f's sums; lowq, the
// two planes of masked columns as they are (MODE 0 writes them out).
// MODE 0: o_counts[18][n - start]   1: tile_cnt[tile] = variants called in the tile   2: o_var, a tile's records from
// tile_voff[tile] on
template <int MODE>
__global__ __launch_bounds__(SC_THREADS) void mnc_pile_scan_strands(PileView P, PileView F, int64_t w0, int64_t n, const int64_t *tile_pre, const int64_t *tile_pre_f,
                                                                    const long long *cbase, const long long *cbase_f, int rid, int64_t start, PileThr thr, StrandThr sthr,
                                                                    const int32_t *lowq, int32_t *o_counts, int64_t *tile_cnt, const int64_t *tile_voff,
                                                                    mnc_variant_strand_t *o_var, int64_t var_cap)
{
	__shared__ long long s[2][SC_THREADS / 64];
	__shared__ int s_n[SC_THREADS / 64];
	const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
	const int64_t base = (int64_t)blockIdx.x * SC_TILE + (int64_t)threadIdx.x * SC_ITEMS, m = n - start;
	int v[SC_ITEMS], vf[SC_ITEMS];
	long long x = 0, xf = 0;
	for (int k = 0; k < SC_ITEMS; ++k) {
		v[k] = base + k < n ? P.track[w0 + base + k] : 0, vf[k] = base + k < n ? F.track[w0 + base + k] : 0;
		x += v[k], xf += vf[k];
	}
	long long inc = x, incf = xf;
	for (int d = 1; d < 64; d <<= 1) {
		const long long o = __shfl_up(inc, d), of = __shfl_up(incf, d);
		if (lane >= d) inc += o, incf += of;
	}
	if (lane == 63) s[0][wave] = inc, s[1][wave] = incf;
	__syncthreads();
	long long pre = tile_pre[blockIdx.x] + inc - x, pre_f = tile_pre_f[blockIdx.x] + incf - xf;
	for (int w = 0; w < wave; ++w) pre += s[0][w], pre_f += s[1][w];
	int c = rid;
	long long cb = 0, cbf = 0;
	if (cbase && base < n) {                                  // the contig of this thread's first word: the last c with off[c] <= it
		int lo = 0, hi = P.n_contigs;
		while (hi - lo > 1) {
			const int mid = lo + (hi - lo) / 2;
			if (P.off[mid] <= w0 + base) lo = mid; else hi = mid;
		}
		c = lo, cb = cbase[c], cbf = cbase_f[c];
	}
	int mask[SC_ITEMS], dep[SC_ITEMS], depf[SC_ITEMS], ctg[SC_ITEMS], n_call = 0;
	for (int k = 0; k < SC_ITEMS; ++k) {
		const int64_t i = base + k;
		pre += v[k], pre_f += vf[k];
		mask[k] = 0, dep[k] = depf[k] = 0, ctg[k] = c;
		if (i >= n) continue;
		if (cbase) while (c + 1 < P.n_contigs && w0 + i >= P.off[c + 1]) { ++c; cb = cbase[c], cbf = cbase_f[c]; }
		dep[k] = (int)(pre - cb), depf[k] = (int)(pre_f - cbf), ctg[k] = c;
		if (i < start) continue;
		const int64_t g = w0 + i;
		const PileBase b = pile_load(P, g, dep[k]), f = pile_load(F, g, depf[k]);
		if (MODE == 0) {
			int32_t *o = o_counts + (i - start);
			o[0] = b.depth, o[(int64_t)MNC_PILE_FWD * m] = f.depth;
			for (int ch = 0; ch < PILE_ALT; ++ch) o[(int64_t)(ch + 1) * m] = b.cnt[ch], o[(int64_t)(MNC_PILE_FWD + ch + 1) * m] = f.cnt[ch];
			o[(int64_t)MNC_PILE_LOWQ * m] = lowq[g], o[(int64_t)MNC_PILE_LOWQ_FWD * m] = lowq[P.n_words + g];
		} else mask[k] = strand_calls(b, f, pile_calls(b, thr), sthr), n_call += __popc((unsigned)mask[k]);
	}
	if (MODE == 0) return;
	int inc_n = n_call;
	for (int d = 1; d < 64; d <<= 1) {
		const int o = __shfl_up(inc_n, d);
		if (lane >= d) inc_n += o;
	}
	if (lane == 63) s_n[wave] = inc_n;
	__syncthreads();
	if (MODE == 1) {
		if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (int64_t)s_n[0] + s_n[1] + s_n[2] + s_n[3];
		return;
	}
	int64_t at = tile_voff[blockIdx.x] + inc_n - n_call;
	for (int w = 0; w < wave; ++w) at += s_n[w];
	for (int k = 0; k < SC_ITEMS; ++k) {
		if (!mask[k]) continue;
		const int64_t g = w0 + base + k;
		const PileBase b = pile_load(P, g, dep[k]), f = pile_load(F, g, depf[k]);
		for (int a = 0; a < 6; ++a) {
			if (!(mask[k] >> a & 1)) continue;
			if (at < var_cap) {
				mnc_variant_strand_t r;
				r.rid = ctg[k], r.pos = (int32_t)(g - P.off[ctg[k]]), r.span = b.span(), r.count = b.allele(a);
				r.ref = (uint8_t)"ACGT"[b.ref], r.alt = (uint8_t)"ACGT-+"[a], r.pad[0] = r.pad[1] = 0;
				r.count_fwd = f.allele(a), r.span_fwd = f.span();
				o_var[at] = r;
			}
			++at;
		}
	}
}

static int strands_need(const mnc_pileup *pu)
{
	if (pu->strands_on) return MNC_OK;
	set_error("the pileup has no strand store (mnc_pileup_store_strands was not called)");
	return MNC_ERR_ARG;
}

// the tile sums of both tracks over the words [w0, w0 + n)
static void strand_tile_sums(mnc_pileup *pu, int64_t w0, int64_t n, bool all)
{
	pile_tile_sums(pu, w0, n, all);
	cov_tile_sums(pu->track_f + w0, n, pu->tile_sums_f, pu->d_off, pu->n_contigs, all ? pu->cbase_f : nullptr, pu->st);
}

template <int MODE>
static void strand_launch(mnc_pileup *pu, int64_t w0, int64_t n, bool all, int rid, int64_t start, PileThr thr, StrandThr sthr, int32_t *o_counts,
                          mnc_variant_strand_t *o_var, int64_t var_cap)
{
	const int32_t *lq = pu->lowq_view();
	const PileView P{pu->track, pu->alt, pu->n_words, pu->didx->seq4, pu->d_off, pu->n_contigs, lq};
	const PileView F{pu->track_f, pu->alt_f, pu->n_words, pu->didx->seq4, pu->d_off, pu->n_contigs, lq ? lq + pu->n_words : nullptr};
	hipLaunchKernelGGL(mnc_pile_scan_strands<MODE>, dim3((unsigned)((n + SC_TILE - 1) / SC_TILE)), dim3(SC_THREADS), 0, pu->st, P, F, w0, n, pu->tile_sums, pu->tile_sums_f,
	                   all ? pu->cbase : nullptr, all ? pu->cbase_f : nullptr, rid, start, thr, sthr, pu->lowq, o_counts, pu->tile_cnt, pu->tile_voff, o_var, var_cap);
}

} // namespace mnc

// ---------------------------------------------------------------- C-ABI: the strand store
extern "C" int mnc_pileup_store_strands(mnc_pileup *pu, int32_t min_qual)
{
	if (!pu) return MNC_ERR_ARG;
	if (min_qual < 0 || min_qual > 93) { set_error("min_qual %d (0 .. 93: a Phred of a Phred+33 character)", min_qual); return MNC_ERR_ARG; }
	HIP_TRY(hipSetDevice(pu->device));
	std::lock_guard<std::mutex> lk(pu->mu);
	if (pu->strands_on || pu->added) { set_error("mnc_pileup_store_strands comes once, before the first add"); return MNC_ERR_ARG; }
	const size_t nw = (size_t)pu->n_words, nc = (size_t)pu->n_contigs, nt = nw / SC_TILE + 2;
	const size_t n_bufs = pu->bufs.size();
	const int64_t bytes0 = pu->bytes;
	hipError_t he = hipSuccess;
	pu->alloc(he, (void**)&pu->track_f, nw * 4);
	pu->alloc(he, (void**)&pu->alt_f, nw * 4 * PILE_ALT);
	pu->alloc(he, (void**)&pu->lowq, nw * 4 * 2);
	pu->alloc(he, (void**)&pu->cbase_f, nc * 8);
	pu->alloc(he, (void**)&pu->tile_sums_f, nt * 8);
	if (he == hipSuccess) he = strands_clear(pu);
	if (he == hipSuccess) he = pu->own_done();                   // an add comes behind the clearing
	if (he != hipSuccess) {
		set_error("strand store of a pileup of %lld bases (40 more bytes each, 72 in all): %s", (long long)pu->n_words, hipGetErrorString(he));
		(void)hipStreamSynchronize(pu->st);
		while (pu->bufs.size() > n_bufs) { (void)hipFree(pu->bufs.back()); pu->bufs.pop_back(); }
		pu->bytes = bytes0, pu->track_f = pu->alt_f = pu->lowq = nullptr, pu->cbase_f = nullptr, pu->tile_sums_f = nullptr;
		return Accum::failed(he);
	}
	pu->min_qual = min_qual, pu->strands_on = true;
	return MNC_OK;
}

extern "C" int mnc_pileup_strands_device(mnc_pileup *pu, const int32_t **d_track_fwd, const int32_t **d_alt_fwd, const int32_t **d_lowq)
{
	if (!pu) return MNC_ERR_ARG;
	if (int rc = strands_need(pu)) return rc;
	if (d_track_fwd) *d_track_fwd = pu->n_words ? pu->track_f : nullptr;
	if (d_alt_fwd) *d_alt_fwd = pu->n_words ? pu->alt_f : nullptr;
	if (d_lowq) *d_lowq = pu->n_words ? pu->lowq : nullptr;
	return MNC_OK;
}

extern "C" int mnc_pileup_fetch_strand_counts(mnc_pileup *pu, int rid, int64_t start, int64_t end, int32_t *out)
{
	if (!pu) return MNC_ERR_ARG;
	if (int rc = strands_need(pu)) return rc;
	if (int rc = accum_interval(pu->off, rid, start, end)) return rc;
	if (end == start) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(pu->device));
	const size_t bytes = (size_t)(end - start) * 4 * MNC_PILE_STRAND_PLANES;
	int32_t *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, bytes));
	strand_tile_sums(pu, pu->off[rid], end, false);             // the contig's words up to `end`: the sums start at the contig
	strand_launch<0>(pu, pu->off[rid], end, false, rid, start, PileThr{0, 0, 0}, StrandThr{0, 0}, tmp, nullptr, 0);
	return pu->finish(hipSuccess, tmp, {out, tmp, bytes}, {}, "pileup counts by strand");
}

extern "C" int mnc_pileup_call_variants_strands(mnc_pileup *pu, int rid, int32_t min_depth, int32_t min_count, int32_t min_permille, int32_t min_strand_count,
                                                int32_t min_strand_permille, mnc_variant_strand_t *out, int64_t cap, int64_t *n)
{
	if (!pu || !n) return MNC_ERR_ARG;
	*n = 0;
	if (int rc = strands_need(pu)) return rc;
	if (rid < -1 || rid >= pu->n_contigs) { set_error("contig %d out of range", rid); return MNC_ERR_ARG; }
	const bool all = rid < 0;
	const int64_t w0 = all ? 0 : pu->off[rid], len = all ? pu->n_words : pu->off[rid + 1] - w0;
	if (len == 0) return MNC_OK;
	HIP_TRY(hipSetDevice(pu->device));
	const PileThr thr{min_depth, min_count, min_permille};
	const StrandThr sthr{min_strand_count, min_strand_permille};
	const int64_t nb = (len + SC_TILE - 1) / SC_TILE;
	// ---- count, scan
	strand_tile_sums(pu, w0, len, all);
	strand_launch<1>(pu, w0, len, all, rid, 0, thr, sthr, nullptr, nullptr, 0);
	exclusive_scan(ScanInPlain<int64_t>{pu->tile_cnt}, nb, pu->tile_voff, pu->sums2, pu->st);
	HIP_TRY(hipGetLastError());
	int64_t total = 0;
	HIP_TRY(hipMemcpyAsync(&total, pu->tile_voff + nb, 8, hipMemcpyDeviceToHost, pu->st));
	HIP_TRY(hipStreamSynchronize(pu->st));
	*n = total;
	if (cap < total) { set_error("%lld variants, room for %lld", (long long)total, (long long)cap); return MNC_ERR_RANGE; }
	if (total == 0) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	// ---- write (as mnc_pileup_call_variants: no tile writes beyond `total`)
	mnc_variant_strand_t *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, (size_t)total * sizeof(mnc_variant_strand_t)));
	strand_launch<2>(pu, w0, len, all, rid, 0, thr, sthr, nullptr, tmp, total);
	return pu->finish(hipSuccess, tmp, {out, tmp, (size_t)total * sizeof(mnc_variant_strand_t)}, {}, "pileup variants by strand");
}
