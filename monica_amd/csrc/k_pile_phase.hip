// Phased pileup (include/monica_amd.h, "phased pileup"): the columns of every selected record go to the planes of the
// haplotype the record was decided for in the phase block the column lies in -- two or three ordinary mnc_pileup accumulators
// (haplotype 0, haplotype 1 and, where the caller wants it, the rest), so that every read-out of a pileup serves a haplotype
// as it stands.  Haplotag's vote fused with the pileup's column walk; the seventh consumer of a batch as it stands in HBM.
// Runs only when asked for.
//
//   mnc_pile_phase_add   one wave per READ, four reads per workgroup, no workgroup barrier.  Per selected record two passes:
//   pass A, the vote     linkage.h's walk with the lanes holding SITES and haplotag's segments (hap_segment): where
//                        mnc_hap_add issues atomics on its block table, the owner lane of a closing segment writes the
//                        decision -- 0 none, 1 haplotype 0, 2 haplotype 1 -- as one byte into the wave's own slice of LDS,
//                        at block - the window's first block.  A record without a site under it has no pass A: all it has
//                        goes to the rest.
//   the window           A slice holds the decisions of PHASE_W consecutive blocks.  A record with more blocks under it
//                        runs both passes once per window; a pass B tallies only the columns its window OWNS -- those whose
//                        block lies in it; columns in no block belong to the first.  Rare: blocks are long where reads overlap.
//   pass B, the columns  pile_add_read's walk with the lanes holding CIGAR operations, then columns.  The block of a column:
//                        a wave-uniform cursor `cur` into the contig's sites never passes the chunk's lowest position; the
//                        lanes load the 64 positions from it on (one coalesced load, a second where the cursor moved), a
//                        column finds its rank among them by bisecting through cross-lane reads, and only a column with
//                        all 64 below it searches the list itself.  pos[i], block[i] and block[i - 1] then decide by the
//                        contract's rule; the decision is one LDS byte.  An I column asks for its anchor, p - 1.
//   the depth runs       at COLUMN granularity, since a run of M columns must end and restart wherever the destination
//                        changes: every column carries e = its destination if it is an M column that this pass tallies, else
//                        -1, and compares it with the e of the nearest reference-consuming column below (one ballot, one
//                        cross-lane read; the last one's e crosses the 64-column and 64-operation borders as a wave-uniform
//                        scalar).  Where they differ the column closes the run of the one (-1 at its own position) and opens
//                        that of the other (+1): the plain pileup's two atomics per run, plus two per change of destination.
// What a destination receives is what mnc_pile_add would have given it for those columns alone: a reference match costs no
// atomic, the contig-end rule is cov_put's.  Integer arithmetic throughout; no host wait.
#include <hip/hip_runtime.h>
#include <climits>
#include "linkage.h"

using namespace mnc;

namespace mnc {

constexpr int PHASE_W = 256;                    // blocks per window: a byte each, one 32-bit word per lane to clear
static_assert(PHASE_W == 64 * 4 && PHASE_W <= 1024, "a lane clears one word of its wave's slice");
constexpr int PH_REST = 2;                      // destinations: 0, 1 the haplotypes

struct PhasePlanes {
	int32_t *track0, *track1, *track2;         // hap0, hap1, rest (nullptr: what would go there is dropped)
	int32_t *alt0, *alt1, *alt2;
	int64_t n_words;
	__device__ __forceinline__ int32_t *track(int d) const { return d == 0 ? track0 : d == 1 ? track1 : track2; }
	__device__ __forceinline__ int32_t *alt(int d) const { return d == 0 ? alt0 : d == 1 ? alt1 : alt2; }
};

// LDS writes of some lanes of a wave before reads of others of the same wave
__device__ __forceinline__ void phase_wave_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	__builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256) void mnc_pile_phase_add(Batch B, int sel, HapView H, PhasePlanes P)
{
	__shared__ uint32_t s_dec[4][PHASE_W / 4];
	const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
	const uint32_t rd = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (rd >= B.n_reads) return;                              // (whole waves; the kernel has no workgroup barrier)
	const int64_t read_off = B.offsets[rd];
	const int qlen = (int)(B.offsets[rd + 1] - read_off);
	if (qlen <= 0) return;
	const uint8_t *read = B.bases + read_off;
	const LinkSites &L = H.list;
	uint8_t *dec = (uint8_t*)s_dec[wave];
	cov_for_records(B, rd, sel, L.n_contigs, [&](const mnc_reg_t &r, int64_t slot) {
		const int n_c = r.n_cigar;
		if (n_c <= 0) return;
		const int s_c0 = L.first[r.rid], s_end = L.first[r.rid + 1];   // the contig's sites
		const int s_lo = link_lower(L.pos, s_c0, s_end, r.rs);
		const int s_hi = link_lower(L.pos, s_lo, s_end, r.re);
		const bool sites = s_lo < s_hi;                           // (wave-uniform, like all of the above)
		if (!sites && !P.track2) return;                          // all of it would go to a rest that is not there
		const int64_t coff = L.off[r.rid], len = L.off[r.rid + 1] - coff;
		const uint32_t *src = B.cig_reg + B.regdp[slot].cig_off;
		auto Q = [&](int p) -> int {                              // column p of the query side, on the hit's strand (pile_add_read)
			int at = r.rev ? r.qe - 1 - p : r.qs + p;
			at = at < 0 ? 0 : at >= qlen ? qlen - 1 : at;
			const int c = base_nt4(read[at]);
			return r.rev ? (c < 4 ? 3 - c : 4) : c;
		};
		const int b_first = sites ? H.block[s_lo] : 0;
		const int n_win = sites ? (H.block[s_hi - 1] - b_first) / PHASE_W + 1 : 1;
		for (int win = 0; win < n_win; ++win) {
			const int wb = b_first + win * PHASE_W;                  // the window's first block
			// ---- pass A: this record's decisions in the blocks [wb, wb + PHASE_W)
			if (sites) {
				phase_wave_sync();                                    // (the window before has been read)
				s_dec[wave][lane] = 0u;
				phase_wave_sync();
				int cb = -1, cn0 = 0, cn1 = 0;                        // the open block carried over the last 64 sites' border
				link_walk_record(B, r, slot, read, qlen, L, s_lo, s_hi, [&](int c0, int s, bool valid, int stmt) {
					const HapSeg g = hap_segment(H.block, H.phase, c0, s, valid, stmt, s_hi, cb, cn0, cn1);
					if (g.closes && hap_decided(g.n0, g.n1, H.min_votes, H.min_permille) && g.b >= wb && g.b - wb < PHASE_W)
						dec[g.b - wb] = (uint8_t)(1 + (int)(g.n1 > g.n0));
				});
				phase_wave_sync();
			}
			// ---- pass B: the columns this window owns
			int64_t toff = r.rs;                                   // reference position before the chunk at hand
			int qoff = 0;                                          // query columns before it
			int prev_e = -1;                                       // e of the last reference-consuming column so far (wave-uniform)
			int cur = s_lo;                                        // no site below it lies at or above a position still to come
			for (int k0 = 0; k0 < n_c; k0 += 64) {
				const int k = k0 + lane;
				const uint32_t wd = k < n_c ? src[k] : 0u;
				const int op = (int)(wd & 0xfu);
				const int l = k < n_c && op <= 2 ? (int)(wd >> 4) : 0;
				const int dt = op != 1 ? l : 0, dq = op != 2 ? l : 0;
				const int cols = op == 1 ? (l > 0) : l;              // an insertion is one column: its bases are not looked at
				const int it = cov_incl_add(dt), iq = cov_incl_add(dq), ie = cov_incl_add(cols);
				const int my_t0 = it - dt, my_q0 = qoff + iq - dq;
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
					const bool is_I = o_op == 1;
					const bool live = valid && (!is_I || p > r.rs);      // an I counts with a reference column of this record on its left
					const int lp = (int)(p - (is_I ? 1 : 0));            // the position that decides where the column goes
					// ---- the column's block (-1: none), its window, its destination
					int blk = -1, d = PH_REST;
					if (sites) {                                        // (wave-uniform: every lane is in the cross-lane reads below)
						const int lp0 = __shfl(lp, 0);                    // the chunk's lowest: positions ascend along the columns
						int sp;                                           // pos[cur + lane], INT_MAX behind the contig's sites
						for (;;) {
							sp = cur + lane < s_end ? L.pos[cur + lane] : INT_MAX;
							const int adv = __popcll(__ballot(sp < lp0));
							if (adv == 0) break;
							cur += adv;
						}
						int rank = 0;                                     // of the 64 positions, those below lp
						for (int step = 32; step > 0; step >>= 1) {
							const int v = __shfl(sp, rank + step - 1);
							if (v < lp) rank += step;
						}
						const int v63 = __shfl(sp, 63);
						if (rank == 63 && v63 < lp) rank = 64;
						const int sp_i = __shfl(sp, rank & 63);
						const int i = rank < 64 ? cur + rank : link_lower(L.pos, min(cur + 64, s_end), s_end, lp);
						if (i < s_end) {
							const int pos_i = rank < 64 ? sp_i : L.pos[i], bi = H.block[i];
							if (pos_i == lp || (i > s_c0 && H.block[i - 1] == bi)) blk = bi;
						}
					}
					const bool mine = blk < 0 ? win == 0 : blk >= wb && blk - wb < PHASE_W;
					if (mine && blk >= 0) {
						const int dc = (int)dec[blk - wb];
						d = dc ? dc - 1 : PH_REST;
					}
					const bool go = live && mine && P.track(d) != nullptr;
					// ---- depth: the runs of M columns of one destination
					const bool is_ref = valid && !is_I;
					const int e = go && o_op == 0 ? d : -1;
					const unsigned long long m_ref = __ballot(is_ref);
					const unsigned long long below = m_ref & ((1ull << lane) - 1ull);
					const int e_below = __shfl(e, below ? 63 - __clzll((long long)below) : 0);
					const int pe = below ? e_below : prev_e;
					if (is_ref && pe != e) {
						if (pe >= 0) cov_put(P.track(pe) + coff, len, p, -1);
						if (e >= 0) cov_put(P.track(e) + coff, len, p, 1);
					}
					if (m_ref) prev_e = __shfl(e, 63 - __clzll((long long)m_ref));
					// ---- the column's own observation
					if (go) {
						int32_t *a = P.alt(d) + coff;                     // channel ch of base p: a[ch * n_words + p]
						if (o_op == 0) {
							if (p >= 0 && p < len) {
								const int qc = Q(q0 + x), tc = pile_ref(B.seq4, coff + p);
								if (tc == 4 || qc != tc) pile_put(a + (int64_t)qc * P.n_words, len, p);
							}
						} else if (o_op == 2) pile_put(a + (int64_t)CH_DEL * P.n_words, len, p);
						else pile_put(a + (int64_t)CH_INS * P.n_words, len, p - 1);
					}
				}
				toff += __shfl(it, 63), qoff += __shfl(iq, 63);
			}
			if (prev_e >= 0 && lane == 0) cov_put(P.track(prev_e) + coff, len, toff, -1);
		}
	});
}

// ---------------------------------------------------------------- the engine's side (mnc_engine_add_pileup_phased, engine.hip)
// MNC_ERR_ARG, before anything is touched: two of the pileups are one object, or one of them keeps a store
int pile_phase_check(const mnc_pileup *hap0, const mnc_pileup *hap1, const mnc_pileup *rest)
{
	if (hap0 == hap1 || (rest && (rest == hap0 || rest == hap1))) { set_error("two of the phased pileup's accumulators are the same object"); return MNC_ERR_ARG; }
	for (const mnc_pileup *pu : {hap0, hap1, rest})
		if (pu && (pu->ins_on || pu->strands_on)) {
			set_error("a pileup with the %s store cannot take a phased add: the allele table and the strand planes by haplotype are a later addition",
			          pu->ins_on ? "insertion" : "strand");
			return MNC_ERR_ARG;
		}
	return MNC_OK;
}

// the batch B, as it stands in HBM, on the engine's stream `st`: one launch, ordered against all the accumulators
int pile_phase_add(const mnc_haplotag *ht, mnc_pileup *hap0, mnc_pileup *hap1, mnc_pileup *rest, const Batch &B, int sel, hipStream_t st)
{
	if (B.n_reads == 0 || hap0->n_words == 0) return MNC_OK;
	const PhasePlanes P{hap0->track, hap1->track, rest ? rest->track : nullptr, hap0->alt, hap1->alt, rest ? rest->alt : nullptr, hap0->n_words};
	const HapView H = haplotag_view(ht);
	Accum *set[3] = {hap0, hap1, rest};
	return accum_add_set(set, 3, st, [&] {
		hap0->added = hap1->added = true;
		if (rest) rest->added = true;
		hipLaunchKernelGGL(mnc_pile_phase_add, dim3((B.n_reads + 3) / 4), dim3(256), 0, st, B, sel, H, P);
	});
}

} // namespace mnc
