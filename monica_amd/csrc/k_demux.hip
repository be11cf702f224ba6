// Demultiplexing (include/monica_amd.h, "demux"): which sample a read is from.  A barcoded run puts several samples on one
// flow cell; a read carries its sample's barcode at the front and, with ligation kits, the reverse complement at the rear.
// An mnc_demux searches every barcode in the first and the last `window` bases of every read, approximately, decides the
// read's barcode, writes a tag per read and counts reads -- and, per barcode, what mnc_counts counts per genome.  An
// accumulator of accum.h, the first that looks at the read's own ends instead of what it aligned to: no region walk.
//
//   the search       d(p, t) = the smallest unit-cost edit distance of the whole pattern to any substring of the text (the
//                    last-row minimum of the DP with first row 0 and first column i), e = the first text index where it is
//                    attained, -1 when no column beats the empty substring's |p|.  Myers' bit-vector algorithm in Hyyrö's
//                    form: the DP column as two words of vertical differences Pv / Mv, one step per text base, the score
//                    followed at bit |p| - 1 of the lane's OWN pattern (the bits above it hold garbage that never comes down:
//                    carries and shifts only go up).
//   mnc_demux_search PERSISTENT workgroups of four waves, DEMUX_WG_PER_CU per CU; a wave takes reads in a strided loop, one
//                    wave per READ, no workgroup barrier inside the loop.  The lanes hold SEARCH SLOTS: slot s = end *
//                    n_barcodes + barcode, 64 a pass.  A lane keeps its pattern's four match masks, Pv, Mv, the score and
//                    the running (min, first index) in registers; the mask of a step is chosen by the bits of the text's
//                    code -- three one-bit extracts and four three-input bit operations, no compare, no branch (see `step`);
//                    no indexed register array, no scratch.
//     LDS            the wave first stages both texts into its slice as codes 0 .. 3, 4 = matches nothing: the front text
//                    as it stands, the rear text reversed and complemented, so one pattern serves both ends.  2 * W bytes a
//                    wave (W rounded up to 4), at most 8 KiB a workgroup at MNC_DEMUX_MAX_WINDOW beside 1 032 bytes of
//                    counts: 17 workgroups would fit the 160 KiB of a CU, the wave slots hold 8 -- LDS never limits the
//                    occupancy.  The search reads a 32-bit word of four codes per four steps; the lanes of one end read the
//                    same word (a broadcast), a pass that straddles the two ends reads two.
//     WORD           uint32_t when every pattern is <= 32 bases (a kit's 24-mers): half the integer work of uint64_t, whose
//                    (Eq & Pv) + Pv is an add with carry.  The host chooses by the longest pattern.
//     the decision   a lane folds each slot's key into the (smallest, second smallest) of the slot's end: four registers.
//                    The key is d << 19 | barcode << 11 | e + 1: ordered by distance, then barcode -- the lower index wins a
//                    tie -- and the cut length rides along instead of being looked up again (the one change against a plain
//                    d << 16 | barcode).  Per end one butterfly gives the best key, a second one the runner-up: every lane
//                    offers its second where its smallest IS the best, its smallest otherwise.  Lane 0 decides and writes
//                    the 8-byte tag as one store.
//     the counts     reads[] is a private uint32 array per workgroup in LDS, flushed at its end with one 64-bit atomic per
//                    NON-ZERO entry (k_lca.hip's direct[]).
//   mnc_demux_taxa   one thread per read: taxa[row][genome][3] += {1, the read's length, its mlen} with 64-bit atomics, from
//                    the batch's assign / best_mlen as they stand in HBM and the tag just written; mnc_count_taxa's shape,
//                    its LDS bins included.
// Integer arithmetic throughout; no host wait in an add.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <new>
#include <type_traits>
#include <vector>
#include "accum.h"
#include "device.h"

using namespace mnc;

constexpr int DEMUX_WG_PER_CU = 8;             // 32 waves a CU: every wave slot (both instantiations stay below 64 VGPRs)
constexpr int DEMUX_THREADS = 256, DEMUX_WAVES = DEMUX_THREADS / 64;
constexpr int64_t DEMUX_MAX_READS = (1LL << 31) - 1;
constexpr uint32_t DEMUX_NO_KEY = ~0u;

struct mnc_demux : mnc::Accum {
	int n_barcodes = 0, window = 0, max_dist = 0, min_margin = 0, ends = 0, max_len = 0, G = 0, n_cu = 1;
	bool wide = false;                         // test switch: the 64-bit instantiation whatever the patterns (mnc_demux_set_word_bits)
	int64_t cap_reads = 0;
	uint64_t *peq = nullptr;                   // [n_barcodes][4] match masks: bit i of peq[b][c] = (base i of barcode b has code c)
	int32_t *plen = nullptr;                   // [n_barcodes]
	unsigned long long *reads = nullptr;       // [n_barcodes + 2]
	unsigned long long *taxa = nullptr;        // [n_barcodes + 1][G][3], with an index
	mnc_demux_tag_t *tags = nullptr;           // [cap_reads]
	// mnc_demux_add's copy of a host batch
	uint8_t *in_bases = nullptr;
	int64_t *in_offsets = nullptr;
	size_t in_bases_cap = 0, in_offsets_cap = 0;
};

namespace mnc {

struct DemuxView {
	const uint8_t *bases;
	const int64_t *offsets;
	int64_t n_reads;
	const uint64_t *peq;
	const int32_t *plen;
	int n_barcodes, window, max_dist, min_margin, ends;
	mnc_demux_tag_t *tags;
	unsigned long long *reads;
};

__device__ __forceinline__ uint32_t demux_wave_min(uint32_t x)
{
	for (int d = 32; d > 0; d >>= 1) {
		const uint32_t o = __shfl_xor(x, d);
		x = o < x ? o : x;
	}
	return x;
}

// base_nt4 (device.h) without a branch: bits 1 and 2 of the letter number A C G T/U as 0 1 3 2, and the five letters are one
// 32-bit set over 'a' .. 'z'
__device__ __forceinline__ int demux_nt4(uint8_t ch)
{
	const uint32_t at = (uint32_t)(ch | 0x20) - 'a', x = ch >> 1 & 3;
	const bool known = at < 26u && (0x180045u >> (at & 31) & 1u);   // a c g t u
	return known ? (int)(x ^ x >> 1) : 4;
}

// one end's verdict from its two smallest keys (wave-uniform)
struct DemuxEnd { bool hit; int barcode, d, cut; };
__device__ __forceinline__ DemuxEnd demux_end(uint32_t best, uint32_t second, int max_dist, int min_margin)
{
	DemuxEnd x;
	x.d = (int)(best >> 19), x.barcode = (int)(best >> 11 & 0xff), x.cut = (int)(best & 0x7ff);
	x.hit = x.d <= max_dist && (second == DEMUX_NO_KEY || (int)(second >> 19) - x.d >= min_margin);
	return x;
}

template <class WORD>
__global__ __launch_bounds__(DEMUX_THREADS) void mnc_demux_search(DemuxView V)
{
	extern __shared__ __align__(16) uint8_t dm_smem[];         // [DEMUX_WAVES][2][wp] text codes
	__shared__ uint32_t s_reads[MNC_DEMUX_MAX_BARCODES + 2];
	for (int k = threadIdx.x; k < V.n_barcodes + 2; k += DEMUX_THREADS) s_reads[k] = 0;
	__syncthreads();
	const int lane = lane_id(), wave = threadIdx.x >> 6;
	const int wp = (V.window + 3) & ~3;
	uint8_t *text = dm_smem + (size_t)wave * 2 * wp;           // front at 0, rear at wp
	const int n_ends = V.ends == MNC_DEMUX_FRONT ? 1 : 2, n_slots = n_ends * V.n_barcodes;
	const int64_t stride = (int64_t)gridDim.x * DEMUX_WAVES;
	for (int64_t r = (int64_t)blockIdx.x * DEMUX_WAVES + wave; r < V.n_reads; r += stride) {   // (whole waves; no barrier inside)
		const int64_t o0 = V.offsets[r], len = V.offsets[r + 1] - o0;
		const int tl = (int)(len < V.window ? (len < 0 ? 0 : len) : V.window);
		// ---- stage: the first tl bases, and the last tl reversed and complemented; the tail of the last word matches nothing
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");     // the last read's search is over
		for (int i = lane; i < ((tl + 3) & ~3); i += 64) {
			int f = 4, b = 4;
			if (i < tl) {
				f = demux_nt4(V.bases[o0 + i]);
				b = demux_nt4(V.bases[o0 + len - 1 - i]);
				b = b < 4 ? 3 - b : 4;
			}
			text[i] = (uint8_t)f;
			if (n_ends == 2) text[wp + i] = (uint8_t)b;
		}
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		__builtin_amdgcn_wave_barrier();
		// ---- search: 64 slots a pass
		uint32_t f1 = DEMUX_NO_KEY, f2 = DEMUX_NO_KEY, r1 = DEMUX_NO_KEY, r2 = DEMUX_NO_KEY;
		for (int base = 0; base < n_slots; base += 64) {
			const int s = base + lane;
			const bool live = s < n_slots;
			const int end = live && s >= V.n_barcodes ? 1 : 0, bc = live ? s - end * V.n_barcodes : 0;
			const uint64_t *q = V.peq + (size_t)bc * 4;
			using SW = typename std::make_signed<WORD>::type;
			const WORD p0 = (WORD)q[0], p2 = (WORD)q[2], x01 = p0 ^ (WORD)q[1], x23 = p2 ^ (WORD)q[3];
			const int m = V.plen[bc];
			const WORD top = (WORD)1 << (m - 1);
			const uint32_t *t32 = reinterpret_cast<const uint32_t*>(text + end * wp);
			WORD Pv = ~(WORD)0, Mv = 0;
			int score = m, best = m, at = -1;
			// c: the text's code in its low three bits.  The mask is chosen by bit 0 inside each pair, by bit 1 between the
			// pairs, and bit 2 ("matches nothing") clears it: three sign-extending one-bit extracts and four three-input bit
			// operations.  (Written as c == 0 ? p0 : .. the compiler built a tree of exec-mask branches around every step.)
			auto step = [&](uint32_t c, int j) {
				const WORD s0 = (WORD)(SW)((int32_t)(c << 31) >> 31), s1 = (WORD)(SW)((int32_t)(c << 30) >> 31), s2 = (WORD)(SW)((int32_t)(c << 29) >> 31);
				const WORD lo = p0 ^ (x01 & s0), hi = p2 ^ (x23 & s0);
				const WORD Eq = (lo ^ ((lo ^ hi) & s1)) & ~s2;
				const WORD Xv = Eq | Mv;
				const WORD Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
				WORD Ph = Mv | ~(Xh | Pv);
				WORD Mh = Pv & Xh;
				score += (Ph & top) ? 1 : 0;
				score -= (Mh & top) ? 1 : 0;
				Ph <<= 1, Mh <<= 1;                                // (the first row is 0: nothing comes in at bit 0)
				Pv = Mh | ~(Xv | Ph);
				Mv = Ph & Xv;
				if (score < best) best = score, at = j;
			};
			int j = 0;
			for (; j + 4 <= tl; j += 4) {
				const uint32_t w = t32[j >> 2];
				step(w, j), step(w >> 8, j + 1), step(w >> 16, j + 2), step(w >> 24, j + 3);
			}
			if (j < tl) {
				uint32_t w = t32[j >> 2];
				for (; j < tl; ++j, w >>= 8) step(w, j);
			}
			if (live) {
				const uint32_t k = (uint32_t)best << 19 | (uint32_t)bc << 11 | (uint32_t)(at + 1);
				uint32_t k1 = end ? r1 : f1, k2 = end ? r2 : f2;
				if (k < k1) k2 = k1, k1 = k;
				else if (k < k2) k2 = k;
				if (end) r1 = k1, r2 = k2; else f1 = k1, f2 = k2;
			}
		}
		// ---- decide
		const uint32_t fb = demux_wave_min(f1), fs = demux_wave_min(f1 == fb ? f2 : f1);
		const DemuxEnd F = demux_end(fb, fs, V.max_dist, V.min_margin);
		DemuxEnd R{false, -1, 255, 0};
		if (n_ends == 2) {
			const uint32_t rb = demux_wave_min(r1), rs = demux_wave_min(r1 == rb ? r2 : r1);
			R = demux_end(rb, rs, V.max_dist, V.min_margin);
		}
		int barcode = -1;
		if (V.ends == MNC_DEMUX_FRONT) barcode = F.hit ? F.barcode : -1;
		else if (V.ends == MNC_DEMUX_BOTH) barcode = F.hit && R.hit && F.barcode == R.barcode ? F.barcode : -1;
		else if (F.hit && R.hit) barcode = F.barcode == R.barcode ? F.barcode : -2;
		else barcode = F.hit ? F.barcode : R.hit ? R.barcode : -1;
		if (lane == 0) {
			const uint32_t cut_f = barcode >= 0 && F.hit && F.barcode == barcode ? (uint32_t)F.cut : 0u;
			const uint32_t cut_r = barcode >= 0 && R.hit && R.barcode == barcode ? (uint32_t)R.cut : 0u;
			uint2 word;
			word.x = (uint32_t)(uint16_t)(int16_t)barcode | (uint32_t)F.d << 16 | (uint32_t)R.d << 24;
			word.y = cut_f | cut_r << 16;
			*reinterpret_cast<uint2*>(V.tags + r) = word;
			atomicAdd(&s_reads[barcode >= 0 ? barcode : V.n_barcodes - 1 - barcode], 1u);   // -1: none, -2: conflict
		}
	}
	__syncthreads();
	for (int k = threadIdx.x; k < V.n_barcodes + 2; k += DEMUX_THREADS)
		if (s_reads[k]) (void)__hip_atomic_fetch_add(V.reads + k, (unsigned long long)s_reads[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// per barcode what mnc_count_taxa (k_post.hip) counts per genome; the reads without a barcode, a conflict among them, in the last row
// As there: a sample of few barcodes and taxa would put every read's three atomics on the same few HBM words (measured: 0.6 ms
// of a 100 000-read add), so a block of DT_READS reads adds up in LDS while the table fits DT_LDS_BINS words -- 96 barcodes of
// 20 genomes do -- and flushes the bins it touched; a larger table is added to directly, where the reads spread by themselves.
constexpr int DT_THREADS = 256, DT_READS = 2048, DT_LDS_BINS = 6144;   // 48 KiB

__global__ __launch_bounds__(DT_THREADS) void mnc_demux_taxa(Batch B, const mnc_demux_tag_t *tags, int n_barcodes, int n_genomes, unsigned long long *taxa)
{
	__shared__ unsigned long long s_bins[DT_LDS_BINS];
	const int64_t n_bins = (int64_t)(n_barcodes + 1) * n_genomes * 3;
	const bool in_lds = n_bins <= DT_LDS_BINS;
	if (in_lds) {
		for (int k = threadIdx.x; k < (int)n_bins; k += DT_THREADS) s_bins[k] = 0;
		__syncthreads();
	}
	unsigned long long *bins = in_lds ? s_bins : taxa;
	const uint32_t lo = blockIdx.x * DT_READS, hi = min(B.n_reads, lo + DT_READS);
	for (uint32_t rd = lo + threadIdx.x; rd < hi; rd += DT_THREADS) {
		const int a = B.assign[rd];
		if (a < 0) continue;
		const int g = B.contig_genome[a], bc = tags[rd].barcode;
		if (g < 0 || g >= n_genomes) continue;
		unsigned long long *row = bins + ((size_t)(bc >= 0 ? bc : n_barcodes) * n_genomes + g) * 3;
		atomicAdd(row + 0, 1ULL);
		atomicAdd(row + 1, (unsigned long long)(B.offsets[rd + 1] - B.offsets[rd]));
		atomicAdd(row + 2, (unsigned long long)B.best_mlen[rd]);
	}
	if (in_lds) {
		__syncthreads();
		for (int k = threadIdx.x; k < (int)n_bins; k += DT_THREADS)
			if (s_bins[k]) atomicAdd(taxa + k, s_bins[k]);
	}
}

// a read without an add: no barcode, neither end searched
__global__ __launch_bounds__(256) void mnc_demux_clear(mnc_demux_tag_t *tags, int64_t n)
{
	const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r < n) *reinterpret_cast<uint2*>(tags + r) = make_uint2(0xffffffffu, 0u);
}

// ---------------------------------------------------------------- the engine's side (mnc_engine_add_demux, engine.hip)
const Accum *as_accum(const mnc_demux *dm) { return dm; }

// MNC_ERR_RANGE, before anything is touched, when the batch holds more reads than the tag store
static int demux_fits(const mnc_demux *dm, int64_t n_reads)
{
	if (n_reads <= dm->cap_reads) return MNC_OK;
	set_error("the batch holds %lld reads, the demux accumulator was created for %lld (cap_reads)", (long long)n_reads, (long long)dm->cap_reads);
	return MNC_ERR_RANGE;
}
int demux_fits(const mnc_demux *dm, const Batch &B) { return demux_fits(dm, (int64_t)B.n_reads); }

// n reads of (bases, offsets), device arrays, on `st`: the persistent grid, the instantiation by the longest pattern
static void demux_launch(const mnc_demux *dm, const uint8_t *bases, const int64_t *offsets, int64_t n, hipStream_t st)
{
	const DemuxView V{bases, offsets, n, dm->peq, dm->plen, dm->n_barcodes, dm->window, dm->max_dist, dm->min_margin, dm->ends, dm->tags, dm->reads};
	const unsigned wg = (unsigned)std::max<int64_t>(1, std::min<int64_t>((int64_t)dm->n_cu * DEMUX_WG_PER_CU, (n + DEMUX_WAVES - 1) / DEMUX_WAVES));
	const size_t lds = (size_t)DEMUX_WAVES * 2 * ((dm->window + 3) & ~3);
	if (dm->max_len <= 32 && !dm->wide) hipLaunchKernelGGL(mnc_demux_search<uint32_t>, dim3(wg), dim3(DEMUX_THREADS), lds, st, V);
	else hipLaunchKernelGGL(mnc_demux_search<uint64_t>, dim3(wg), dim3(DEMUX_THREADS), lds, st, V);
}

// the batch B, as it stands in HBM, on the engine's stream `st`; an empty batch is an add of no reads.  taxa only for the
// accumulator of an index (the engine's: add_precheck)
int demux_add(mnc_demux *dm, const Batch &B, hipStream_t st)
{
	return dm->add(st, [&] {
		if (!B.n_reads) return;
		demux_launch(dm, B.bases, B.offsets, B.n_reads, st);
		if (dm->taxa) hipLaunchKernelGGL(mnc_demux_taxa, dim3((B.n_reads + DT_READS - 1) / DT_READS), dim3(DT_THREADS), 0, st, B, dm->tags, dm->n_barcodes, dm->G, dm->taxa);
	});
}

} // namespace mnc

// ---------------------------------------------------------------- the barcodes, on the host
// checked (the message names the barcode and the position), then as match masks
static int demux_patterns(const uint8_t *barcodes, const int64_t *off, int n, std::vector<uint64_t> &peq, std::vector<int32_t> &plen, int &max_len)
{
	if (n < 1 || n > MNC_DEMUX_MAX_BARCODES) { set_error("n_barcodes %d outside 1 .. %d (MNC_DEMUX_MAX_BARCODES)", n, MNC_DEMUX_MAX_BARCODES); return MNC_ERR_ARG; }
	if (!barcodes || !off) { set_error("`%s` is NULL", barcodes ? "bc_offsets" : "barcodes"); return MNC_ERR_ARG; }
	peq.assign((size_t)n * 4, 0), plen.assign((size_t)n, 0), max_len = 0;
	for (int b = 0; b < n; ++b) {
		const int64_t len = off[b + 1] - off[b];
		if (off[b] < 0 || len < 1 || len > MNC_DEMUX_MAX_LEN) {
			set_error("barcode %d: length %lld outside 1 .. %d (MNC_DEMUX_MAX_LEN)", b, (long long)len, MNC_DEMUX_MAX_LEN);
			return MNC_ERR_ARG;
		}
		for (int i = 0; i < (int)len; ++i) {
			int c;
			switch (barcodes[off[b] + i]) {
			case 'A': case 'a': c = 0; break;
			case 'C': case 'c': c = 1; break;
			case 'G': case 'g': c = 2; break;
			case 'T': case 't': case 'U': case 'u': c = 3; break;
			default:
				set_error("barcode %d, position %d: character 0x%02x is none of ACGTU", b, i, barcodes[off[b] + i]);
				return MNC_ERR_ARG;
			}
			peq[(size_t)b * 4 + c] |= 1ULL << i;
		}
		plen[(size_t)b] = (int32_t)len, max_len = std::max(max_len, (int)len);
	}
	return MNC_OK;
}

// ---------------------------------------------------------------- C-ABI
extern "C" void mnc_demux_free(mnc_demux *dm)
{
	if (!dm) return;
	dm->release();
	delete dm;
}

extern "C" int mnc_demux_create(mnc_index *idx, int device, const uint8_t *barcodes, const int64_t *bc_offsets, int32_t n_barcodes, int32_t window,
                                int32_t max_dist, int32_t min_margin, int32_t ends, int64_t cap_reads, mnc_demux **out)
{
	if (!out) return MNC_ERR_ARG;
	*out = nullptr;
	std::vector<uint64_t> peq;
	std::vector<int32_t> plen;
	int max_len = 0;
	try {
		if (int rc = demux_patterns(barcodes, bc_offsets, n_barcodes, peq, plen, max_len)) return rc;
	} catch (const std::bad_alloc &) { return MNC_ERR_NOMEM; }
	if (window < 1 || window > MNC_DEMUX_MAX_WINDOW) { set_error("window %d outside 1 .. %d (MNC_DEMUX_MAX_WINDOW)", window, MNC_DEMUX_MAX_WINDOW); return MNC_ERR_ARG; }
	if (max_dist < 0) { set_error("max_dist %d: max_dist >= 0 is required", max_dist); return MNC_ERR_ARG; }
	if (min_margin < 0) { set_error("min_margin %d: min_margin >= 0 is required", min_margin); return MNC_ERR_ARG; }
	if (ends != MNC_DEMUX_FRONT && ends != MNC_DEMUX_BOTH && ends != MNC_DEMUX_EITHER) { set_error("ends %d: one of MNC_DEMUX_FRONT / BOTH / EITHER is required", ends); return MNC_ERR_ARG; }
	if (cap_reads < 1 || cap_reads > DEMUX_MAX_READS) { set_error("cap_reads %lld outside 1 .. %lld", (long long)cap_reads, (long long)DEMUX_MAX_READS); return MNC_ERR_ARG; }
	mnc_demux *dm = new (std::nothrow) mnc_demux;
	if (!dm) return MNC_ERR_NOMEM;
	if (int rc = check_device(device)) { delete dm; return rc; }
	dm->n_barcodes = n_barcodes, dm->window = window, dm->max_dist = max_dist, dm->min_margin = min_margin, dm->ends = ends, dm->max_len = max_len;
	dm->cap_reads = cap_reads, dm->G = idx ? (int)idx->genome_name.size() : 0;
	// Adds run one behind the other on the device, whichever engine's they are: the taxa kernel reads the barcodes back from the
	// ONE tag store, so another engine's search between an add's two kernels would have this add's reads counted under that
	// batch's barcodes.  It also makes "the latest add's tags" one add's, never a mixture.  A search fills every wave slot of the
	// device, so two of them side by side would gain little.
	dm->serial = true;
	const size_t nb = (size_t)n_barcodes;
	hipError_t he = dm->begin(idx, device);
	if (he == hipSuccess) he = hipDeviceGetAttribute(&dm->n_cu, hipDeviceAttributeMultiprocessorCount, device);
	dm->alloc(he, (void**)&dm->peq, nb * 32);
	dm->alloc(he, (void**)&dm->plen, nb * 4);
	dm->alloc(he, (void**)&dm->reads, (nb + 2) * 8);
	if (idx) dm->alloc(he, (void**)&dm->taxa, (nb + 1) * (size_t)dm->G * 24);
	dm->alloc(he, (void**)&dm->tags, (size_t)cap_reads * sizeof(mnc_demux_tag_t));
	dm->streams(he);
	if (he == hipSuccess) dm->n_cu = std::max(dm->n_cu, 1);
	if (he == hipSuccess) he = hipMemcpy(dm->peq, peq.data(), nb * 32, hipMemcpyHostToDevice);
	if (he == hipSuccess) he = hipMemcpy(dm->plen, plen.data(), nb * 4, hipMemcpyHostToDevice);
	if (he != hipSuccess) {
		set_error("demux accumulator of %d barcodes, %d genomes and %lld reads (8 bytes each): %s", n_barcodes, dm->G, (long long)cap_reads, hipGetErrorString(he));
		const int rc = Accum::failed(he);
		mnc_demux_free(dm);
		return rc;
	}
	if (int rc = mnc_demux_reset(dm)) { mnc_demux_free(dm); return rc; }
	*out = dm;
	return MNC_OK;
}

extern "C" int mnc_demux_reset(mnc_demux *dm)
{
	if (!dm) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(dm->device));
	std::lock_guard<std::mutex> g(dm->mu);
	HIP_TRY(hipMemsetAsync(dm->reads, 0, (size_t)(dm->n_barcodes + 2) * 8, dm->st));
	if (dm->taxa) HIP_TRY(hipMemsetAsync(dm->taxa, 0, (size_t)(dm->n_barcodes + 1) * dm->G * 24, dm->st));
	hipLaunchKernelGGL(mnc_demux_clear, dim3((unsigned)((dm->cap_reads + 255) / 256)), dim3(256), 0, dm->st, dm->tags, dm->cap_reads);
	HIP_TRY(hipGetLastError());
	HIP_TRY(dm->own_done());
	return MNC_OK;
}

extern "C" int mnc_demux_device_bytes(const mnc_demux *dm, int64_t *bytes) { return accum_device_bytes(dm, bytes); }

extern "C" int mnc_demux_set_word_bits(mnc_demux *dm, int bits)
{
	if (!dm) return MNC_ERR_ARG;
	if (bits != 0 && bits != 64) { set_error("word bits %d: 0 (by the longest pattern) or 64", bits); return MNC_ERR_ARG; }
	std::lock_guard<std::mutex> g(dm->mu);
	dm->wide = bits == 64;
	return MNC_OK;
}

extern "C" int mnc_demux_info(mnc_demux *dm, int32_t *word_bits, int64_t *n_assigned, int64_t *n_none, int64_t *n_conflict)
{
	if (!dm) return MNC_ERR_ARG;
	if (word_bits) {
		std::lock_guard<std::mutex> g(dm->mu);
		*word_bits = dm->max_len <= 32 && !dm->wide ? 32 : 64;
	}
	if (!n_assigned && !n_none && !n_conflict) return MNC_OK;
	std::vector<int64_t> c;
	try {
		c.resize((size_t)dm->n_barcodes + 2);
	} catch (const std::bad_alloc &) { return MNC_ERR_NOMEM; }
	if (int rc = mnc_demux_fetch_counts(dm, c.data(), nullptr)) return rc;
	int64_t sum = 0;
	for (int b = 0; b < dm->n_barcodes; ++b) sum += c[(size_t)b];
	if (n_assigned) *n_assigned = sum;
	if (n_none) *n_none = c[(size_t)dm->n_barcodes];
	if (n_conflict) *n_conflict = c[(size_t)dm->n_barcodes + 1];
	return MNC_OK;
}

// The search on the caller's own arrays.  A host batch is checked (offsets from 0, ascending) and copied to buffers of the
// accumulator's on its stream, so the kernel comes behind the copy and the next call's copy behind the kernel; device arrays
// are taken as they are (the caller's to be right, as for mnc_classify_device) and must be complete on the caller's side.
extern "C" int mnc_demux_add(mnc_demux *dm, const uint8_t *bases, const int64_t *offsets, int64_t n_reads, int on_device)
{
	if (!dm) return MNC_ERR_ARG;
	if (n_reads < 0) { set_error("n_reads %lld: a number of reads", (long long)n_reads); return MNC_ERR_ARG; }
	if (int rc = demux_fits(dm, n_reads)) return rc;
	if (n_reads == 0) return MNC_OK;
	if (!offsets) { set_error("`offsets` is NULL"); return MNC_ERR_ARG; }
	int64_t total = 0;
	if (!on_device) {
		if (offsets[0] != 0) { set_error("offsets[0] is %lld: a batch begins at 0", (long long)offsets[0]); return MNC_ERR_ARG; }
		for (int64_t r = 0; r < n_reads; ++r)
			if (offsets[r + 1] < offsets[r]) { set_error("offsets[%lld] lies below offsets[%lld]", (long long)r + 1, (long long)r); return MNC_ERR_ARG; }
		total = offsets[n_reads];
	}
	if (!bases && (on_device || total)) { set_error("`bases` is NULL"); return MNC_ERR_ARG; }
	HIP_TRY(hipSetDevice(dm->device));
	std::lock_guard<std::mutex> lk(dm->mu);
	if (!on_device) {
		const size_t nb = (size_t)total + 8, no = ((size_t)n_reads + 1) * 8;
		if (nb > dm->in_bases_cap || no > dm->in_offsets_cap) {
			HIP_TRY(hipStreamSynchronize(dm->st));                 // an earlier add may still read the buffer that is let go
			hipError_t he = hipSuccess;
			dm->regrow(he, (void**)&dm->in_bases, dm->in_bases_cap, nb);
			dm->regrow(he, (void**)&dm->in_offsets, dm->in_offsets_cap, no);
			if (he != hipSuccess) { set_error("a batch of %lld bases in %lld reads: %s", (long long)total, (long long)n_reads, hipGetErrorString(he)); return Accum::failed(he); }
		}
		if (total) HIP_TRY(hipMemcpyAsync(dm->in_bases, bases, (size_t)total, hipMemcpyHostToDevice, dm->st));
		HIP_TRY(hipMemcpyAsync(dm->in_offsets, offsets, no, hipMemcpyHostToDevice, dm->st));
		bases = dm->in_bases, offsets = dm->in_offsets;
	}
	demux_launch(dm, bases, offsets, n_reads, dm->st);
	HIP_TRY(hipGetLastError());
	HIP_TRY(dm->own_done());                                   // an engine's add comes behind it
	if (!on_device) HIP_TRY(hipStreamSynchronize(dm->st));     // the caller's arrays are free again
	return MNC_OK;
}

extern "C" int mnc_demux_fetch_counts(mnc_demux *dm, int64_t *reads, int64_t *taxa)
{
	if (!dm) return MNC_ERR_ARG;
	if (taxa && !dm->taxa) { set_error("this demux accumulator was created without an index: it holds no taxa"); return MNC_ERR_ARG; }
	HIP_TRY(hipSetDevice(dm->device));
	return dm->finish(hipSuccess, nullptr, {reads, dm->reads, (size_t)(dm->n_barcodes + 2) * 8},
	                  {taxa, dm->taxa, (size_t)(dm->n_barcodes + 1) * dm->G * 24}, "demux counts");
}

extern "C" int mnc_demux_fetch_tags(mnc_demux *dm, int64_t first, int64_t n, mnc_demux_tag_t *out)
{
	if (!dm) return MNC_ERR_ARG;
	if (first < 0 || n < 0 || first > dm->cap_reads || n > dm->cap_reads - first) {
		set_error("reads [%lld, %lld) outside the %lld of the accumulator (cap_reads)", (long long)first, (long long)(first + n), (long long)dm->cap_reads);
		return MNC_ERR_ARG;
	}
	if (n == 0) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(dm->device));
	return dm->finish(hipSuccess, nullptr, {out, dm->tags + first, (size_t)n * sizeof(mnc_demux_tag_t)}, {}, "demux tags");
}

extern "C" int mnc_demux_device(mnc_demux *dm, const int64_t **d_reads, const int64_t **d_taxa, const mnc_demux_tag_t **d_tags)
{
	if (!dm) return MNC_ERR_ARG;
	if (d_reads) *d_reads = (const int64_t*)dm->reads;
	if (d_taxa) *d_taxa = (const int64_t*)dm->taxa;
	if (d_tags) *d_tags = dm->tags;
	return MNC_OK;
}
