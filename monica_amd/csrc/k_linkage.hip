// Linkage (include/monica_amd.h, "linkage"): which variant alleles the reads carry TOGETHER -- per site of a caller's list a
// REF and an ALT count, per pair of sites up to `window` apart in the list the four joint counts, and from the adjacent
// pairs phase blocks.  The fifth consumer of a batch as it stands in HBM (regions, region CIGARs, the reads' bases, the
// contigs' 4-bit store), an accumulator of accum.h like the others; runs only when asked for.
//
//   mnc_link_add    one wave per READ, the records found and selected as mnc_pile_add does -- but the lanes hold SITES, not
//                   columns.  A record's sites are one contiguous range of the sorted list (two bisections of the contig's
//                   positions by rs and re), taken 64 at a time.  The CIGAR is walked 64 operations at a time with the
//                   inclusive sums of pile_add_read; sites and operations both ascend, so the two walks are a MERGE: a site
//                   lane whose position lies before the end of the chunk at hand finds its operation by bisecting the
//                   chunk's inclusive reference advance through cross-lane reads and fetches its one read base and its one
//                   reference nibble; when lanes are left, the chunk moves on.  The chunk stays where it is from one 64
//                   sites to the next (the next site may lie under the same operations).  Two ballots make the 64 statements
//                   two masks, REF and ALT; with the last 64 sites' masks a lane cuts the window of the 64 sites in front of
//                   its own out of the 128 bits, bit 63 - d being site i = j - d - 1.
//   the pair words  A naive form is one atomic per (pair, record) with both statements, and on a covered stretch nearly
//                   all of them are REF / REF.  That cell is DERIVED instead, as the pileup derives the reference count
//                   from the depth.  Per record and distance d, the pairs (i, i + d + 1) that lie inside its site range are
//                   a run of i: +1 / -1 in a difference track[n_sites][window] (two atomics per d and record, whatever the
//                   number of sites).  A pair inside the range that is NOT REF / REF costs its one atomic: on cell 1, 2 or 3
//                   with both statements, on word 0 ("missing") where either site has none.  On read-out
//                   n00[i][d] = (sum of track[0 .. i][d]) - (word 0 + n01 + n10 + n11)[i][d].  At 10 % errors that is a
//                   fifth of the atomics.  Every word stays additive, the differences included.
//   read-outs       fetch_pairs: scan.h's exclusive scan over the track read column by column (every column sums to zero:
//                   each +1 has its -1 inside the list, so no column carries into the next), then one thread per cell.
//                   phase: the same scan over column 0 alone; a second scan over (block start | flip << 32) per site, whose
//                   low half is the block number and whose bit 32 is the parity of the flips so far -- the segmented XOR is
//                   that parity against the parity at the block's start, which the first write pass leaves per block and
//                   the second reads.  Count, scan, write; only the answer travels.
//   phase_window    the read-out over every distance d < reach (include/monica_amd.h has the definition).  The same scan over
//                   the first reach columns of the track, then
//     mnc_linkw_parent  one workgroup per LW_TILE = 128 consecutive sites.  The rows [tile - reach, tile end) x reach cells
//                   go through LDS twice: first the track sums, read ALONG the columns as the scan leaves them (lanes on
//                   consecutive rows), then the cells, read along the rows as stored, 16 bytes a lane -- each cell becomes
//                   one 32-bit word, |cis - trans| in full width (it is below 2^32) or 0 where the pair is not linked; the
//                   orientation is bit d of a 64-bit mask per row.  Then the DIAGONALS: the lanes of a wave hold the d of one
//                   site (of 64 / G sites where reach <= G < 64, G a power of two), word[i - d - 1][d], and a butterfly of
//                   shuffles over (diff << 6 | 63 - d) gives the largest diff, ties to the smallest d.  One byte per site:
//                   the parent's distance, bit 7 its orientation; 0 = a root.
//                   The LDS row is reach words padded to S = 3 (mod 4): a column write has lane stride S (odd, no
//                   conflict), a diagonal read lane stride S - 1 = 2 (mod 4) (two lanes a bank at worst); with S a multiple
//                   of 64 either would put a whole wave on one bank.  At reach 64 a tile is 192 rows x 67 words + 192
//                   masks = 52 992 bytes: three workgroups in the 160 KB of a CU, below the 64 KB a launch gets without
//                   asking for more, and a halo of half the tile (256 sites would read a quarter but leave room for one
//                   workgroup only beside the 64 KB limit).
//     mnc_linkw_local   one workgroup per LJ_TILE = 1024 sites, the parent bytes of the tile and of the reach sites behind
//                   it in LDS.  Interval starts: site k is one iff none of the bytes k .. k + reach - 1 reaches in front
//                   of k.  Roots: pointer jumping in LDS over one word per site (target, resolved, parity -- one word, so
//                   a word read while its owner rewrites it is still a true statement), ten rounds; a site ends at a root of
//                   its tile (resolved) or at one of the last 64 sites of the tile in front.
//     mnc_linkw_hop     those last 64 sites per tile are the only doors between tiles: their words, compacted, jump among
//                   themselves -- ceil(log2(tiles)) rounds over n / 16 words, ping-pong, the count fixed by n_sites, no host
//                   wait between them.
//     mnc_linkw_write   every site takes at most one more hop through its door, then kept = its root is a start;
//                   block = the starts before the root (scan.h again), phase = the parity.
//   add_tables      tables as fetch_sites / fetch_pairs write them, checked on the host, added by one thread per cell: the
//                   three stored cells onto their words, the rise of the cell's total over the row above onto the track.
// Integer arithmetic throughout.
#include <hip/hip_runtime.h>
#include <new>
#include <vector>
#include "linkage.h"

using namespace mnc;

struct mnc_linkage : mnc::Accum {
	int64_t n_sites = 0;
	int window = 0, n_contigs = 0;
	LinkSitesDev list;                         // the sites' positions and alleles, the contigs' first sites and first bases (linkage.h)
	int32_t *d_rid = nullptr;                  // [n_sites] the sites' contigs
	int32_t *site = nullptr;                   // [n_sites][2]
	int32_t *pair = nullptr;                   // [n_sites][window][4]: missing, n01, n10, n11; behind them track[n_sites][window]
	int32_t *track = nullptr;
	int64_t words() const { return n_sites * window * 5; }   // of `pair` and `track` together
	// scratch of the read-outs
	int64_t *run0 = nullptr, *marks = nullptr; // [n_sites + 1] each: the scans of phase
	int64_t *sums = nullptr;                   // the scans' tile sums: [n_sites * window / SC_TILE + 2]
	int32_t *o_block = nullptr, *blk_par = nullptr;   // [n_sites] each
	uint8_t *o_phase = nullptr;                // [n_sites]
	std::vector<int32_t> h_first;              // [n_contigs + 1] the contigs' first sites, on the host (add_tables' check)
};

namespace mnc {

struct LinkView {
	LinkSites list;
	int window;
	int32_t *site, *pair, *track;
};

// the walk is linkage.h's; here, what is done with the 64 statements it hands over
__global__ __launch_bounds__(256) void mnc_link_add(Batch B, int sel, LinkView L)
{
	const int lane = lane_id(), W = L.window;
	const uint32_t rd = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (rd >= B.n_reads) return;                              // (whole waves; the kernel has no workgroup barrier)
	int s_lo = 0;
	unsigned long long p_ref = 0, p_alt = 0;                  // the statements of the 64 sites before
	link_walk(B, rd, sel, L.list, [&](int lo, int s_hi) {
		s_lo = lo, p_ref = p_alt = 0;
		// ---- the pairs inside the record's range, per distance: lane d's run of i is [s_lo, s_hi - d - 1)
		if (lane < W && s_hi - lane - 1 > s_lo) {
			link_put(L.track + (int64_t)s_lo * W + lane, 1);
			link_put(L.track + (int64_t)(s_hi - lane - 1) * W + lane, -1);
		}
	}, [&](int, int s, bool valid, int stmt) {
		const unsigned long long c_ref = __ballot(stmt == 1), c_alt = __ballot(stmt == 2);
		const int nb = valid ? min(W, s - s_lo) : 0;             // the sites in front of this one, in the window and in the record's range
		if (stmt) link_put(L.site + (int64_t)s * 2 + (stmt - 1), 1);
		if (nb > 0) {
			// sites s - 64 .. s - 1 as bits 0 .. 63: site s - d - 1 is bit 63 - d
			const unsigned long long v_ref = lane ? (p_ref >> lane) | (c_ref << (64 - lane)) : p_ref;
			const unsigned long long v_alt = lane ? (p_alt >> lane) | (c_alt << (64 - lane)) : p_alt;
			unsigned long long todo = ~0ull << (64 - nb);
			if (stmt == 1) todo &= ~v_ref;                        // REF / REF is derived
			while (todo) {
				const int b = 63 - __clzll((long long)todo), d = 63 - b;
				todo &= ~(1ull << b);
				const int a_i = (v_alt >> b & 1ull) ? 1 : (v_ref >> b & 1ull) ? 0 : -1;
				const int cell = a_i < 0 || !stmt ? 0 : 2 * a_i + (stmt - 1);
				link_put(L.pair + ((int64_t)(s - d - 1) * W + d) * 4 + cell, 1);
			}
		}
		p_ref = c_ref, p_alt = c_alt;
	});
}

// ---------------------------------------------------------------- read-outs
// the track column by column: element k is track[k % n][k / n]
struct LinkTrackIn {
	const int32_t *track;
	int64_t n;
	int W;
	__device__ long long operator()(int64_t k) const { return (long long)track[(k % n) * W + k / n]; }
};

// runs: the exclusive scan over LinkTrackIn, so the running sum up to and with (i, d) is runs[d * n + i + 1]
__global__ __launch_bounds__(256) void mnc_link_pairs(const int32_t *pair, const int64_t *runs, int64_t n_sites, int W, int64_t first, int64_t n, int32_t *out)
{
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n * W) return;
	const int64_t i = first + t / W;
	const int d = (int)(t % W);
	const int32_t *w = pair + (i * W + d) * 4;
	out[t * 4] = (int32_t)(runs[d * n_sites + i + 1] - ((long long)w[0] + w[1] + w[2] + w[3]));
	for (int c = 1; c < 4; ++c) out[t * 4 + c] = w[c];
}

// per site i: 1 where it starts a block, 1 << 32 where it is linked to site i - 1 in trans
struct LinkMarkIn {
	const int32_t *pair, *rid;
	const int64_t *run0;                      // the exclusive scan over column 0 of the track
	int W, min_pairs, min_permille;
	__device__ long long operator()(int64_t i) const
	{
		if (i == 0 || rid[i] != rid[i - 1]) return 1;
		const int32_t *w = pair + (i - 1) * W * 4;
		const long long n01 = w[1], n10 = w[2], n11 = w[3], n00 = run0[i] - (w[0] + n01 + n10 + n11);
		const long long cis = n00 + n11, trans = n01 + n10, tot = cis + trans, diff = cis > trans ? cis - trans : trans - cis;
		if (tot < min_pairs || cis == trans || diff * 1000 < (long long)min_permille * tot) return 1;
		return trans > cis ? 1ll << 32 : 0;
	}
};

// marks: the exclusive scan over LinkMarkIn.  The inclusive one at i holds the blocks so far in its low half and the flips
// so far in its high half; a block's first site leaves the parity of the flips before the block.
__global__ __launch_bounds__(256) void mnc_link_blocks(const int64_t *marks, int64_t n, int32_t *block, int32_t *blk_par)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int64_t v = marks[i + 1];
	const int32_t b = (int32_t)(v & 0xffffffffll) - 1;
	block[i] = b;
	if ((v & 0xffffffffll) != (marks[i] & 0xffffffffll)) blk_par[b] = (int32_t)(v >> 32 & 1);
}

__global__ __launch_bounds__(256) void mnc_link_phase(const int64_t *marks, int64_t n, const int32_t *block, const int32_t *blk_par, uint8_t *phase)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) phase[i] = (uint8_t)((marks[i + 1] >> 32 & 1) ^ blk_par[block[i]]);
}

// ---------------------------------------------------------------- phase_window
constexpr int LW_TILE = 128, LW_THREADS = 256;                // mnc_linkw_parent: sites per workgroup
constexpr int LJ_TILE = 1024, LJ_THREADS = 256, LJ_DOOR = 64, LJ_ROUNDS = 10;   // mnc_linkw_local; 2^LJ_ROUNDS >= LJ_TILE, LJ_DOOR >= the window

// words of one LDS row of `reach` cells: the next number that is 3 (mod 4)
__host__ __device__ inline int linkw_stride(int R) { return R + ((3 - R) & 3); }
inline size_t linkw_lds(int R) { return (size_t)(LW_TILE + R) * (8 + 4 * (size_t)linkw_stride(R)); }

// runs: the exclusive scan over the first n * R elements of LinkTrackIn.  par[i]: 0 = a root, else the parent's distance
// i - p(i) in bits 0 .. 6 and the link's orientation in bit 7.
__global__ __launch_bounds__(LW_THREADS) void mnc_linkw_parent(const int32_t *pair, const int64_t *runs, const int32_t *rid, const int32_t *first, int64_t n, int W,
                                                               int R, int min_pairs, int min_permille, uint8_t *par)
{
	extern __shared__ unsigned long long lw_lds[];
	const int S = linkw_stride(R);
	unsigned long long *omask = lw_lds;                       // [rows] bit d: cell (row, d) is linked in trans
	uint32_t *word = (uint32_t*)(lw_lds + LW_TILE + R);       // [rows][S] first the track sum, then |cis - trans| or 0
	const int64_t t0 = (int64_t)blockIdx.x * LW_TILE;
	const int64_t lo = t0 > R ? t0 - R : 0, hi = t0 + LW_TILE < n ? t0 + LW_TILE : n;
	const int rows = (int)(hi - lo);                          // <= LW_TILE + R
	for (int r = threadIdx.x; r < rows; r += LW_THREADS) omask[r] = 0;
	// ---- the track sums, along the columns (the low half: n00 fits int32, so the difference below is exact modulo 2^32)
	for (int e = threadIdx.x; e < rows * R; e += LW_THREADS) {
		const int d = e / rows, r = e - d * rows;
		word[r * S + d] = (uint32_t)runs[(int64_t)d * n + lo + r + 1];
	}
	__syncthreads();
	// ---- the cells, along the rows: one link word each
	for (int e = threadIdx.x; e < rows * R; e += LW_THREADS) {
		const int r = e / R, d = e - r * R;
		const int4 w = *reinterpret_cast<const int4*>(pair + ((lo + r) * W + d) * 4);
		const long long n00 = (int32_t)(word[r * S + d] - ((uint32_t)w.x + (uint32_t)w.y + (uint32_t)w.z + (uint32_t)w.w));
		const long long cis = n00 + w.w, trans = (long long)w.y + w.z, tot = cis + trans, diff = cis > trans ? cis - trans : trans - cis;
		const bool linked = tot >= min_pairs && cis != trans && diff * 1000 >= (long long)min_permille * tot;
		word[r * S + d] = linked ? (uint32_t)diff : 0u;         // (diff < 2^32: cis and trans are sums of two int32 counts)
		if (linked && trans > cis) atomicOr(&omask[r], 1ull << d);
	}
	__syncthreads();
	// ---- the diagonals: G lanes per site, lane d of them holds word[i - d - 1][d]
	int G = 1;
	while (G < R) G <<= 1;
	const int lane = lane_id(), per = 64 / G, d = lane & (G - 1);
	for (int base = (int)(threadIdx.x >> 6) * per; base < LW_TILE; base += (LW_THREADS / 64) * per) {   // (the wave's own bounds)
		const int64_t i = t0 + base + lane / G;
		const bool ok = i < n && d < R && i - d - 1 >= first[rid[i]];   // (so i - d - 1 >= lo: d < R and i >= t0)
		long long key = ok ? (long long)word[(int)(i - d - 1 - lo) * S + d] << 6 | (63 - d) : 0;
		for (int off = G >> 1; off > 0; off >>= 1) {
			const long long o = __shfl_xor(key, off);
			key = o > key ? o : key;
		}
		if (d == 0 && i < n) {
			int b = 0;
			if (key >> 6) {
				const int dd = 63 - (int)(key & 63);
				b = (dd + 1) | (int)(omask[(int)(i - dd - 1 - lo)] >> dd & 1ull) << 7;
			}
			par[i] = (uint8_t)b;
		}
	}
}

// A site's word, here and below: target << 2 | resolved << 1 | parity of the orientations from the site to the target.
// resolved: the target is the site's root.  In LDS the target is tile-relative + LJ_DOOR; in `res` and `door` it is the site.
__device__ __forceinline__ uint32_t linkw_join(uint32_t s, uint32_t u) { return (u & ~1u) | ((s ^ u) & 1u); }

// door[tile * LJ_DOOR + k]: the word of the tile's site LJ_TILE - LJ_DOOR + k
__global__ __launch_bounds__(LJ_THREADS) void mnc_linkw_local(const uint8_t *par, int64_t n, int R, uint8_t *start, uint32_t *res, uint32_t *door)
{
	__shared__ uint8_t pb[LJ_TILE + LJ_DOOR];
	__shared__ uint32_t st[LJ_TILE];
	const int64_t t0 = (int64_t)blockIdx.x * LJ_TILE;
	for (int k = threadIdx.x; k < LJ_TILE + LJ_DOOR; k += LJ_THREADS) pb[k] = t0 + k < n ? par[t0 + k] : 0;
	__syncthreads();
	for (int sl = threadIdx.x; sl < LJ_TILE; sl += LJ_THREADS) {
		bool is_start = true;                                   // no parent edge from k .. k + R - 1 to in front of k
		for (int j = 0; j < R; ++j) is_start &= (pb[sl + j] & 127) <= j;
		const int dist = pb[sl] & 127;
		st[sl] = dist ? (uint32_t)(sl + LJ_DOOR - dist) << 2 | (uint32_t)(pb[sl] >> 7) : (uint32_t)(sl + LJ_DOOR) << 2 | 2u;
		if (t0 + sl < n) start[t0 + sl] = is_start;
	}
	volatile uint32_t *v = st;
	for (int round = 0; round < LJ_ROUNDS; ++round) {
		__syncthreads();
		for (int sl = threadIdx.x; sl < LJ_TILE; sl += LJ_THREADS) {
			const uint32_t s = v[sl];
			if (!(s & 2u) && (s >> 2) >= (uint32_t)LJ_DOOR) v[sl] = linkw_join(s, v[(s >> 2) - LJ_DOOR]);
		}
	}
	__syncthreads();
	for (int sl = threadIdx.x; sl < LJ_TILE; sl += LJ_THREADS) {
		const uint32_t s = st[sl];
		// (tile 0 has no target in front of it: t0 + target - LJ_DOOR >= 0.)  Behind the list: a root nobody asks for
		const uint32_t out = t0 + sl < n ? (uint32_t)(t0 + (int64_t)(s >> 2) - LJ_DOOR) << 2 | (s & 3u) : 2u;
		if (t0 + sl < n) res[t0 + sl] = out;
		if (sl >= LJ_TILE - LJ_DOOR) door[(int64_t)blockIdx.x * LJ_DOOR + sl - (LJ_TILE - LJ_DOOR)] = out;
	}
}

// one hop of word s through the doors: an unresolved word's target is a door of the tile in front
__device__ __forceinline__ uint32_t linkw_through(uint32_t s, const uint32_t *door, int64_t n_door)
{
	const uint32_t t = s >> 2, k = t % LJ_TILE;
	const int64_t at = (int64_t)(t / LJ_TILE) * LJ_DOOR + k - (LJ_TILE - LJ_DOOR);
	if ((s & 2u) || k < (uint32_t)(LJ_TILE - LJ_DOOR) || at >= n_door) return s;
	return linkw_join(s, door[at]);
}

__global__ __launch_bounds__(256) void mnc_linkw_hop(const uint32_t *in, int64_t n_door, uint32_t *out)
{
	const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (x < n_door) out[x] = linkw_through(in[x], in, n_door);
}

// marks: the exclusive scan over start[]
__global__ __launch_bounds__(256) void mnc_linkw_write(const uint32_t *res, const uint32_t *door, int64_t n_door, const uint8_t *start, const int64_t *marks, int64_t n,
                                                       int32_t *block, uint8_t *phase, unsigned long long *n_kept)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool kept = false;
	if (i < n) {
		const uint32_t s = linkw_through(res[i], door, n_door);
		const int64_t root = s >> 2;
		kept = start[root];
		block[i] = kept ? (int32_t)marks[root] : -1;
		phase[i] = kept ? (uint8_t)(s & 1u) : (uint8_t)0;
	}
	const unsigned long long m = __ballot(kept);
	if (lane_id() == 0 && m) atomicAdd(n_kept, (unsigned long long)__popcll(m));
}

// ---------------------------------------------------------------- add_tables
// in_site[n][2], in_pair[n][W][4] as the fetches write them, checked by the caller
__global__ __launch_bounds__(256) void mnc_link_add_tables(const int32_t *in_site, const int32_t *in_pair, int64_t n, int W, int32_t *site, int32_t *pair, int32_t *track)
{
	const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n * W) return;
	const int32_t *c = in_pair + t * 4;
	long long rise = (long long)c[0] + c[1] + c[2] + c[3];       // of the cell's total over the row above
	if (t >= W) rise -= (long long)c[-4 * W] + c[-4 * W + 1] + c[-4 * W + 2] + c[-4 * W + 3];
	for (int k = 1; k < 4; ++k)
		if (c[k]) link_put(pair + t * 4 + k, c[k]);
	if (rise) link_put(track + t, (int)rise);
	if (t % W == 0)
		for (int k = 0; k < 2; ++k)
			if (in_site[t / W * 2 + k]) link_put(site + t / W * 2 + k, in_site[t / W * 2 + k]);
}

// ---------------------------------------------------------------- the engine's side (mnc_engine_add_linkage, engine.hip)
const Accum *as_accum(const mnc_linkage *lk) { return lk; }

int linkage_add(mnc_linkage *lk, const Batch &B, int sel, hipStream_t st)
{
	if (B.n_reads == 0 || lk->n_sites == 0) return MNC_OK;
	const LinkView L{lk->list.view(lk->n_contigs), lk->window, lk->site, lk->pair, lk->track};
	return lk->add(st, [&] { hipLaunchKernelGGL(mnc_link_add, dim3((B.n_reads + 3) / 4), dim3(256), 0, st, B, sel, L); });
}

} // namespace mnc

// ---------------------------------------------------------------- C-ABI
extern "C" void mnc_linkage_free(mnc_linkage *lk)
{
	if (!lk) return;
	lk->release();
	delete lk;
}

extern "C" int mnc_linkage_create(mnc_index *idx, int device, const mnc_variant_t *sites, int64_t n_sites, int32_t window, mnc_linkage **out)
{
	if (!idx || !out) return MNC_ERR_ARG;
	*out = nullptr;
	if (n_sites < 0 || (n_sites && !sites)) return MNC_ERR_ARG;
	if (window < 1 || window > MNC_LINKAGE_MAX_WINDOW) { set_error("window %d outside 1 .. %d", (int)window, MNC_LINKAGE_MAX_WINDOW); return MNC_ERR_ARG; }
	LinkSitesHost H;
	if (int rc = link_sites_check(idx, sites, n_sites, H)) return rc;
	const int n_contigs = H.n_contigs;
	mnc_linkage *lk = new (std::nothrow) mnc_linkage;
	if (!lk) return MNC_ERR_NOMEM;
	if (int rc = check_device(device)) { delete lk; return rc; }
	lk->n_sites = n_sites, lk->window = window, lk->n_contigs = n_contigs;
	const size_t ns = (size_t)n_sites, nw = (size_t)lk->words();
	hipError_t he = lk->begin(idx, device);
	lk->list.alloc(*lk, he, H);
	lk->alloc(he, (void**)&lk->d_rid, ns * 4);
	lk->alloc(he, (void**)&lk->site, ns * 8);
	lk->alloc(he, (void**)&lk->pair, nw * 4);
	lk->alloc(he, (void**)&lk->run0, (ns + 1) * 8);
	lk->alloc(he, (void**)&lk->marks, (ns + 1) * 8);
	lk->alloc(he, (void**)&lk->sums, (ns * (size_t)window / SC_TILE + 2) * 8);
	lk->alloc(he, (void**)&lk->o_block, ns * 4);
	lk->alloc(he, (void**)&lk->blk_par, ns * 4);
	lk->alloc(he, (void**)&lk->o_phase, ns);
	lk->streams(he);
	if (he == hipSuccess) lk->track = lk->pair + ns * (size_t)window * 4;
	lk->list.fill(he, H);
	if (he == hipSuccess && ns) he = hipMemcpy(lk->d_rid, H.rid.data(), ns * 4, hipMemcpyHostToDevice);
	if (he != hipSuccess) {
		set_error("linkage accumulator of %lld sites, window %d (%d bytes a site): %s", (long long)n_sites, (int)window, 20 * window + 50, hipGetErrorString(he));
		const int rc = Accum::failed(he);
		mnc_linkage_free(lk);
		return rc;
	}
	lk->h_first.swap(H.first);
	if (int rc = mnc_linkage_reset(lk)) { mnc_linkage_free(lk); return rc; }
	*out = lk;
	return MNC_OK;
}

extern "C" int mnc_linkage_reset(mnc_linkage *lk)
{
	if (!lk) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(lk->device));
	std::lock_guard<std::mutex> g(lk->mu);
	if (lk->n_sites) {
		HIP_TRY(hipMemsetAsync(lk->site, 0, (size_t)lk->n_sites * 8, lk->st));
		HIP_TRY(hipMemsetAsync(lk->pair, 0, (size_t)lk->words() * 4, lk->st));
	}
	HIP_TRY(lk->own_done());
	return MNC_OK;
}

extern "C" int mnc_linkage_device_bytes(const mnc_linkage *lk, int64_t *bytes) { return accum_device_bytes(lk, bytes); }

extern "C" int mnc_linkage_device(mnc_linkage *lk, const int32_t **d_site, const int32_t **d_pair)
{
	if (!lk) return MNC_ERR_ARG;
	if (d_site) *d_site = lk->n_sites ? lk->site : nullptr;
	if (d_pair) *d_pair = lk->n_sites ? lk->pair : nullptr;
	return MNC_OK;
}

// rows [first, first + n) of the site list
static int link_rows(const mnc_linkage *lk, int64_t first, int64_t n)
{
	if (first < 0 || n < 0 || first > lk->n_sites || n > lk->n_sites - first) {
		set_error("sites [%lld, %lld) outside the list of %lld", (long long)first, (long long)(first + n), (long long)lk->n_sites);
		return MNC_ERR_ARG;
	}
	return MNC_OK;
}

extern "C" int mnc_linkage_fetch_sites(mnc_linkage *lk, int64_t first, int64_t n, int32_t *out)
{
	if (!lk) return MNC_ERR_ARG;
	if (int rc = link_rows(lk, first, n)) return rc;
	if (n == 0) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(lk->device));
	return lk->finish(hipSuccess, nullptr, {out, lk->site + first * 2, (size_t)n * 8}, {}, "linkage site counts");
}

extern "C" int mnc_linkage_fetch_pairs(mnc_linkage *lk, int64_t first, int64_t n, int32_t *out)
{
	if (!lk) return MNC_ERR_ARG;
	if (int rc = link_rows(lk, first, n)) return rc;
	if (n == 0) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(lk->device));
	const int W = lk->window;
	const int64_t cells = lk->n_sites * W;
	const size_t out_bytes = (size_t)n * W * 16;
	char *tmp = nullptr;                                        // the cells, then the scan of the track
	HIP_TRY(hipMalloc((void**)&tmp, out_bytes + (size_t)(cells + 1) * 8));
	int64_t *runs = (int64_t*)(tmp + out_bytes);
	exclusive_scan(LinkTrackIn{lk->track, lk->n_sites, W}, cells, runs, lk->sums, lk->st);
	hipLaunchKernelGGL(mnc_link_pairs, dim3((unsigned)((n * W + 255) / 256)), dim3(256), 0, lk->st, lk->pair, runs, lk->n_sites, W, first, n, (int32_t*)tmp);
	return lk->finish(hipSuccess, tmp, {out, tmp, out_bytes}, {}, "linkage pairs");
}

extern "C" int mnc_linkage_phase(mnc_linkage *lk, int32_t min_pairs, int32_t min_permille, int32_t *block, uint8_t *phase)
{
	if (!lk) return MNC_ERR_ARG;
	const int64_t n = lk->n_sites;
	if (n == 0) return MNC_OK;
	if (!block || !phase) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(lk->device));
	const unsigned nb = (unsigned)((n + 255) / 256);
	// column 0 of the track: the first n elements of the column-by-column order
	exclusive_scan(LinkTrackIn{lk->track, n, lk->window}, n, lk->run0, lk->sums, lk->st);
	exclusive_scan(LinkMarkIn{lk->pair, lk->d_rid, lk->run0, lk->window, min_pairs, min_permille}, n, lk->marks, lk->sums, lk->st);
	hipLaunchKernelGGL(mnc_link_blocks, dim3(nb), dim3(256), 0, lk->st, lk->marks, n, lk->o_block, lk->blk_par);
	hipLaunchKernelGGL(mnc_link_phase, dim3(nb), dim3(256), 0, lk->st, lk->marks, n, lk->o_block, lk->blk_par, lk->o_phase);
	return lk->finish(hipSuccess, nullptr, {block, lk->o_block, (size_t)n * 4}, {phase, lk->o_phase, (size_t)n}, "linkage phase");
}

extern "C" int mnc_linkage_phase_window(mnc_linkage *lk, int32_t reach, int32_t min_pairs, int32_t min_permille, int32_t *block, uint8_t *phase, int64_t *n_kept)
{
	if (!lk) return MNC_ERR_ARG;
	if (reach < 1 || reach > lk->window) { set_error("reach %d outside 1 .. the window %d", (int)reach, lk->window); return MNC_ERR_ARG; }
	const int64_t n = lk->n_sites;
	if (n_kept) *n_kept = 0;
	if (n == 0) return MNC_OK;
	if (!block || !phase) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(lk->device));
	const int R = reach;
	const int64_t tiles = (n + LJ_TILE - 1) / LJ_TILE, n_door = tiles * LJ_DOOR;
	int rounds = 0;                                             // a door's word spans 2^rounds tiles after that many hops
	while (((int64_t)1 << rounds) < tiles) ++rounds;
	// the scan of the track's first R columns, the doors twice, the count; the rest is the phase read-out's scratch
	const size_t b_runs = (size_t)(n * R + 1) * 8, b_door = (size_t)n_door * 4;
	char *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, b_runs + 2 * b_door + 8));
	int64_t *runs = (int64_t*)tmp;
	uint32_t *door[2] = {(uint32_t*)(tmp + b_runs), (uint32_t*)(tmp + b_runs + b_door)};
	unsigned long long *cnt = (unsigned long long*)(tmp + b_runs + 2 * b_door);
	uint8_t *par = (uint8_t*)lk->run0, *start = par + n;       // (run0 holds 8 bytes a site)
	uint32_t *res = (uint32_t*)lk->blk_par;
	const unsigned nb = (unsigned)((n + 255) / 256);
	hipError_t e = hipMemsetAsync(cnt, 0, 8, lk->st);
	exclusive_scan(LinkTrackIn{lk->track, n, lk->window}, n * R, runs, lk->sums, lk->st);
	hipLaunchKernelGGL(mnc_linkw_parent, dim3((unsigned)((n + LW_TILE - 1) / LW_TILE)), dim3(LW_THREADS), linkw_lds(R), lk->st, lk->pair, runs, lk->d_rid,
	                   lk->list.first, n, lk->window, R, min_pairs, min_permille, par);
	hipLaunchKernelGGL(mnc_linkw_local, dim3((unsigned)tiles), dim3(LJ_THREADS), 0, lk->st, par, n, R, start, res, door[0]);
	for (int r = 0; r < rounds; ++r)
		hipLaunchKernelGGL(mnc_linkw_hop, dim3((unsigned)((n_door + 255) / 256)), dim3(256), 0, lk->st, door[r & 1], n_door, door[(r + 1) & 1]);
	exclusive_scan(ScanInPlain<uint8_t>{start}, n, lk->marks, lk->sums, lk->st);
	hipLaunchKernelGGL(mnc_linkw_write, dim3(nb), dim3(256), 0, lk->st, res, door[rounds & 1], n_door, start, lk->marks, n, lk->o_block, lk->o_phase, cnt);
	if (e == hipSuccess) e = hipGetLastError();
	if (e == hipSuccess && n_kept) e = hipMemcpyAsync(n_kept, cnt, 8, hipMemcpyDeviceToHost, lk->st);
	return lk->finish(e, tmp, {block, lk->o_block, (size_t)n * 4}, {phase, lk->o_phase, (size_t)n}, "linkage phase over the window");
}

extern "C" int mnc_linkage_add_tables(mnc_linkage *lk, const int32_t *site, const int32_t *pair)
{
	if (!lk) return MNC_ERR_ARG;
	const int64_t n = lk->n_sites;
	const int W = lk->window;
	if (n == 0) return MNC_OK;
	if (!site || !pair) return MNC_ERR_ARG;
	// ---- every check on the host, before anything is touched
	int c = 0;                                                  // the contig of site i
	for (int64_t i = 0; i < n; ++i) {
		while (i >= lk->h_first[c + 1]) ++c;
		for (int k = 0; k < 2; ++k)
			if (site[i * 2 + k] < 0) { set_error("site[%lld][%d] = %d is negative", (long long)i, k, (int)site[i * 2 + k]); return MNC_ERR_ARG; }
		for (int d = 0; d < W; ++d)
			for (int k = 0; k < 4; ++k) {
				const int32_t v = pair[(i * W + d) * 4 + k];
				if (v < 0) { set_error("pair[%lld][%d][%d] = %d is negative", (long long)i, d, k, (int)v); return MNC_ERR_ARG; }
				if (v && i + d + 1 >= lk->h_first[c + 1]) {
					set_error("pair[%lld][%d][%d] = %d, but site %lld lies past the last site of contig %d", (long long)i, d, k, (int)v, (long long)(i + d + 1), c);
					return MNC_ERR_ARG;
				}
			}
	}
	HIP_TRY(hipSetDevice(lk->device));
	const size_t b_site = (size_t)n * 8, b_pair = (size_t)n * W * 16;
	char *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, b_pair + b_site));
	std::lock_guard<std::mutex> g(lk->mu);
	hipError_t he = hipMemcpyAsync(tmp, pair, b_pair, hipMemcpyHostToDevice, lk->st);
	if (he == hipSuccess) he = hipMemcpyAsync(tmp + b_pair, site, b_site, hipMemcpyHostToDevice, lk->st);
	if (he == hipSuccess) {
		hipLaunchKernelGGL(mnc_link_add_tables, dim3((unsigned)((n * W + 255) / 256)), dim3(256), 0, lk->st, (const int32_t*)(tmp + b_pair), (const int32_t*)tmp, n, W,
		                   lk->site, lk->pair, lk->track);
		he = hipGetLastError();
	}
	if (he == hipSuccess) he = lk->own_done();                   // an engine's add comes behind it
	const hipError_t hs = hipStreamSynchronize(lk->st);         // the host arrays are read until here
	if (he == hipSuccess) he = hs;
	(void)hipFree(tmp);
	if (he != hipSuccess) { set_error("linkage add_tables: %s", hipGetErrorString(he)); return MNC_ERR_HIP; }
	return MNC_OK;
}
