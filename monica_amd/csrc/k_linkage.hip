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
