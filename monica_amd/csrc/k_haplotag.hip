// Haplotag (include/monica_amd.h, "haplotag"): which reads belong to which side of a phase block -- per block of the caller's
// (block[], phase[]) how many records were decided for haplotype 0, for haplotype 1, how many stayed undecided and how many
// votes went against the record's own majority; per read of the last batch its best decision.  The sixth consumer of a batch
// as it stands in HBM, an accumulator of accum.h like the others; runs only when asked for.
//
//   mnc_hap_add     one wave per READ, the lanes hold SITES: the walk is linkage.h's, the one mnc_link_add runs, and hands over
//                   64 statements at a time.  A statement a at site s is a vote for haplotype a XOR phase[s] of block[s]; two
//                   ballots make the 64 votes two masks, v0 and v1.  Blocks ascend along the list, so a block's sites are a
//                   run of lanes: a third ballot marks the HEADS, the lanes whose block differs from the lane below (lane 0:
//                   from the block carried in).  Lane 0 and every head own a segment -- the bits from themselves up to the next
//                   head -- and count it with two popcounts of v0 / v1 under the segment's mask: no shuffle, no LDS.
//   the border      The last segment of 64 sites stays OPEN when the record's next site lies in the same block (one
//                   wave-uniform load of block[c0 + 64]).  It crosses the border as three wave-uniform scalars -- block, n0,
//                   n1 -- which every lane computes for itself from the masks; lane 0's segment adds them.  Every other
//                   segment CLOSES where it stands: its owner makes the decision and issues at most two atomics, one on the
//                   decision word, one on the minority word where that is not zero.
//   the read's tag  A wave-uniform running maximum of |n0 - n1| over the decided closures, records in cov_for_records order,
//                   blocks ascending: per 64 sites a ballot of the closing lanes that beat it, taken in ascending lane order
//                   with three cross-lane reads each, so ties stay with the first.  Lane 0 writes tag and votes once, with
//                   plain stores, for EVERY read of the batch: a read without a record writes -1.
// Integer arithmetic throughout; no workgroup barrier, no host wait.
#include <hip/hip_runtime.h>
#include <new>
#include <vector>
#include "linkage.h"

using namespace mnc;

struct mnc_haplotag : mnc::Accum {
	int64_t n_sites = 0, n_blocks = 0, cap_reads = 0;
	int64_t last_reads = 0;                    // the reads of the most recent add (under `mu`)
	int n_contigs = 0, min_votes = 0, min_permille = 0;
	LinkSitesDev list;                         // the site list on the device (linkage.h)
	int32_t *d_block = nullptr;                // [n_sites]
	uint8_t *d_phase = nullptr;                // [n_sites]
	int32_t *blk = nullptr;                    // [n_blocks][4]: decided 0, decided 1, undecided, minority votes
	int32_t *tag = nullptr;                    // [cap_reads]; behind it votes[cap_reads][2]
	int32_t *votes = nullptr;
};

namespace mnc {

__global__ __launch_bounds__(256) void mnc_hap_add(Batch B, int sel, HapView H)
{
	const int lane = lane_id();
	const uint32_t rd = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (rd >= B.n_reads) return;                              // (whole waves; the kernel has no workgroup barrier)
	int best = 0, best_tag = -1, best_n0 = 0, best_n1 = 0;    // the read's best decision so far: |n0 - n1| and whose it is
	int s_hi = 0;
	int cb = -1, cn0 = 0, cn1 = 0;                            // the open block carried over the last 64 sites' border
	link_walk(B, rd, sel, H.list, [&](int, int hi) { s_hi = hi, cb = -1, cn0 = cn1 = 0; }, [&](int c0, int s, bool valid, int stmt) {
		const HapSeg g = hap_segment(H.block, H.phase, c0, s, valid, stmt, s_hi, cb, cn0, cn1);
		const int b = g.b, n0 = g.n0, n1 = g.n1, diff = n0 > n1 ? n0 - n1 : n1 - n0;
		const bool closes = g.closes, decided = closes && hap_decided(n0, n1, H.min_votes, H.min_permille);
		if (closes) {
			int32_t *w = H.blk + (int64_t)b * 4;
			link_put(w + (decided ? (int)(n1 > n0) : 2), 1);
			if (min(n0, n1)) link_put(w + 3, min(n0, n1));
		}
		// ---- the read's best: the closing lanes that beat it, in ascending lane order
		for (unsigned long long cand = __ballot(decided && diff > best); cand; ) {
			const int l = __ffsll((long long)cand) - 1;
			const int x0 = __shfl(n0, l), x1 = __shfl(n1, l);
			best = x0 > x1 ? x0 - x1 : x1 - x0, best_n0 = x0, best_n1 = x1, best_tag = __shfl(b, l) * 2 + (int)(x1 > x0);
			cand = l < 63 ? __ballot(decided && diff > best) & (~0ull << (l + 1)) : 0ull;
		}
	});
	if (lane == 0) {
		H.tag[rd] = best_tag;
		H.votes[(int64_t)rd * 2] = max(best_n0, best_n1), H.votes[(int64_t)rd * 2 + 1] = min(best_n0, best_n1);
	}
}

// ---------------------------------------------------------------- the engine's side (mnc_engine_add_haplotag, engine.hip)
const Accum *as_accum(const mnc_haplotag *ht) { return ht; }

// MNC_ERR_RANGE, before anything is touched, when the batch holds more reads than the tag buffer
int haplotag_fits(const mnc_haplotag *ht, const Batch &B)
{
	if ((int64_t)B.n_reads <= ht->cap_reads) return MNC_OK;
	set_error("the batch holds %lld reads, the haplotag accumulator was created for %lld (cap_reads)", (long long)B.n_reads, (long long)ht->cap_reads);
	return MNC_ERR_RANGE;
}

HapView haplotag_view(const mnc_haplotag *ht)
{
	return HapView{ht->list.view(ht->n_contigs), ht->d_block, ht->d_phase, ht->min_votes, ht->min_permille, ht->blk, ht->tag, ht->votes};
}

int haplotag_add(mnc_haplotag *ht, const Batch &B, int sel, hipStream_t st)
{
	const HapView H = haplotag_view(ht);
	return ht->add(st, [&] {
		ht->last_reads = B.n_reads;
		if (B.n_reads) hipLaunchKernelGGL(mnc_hap_add, dim3((B.n_reads + 3) / 4), dim3(256), 0, st, B, sel, H);
	});
}

} // namespace mnc

// ---------------------------------------------------------------- C-ABI
extern "C" void mnc_haplotag_free(mnc_haplotag *ht)
{
	if (!ht) return;
	ht->release();
	delete ht;
}

// block[] and phase[] as mnc_linkage_phase writes them, over the list `H`
static int hap_blocks_check(const LinkSitesHost &H, int64_t n_sites, const int32_t *block, const uint8_t *phase)
{
	if (n_sites && (!block || !phase)) return MNC_ERR_ARG;
	for (int64_t i = 0; i < n_sites; ++i) {
		const bool start = i == 0 || block[i] != block[i - 1];
		if (i == 0 ? block[0] != 0 : (block[i] - (int64_t)block[i - 1] != 0 && block[i] - (int64_t)block[i - 1] != 1))
			set_error("site %lld: block %d after block %d (blocks start at 0 and ascend by 0 or 1)", (long long)i, (int)block[i], i ? (int)block[i - 1] : -1);
		else if (i && H.rid[i] != H.rid[i - 1] && !start)
			set_error("site %lld: the first site of contig %d continues block %d (a contig change starts a block)", (long long)i, (int)H.rid[i], (int)block[i]);
		else if (phase[i] > 1) set_error("site %lld: phase %d is neither 0 nor 1", (long long)i, (int)phase[i]);
		else if (start && phase[i]) set_error("site %lld: phase 1 at the first site of block %d (a block starts at phase 0)", (long long)i, (int)block[i]);
		else continue;
		return MNC_ERR_ARG;
	}
	return MNC_OK;
}

extern "C" int mnc_haplotag_create(mnc_index *idx, int device, const mnc_variant_t *sites, int64_t n_sites, const int32_t *block, const uint8_t *phase,
                                   int64_t cap_reads, int32_t min_votes, int32_t min_permille, mnc_haplotag **out)
{
	if (!idx || !out) return MNC_ERR_ARG;
	*out = nullptr;
	LinkSitesHost L;
	if (int rc = link_sites_check(idx, sites, n_sites, L)) return rc;
	if (int rc = hap_blocks_check(L, n_sites, block, phase)) return rc;
	if (min_votes < 1) { set_error("min_votes %d below 1", (int)min_votes); return MNC_ERR_ARG; }
	if (min_permille < 0 || min_permille > 1000) { set_error("min_permille %d outside 0 .. 1000", (int)min_permille); return MNC_ERR_ARG; }
	if (cap_reads < 1 || cap_reads > MNC_HAPLOTAG_MAX_READS) {
		set_error("cap_reads %lld outside 1 .. %lld", (long long)cap_reads, (long long)MNC_HAPLOTAG_MAX_READS);
		return MNC_ERR_ARG;
	}
	mnc_haplotag *ht = new (std::nothrow) mnc_haplotag;
	if (!ht) return MNC_ERR_NOMEM;
	if (int rc = check_device(device)) { delete ht; return rc; }
	ht->n_sites = n_sites, ht->n_blocks = n_sites ? (int64_t)block[n_sites - 1] + 1 : 0, ht->cap_reads = cap_reads;
	ht->n_contigs = L.n_contigs, ht->min_votes = min_votes, ht->min_permille = min_permille;
	const size_t ns = (size_t)n_sites, nr = (size_t)cap_reads;
	hipError_t he = ht->begin(idx, device);
	ht->list.alloc(*ht, he, L);
	ht->alloc(he, (void**)&ht->d_block, ns * 4);
	ht->alloc(he, (void**)&ht->d_phase, ns);
	ht->alloc(he, (void**)&ht->blk, (size_t)ht->n_blocks * 16);
	ht->alloc(he, (void**)&ht->tag, nr * 12);
	ht->streams(he);
	if (he == hipSuccess) ht->votes = ht->tag + nr;
	ht->list.fill(he, L);
	if (he == hipSuccess && ns) he = hipMemcpy(ht->d_block, block, ns * 4, hipMemcpyHostToDevice);
	if (he == hipSuccess && ns) he = hipMemcpy(ht->d_phase, phase, ns, hipMemcpyHostToDevice);
	if (he != hipSuccess) {
		set_error("haplotag accumulator of %lld sites, %lld blocks, %lld reads: %s", (long long)n_sites, (long long)ht->n_blocks, (long long)cap_reads, hipGetErrorString(he));
		const int rc = Accum::failed(he);
		mnc_haplotag_free(ht);
		return rc;
	}
	if (int rc = mnc_haplotag_reset(ht)) { mnc_haplotag_free(ht); return rc; }
	*out = ht;
	return MNC_OK;
}

extern "C" int mnc_haplotag_reset(mnc_haplotag *ht)
{
	if (!ht) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(ht->device));
	std::lock_guard<std::mutex> g(ht->mu);
	if (ht->n_blocks) HIP_TRY(hipMemsetAsync(ht->blk, 0, (size_t)ht->n_blocks * 16, ht->st));
	HIP_TRY(hipMemsetAsync(ht->tag, 0xff, (size_t)ht->cap_reads * 4, ht->st));
	HIP_TRY(hipMemsetAsync(ht->votes, 0, (size_t)ht->cap_reads * 8, ht->st));
	HIP_TRY(ht->own_done());
	return MNC_OK;
}

extern "C" int mnc_haplotag_device_bytes(const mnc_haplotag *ht, int64_t *bytes) { return accum_device_bytes(ht, bytes); }

extern "C" int mnc_haplotag_n_blocks(const mnc_haplotag *ht, int64_t *n_blocks)
{
	if (!ht || !n_blocks) return MNC_ERR_ARG;
	*n_blocks = ht->n_blocks;
	return MNC_OK;
}

extern "C" int mnc_haplotag_device(mnc_haplotag *ht, const int32_t **d_blk, const int32_t **d_tag)
{
	if (!ht) return MNC_ERR_ARG;
	if (d_blk) *d_blk = ht->n_blocks ? ht->blk : nullptr;
	if (d_tag) *d_tag = ht->tag;
	return MNC_OK;
}

extern "C" int mnc_haplotag_fetch_blocks(mnc_haplotag *ht, int64_t first, int64_t n, int32_t *out)
{
	if (!ht) return MNC_ERR_ARG;
	if (first < 0 || n < 0 || first > ht->n_blocks || n > ht->n_blocks - first) {
		set_error("blocks [%lld, %lld) outside the %lld of the accumulator", (long long)first, (long long)(first + n), (long long)ht->n_blocks);
		return MNC_ERR_ARG;
	}
	if (n == 0) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(ht->device));
	return ht->finish(hipSuccess, nullptr, {out, ht->blk + first * 4, (size_t)n * 16}, {}, "haplotag blocks");
}

extern "C" int mnc_haplotag_fetch_tags(mnc_haplotag *ht, int64_t n_reads, int32_t *tag, int32_t *votes)
{
	if (!ht) return MNC_ERR_ARG;
	int64_t last = 0;
	{
		std::lock_guard<std::mutex> g(ht->mu);
		last = ht->last_reads;
	}
	if (n_reads != last) { set_error("tags of %lld reads asked for, the last add held %lld", (long long)n_reads, (long long)last); return MNC_ERR_ARG; }
	if (n_reads == 0) return MNC_OK;
	HIP_TRY(hipSetDevice(ht->device));
	return ht->finish(hipSuccess, nullptr, {tag, ht->tag, (size_t)n_reads * 4}, {votes, ht->votes, (size_t)n_reads * 8}, "haplotag tags");
}
