// Per-base pileup (include/monica_amd.h, "pileup"): what the reads say at each reference base -- allele counts, variants,
// consensus -- in an accumulator that lives across classify calls, added to from the last batch as it stands in HBM
// (regions, region CIGARs, the reads' bases, the contigs' 4-bit store).  The third consumer of that data after k_export.hip
// and k_coverage.hip, and made of their parts.  Runs only when asked for; nothing here is on the classification path.
//
// The planes.  Eight int32 words per reference base, each plane laid out as the coverage track is (base p of contig c is
// word off[c] + p):
//   track   [n_words]      depth DIFFERENCES of the M columns, exactly k_coverage.hip's track: two atomics per maximal run of
//                          M columns, the contig-end rule unchanged (cov_put)
//   alt     [7][n_words]   A C G T N DEL INS, channel-major.  Most columns match the reference, and a match costs nothing: an
//                          M column adds to its query base's channel only where it is not a reference match (a mismatch, a
//                          query N, any column over a reference N); a D adds to DEL for every base, an I to INS once, at the
//                          base on its left.  At 10 % errors that is a tenth of the atomics of one per column.
//   on read-out            count[b][p] = alt[b][p] + (ref[p] == b ? depth[p] - (alt[A] + alt[C] + alt[G] + alt[T] + alt[N])[p] : 0)
//
//   mnc_pile_add    one wave per READ, the records found and selected as mnc_cov_add_runs does.  A selected record's CIGAR
//                   is walked 64 operations at a time (prefix sums of the query and the reference lengths; the depth runs
//                   from two ballots as in k_coverage.hip), and the columns of a chunk 64 at a time with ONE LANE PER COLUMN:
//                   a lane finds its operation by bisecting the operations' inclusive column counts through cross-lane
//                   reads, as mnc_export_strings does -- except that an I operation counts as ONE column here: its lane
//                   counts it once.  An M lane fetches its two bases and, if they differ or the reference has an
//                   N, issues its one atomic.  What crosses a chunk border is scalar: the two offsets and "a run is open".
//                   The walk itself is pileup.h's pile_add_read; with the insertion store on, k_pile_ins.hip's
//                   mnc_pile_add_ins runs the same walk and also hands every I operation's bases to the allele table.
//   mnc_pile_scan   the read-outs, one pass over the tiles of scan.h with depth as a running sum (k_coverage.hip's summary:
//                   the plain sum G over the words minus G in front of the contig).  MODE 0 writes the eight planes, MODE 3
//                   the consensus; variants take MODE 1 (calls per tile), scan.h's exclusive scan over the tiles, and MODE 2
//                   (each tile places its records behind its offset by a prefix sum over its threads): compacted and in
//                   (contig, position, allele) order without a per-base offset array.
// With the strand store (mnc_pileup_store_strands) the add and the read-outs by strand are k_pile_strand.hip's; the read-outs
// here then see a nullable plane of masked columns (PileView::lowq) and nothing else of it.
#include <hip/hip_runtime.h>
#include <new>
#include <vector>
#include "pileup.h"

using namespace mnc;

using namespace mnc;

static_assert(sizeof(mnc_variant_t) == 20, "mnc_variant_t is 4 int32 and 4 bytes (monica_amd/_capi.py: VARIANT_DTYPE)");

namespace mnc {

__global__ __launch_bounds__(256) void mnc_pile_add(Batch B, int sel, const int64_t *off, int n_contigs, int64_t n_words, int32_t *track, int32_t *alt)
{
	pile_add_read<false>(B, sel, off, n_contigs, n_words, track, alt, InsTable{});
}

// ---------------------------------------------------------------- the engine's side (mnc_engine_add_pileup, engine.hip)
const Accum *as_accum(const mnc_pileup *pu) { return pu; }

// the batch B, as it stands in HBM, on the engine's stream `st`; nothing waits on the host
int pileup_add(mnc_pileup *pu, const Batch &B, int sel, hipStream_t st, const uint8_t *d_quals)
{
	if (B.n_reads == 0 || pu->n_words == 0) return MNC_OK;
	return pu->add(st, [&] {
		pu->added = true;
		if (pu->strands_on) pileup_add_strands_launch(pu, B, sel, st, d_quals);
		else if (pu->ins_on) pileup_add_ins_launch(pu, B, sel, st);
		else
			hipLaunchKernelGGL(mnc_pile_add, dim3((B.n_reads + 3) / 4), dim3(256), 0, st, B, sel, pu->d_off, pu->n_contigs, pu->n_words, pu->track, pu->alt);
	});
}

} // namespace mnc

// ---------------------------------------------------------------- C-ABI
extern "C" void mnc_pileup_free(mnc_pileup *pu)
{
	if (!pu) return;
	pu->release();
	delete pu;
}

extern "C" int mnc_pileup_create(mnc_index *idx, int device, mnc_pileup **out)
{
	if (!idx || !out) return MNC_ERR_ARG;
	*out = nullptr;
	if (int rc = check_device(device)) return rc;
	if (idx->seq_off.size() != idx->contig_len.size() + 1) { set_error("the index holds no contig bases"); return MNC_ERR_ARG; }
	mnc_pileup *pu = new (std::nothrow) mnc_pileup;
	if (!pu) return MNC_ERR_NOMEM;
	pu->n_contigs = (int)idx->contig_len.size();
	try {
		pu->off.assign(idx->seq_off.begin(), idx->seq_off.end());   // the planes' layout is the 4-bit store's
	} catch (const std::bad_alloc &) { delete pu; return MNC_ERR_NOMEM; }
	pu->n_words = pu->off[pu->n_contigs];
	if (int rc = index_upload(idx, device, &pu->didx)) { delete pu; return rc; }
	const size_t nc = (size_t)pu->n_contigs, nw = (size_t)pu->n_words, nt = nw / SC_TILE + 2;
	hipError_t he = pu->begin(idx, device);
	pu->alloc(he, (void**)&pu->track, nw * 4);
	pu->alloc(he, (void**)&pu->alt, nw * 4 * PILE_ALT);
	pu->alloc(he, (void**)&pu->d_off, (nc + 1) * 8);
	pu->alloc(he, (void**)&pu->cbase, nc * 8);
	pu->alloc(he, (void**)&pu->tile_sums, nt * 8);
	pu->alloc(he, (void**)&pu->tile_cnt, nt * 8);
	pu->alloc(he, (void**)&pu->tile_voff, nt * 8);
	pu->alloc(he, (void**)&pu->sums2, (nt / SC_TILE + 2) * 8);
	pu->streams(he);
	if (he == hipSuccess) he = hipMemcpy(pu->d_off, pu->off.data(), (nc + 1) * 8, hipMemcpyHostToDevice);
	if (he != hipSuccess) {
		set_error("pileup accumulator of %lld bases (32 bytes each; 72 with the strand store): %s", (long long)pu->n_words, hipGetErrorString(he));
		const int rc = Accum::failed(he);
		mnc_pileup_free(pu);
		return rc;
	}
	if (int rc = mnc_pileup_reset(pu)) { mnc_pileup_free(pu); return rc; }
	*out = pu;
	return MNC_OK;
}

extern "C" int mnc_pileup_reset(mnc_pileup *pu)
{
	if (!pu) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(pu->device));
	std::lock_guard<std::mutex> lk(pu->mu);
	if (pu->n_words) {
		HIP_TRY(hipMemsetAsync(pu->track, 0, (size_t)pu->n_words * 4, pu->st));
		HIP_TRY(hipMemsetAsync(pu->alt, 0, (size_t)pu->n_words * 4 * PILE_ALT, pu->st));
	}
	if (pu->ins_on) HIP_TRY(ins_clear(pu));
	if (pu->strands_on) HIP_TRY(strands_clear(pu));
	HIP_TRY(pu->own_done());
	return MNC_OK;
}

extern "C" int mnc_pileup_device_bytes(const mnc_pileup *pu, int64_t *bytes) { return accum_device_bytes(pu, bytes); }

extern "C" int mnc_pileup_device(mnc_pileup *pu, const int32_t **d_depth, const int32_t **d_alt, int64_t *n_words)
{
	if (!pu) return MNC_ERR_ARG;
	if (d_depth) *d_depth = pu->n_words ? pu->track : nullptr;
	if (d_alt) *d_alt = pu->n_words ? pu->alt : nullptr;
	if (n_words) *n_words = pu->n_words;
	return MNC_OK;
}

extern "C" int mnc_pileup_fetch_counts(mnc_pileup *pu, int rid, int64_t start, int64_t end, int32_t *out)
{
	if (!pu) return MNC_ERR_ARG;
	if (int rc = accum_interval(pu->off, rid, start, end)) return rc;
	if (end == start) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(pu->device));
	const size_t bytes = (size_t)(end - start) * 4 * MNC_PILE_PLANES;
	int32_t *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, bytes));
	pile_tile_sums(pu, pu->off[rid], end, false);               // the contig's words up to `end`: the sum starts at the contig
	pile_launch<0>(pu, pu->off[rid], end, false, rid, start, PileThr{0, 0, 0}, tmp, nullptr, 0, nullptr);
	return pu->finish(hipSuccess, tmp, {out, tmp, bytes}, {}, "pileup counts");
}

extern "C" int mnc_pileup_consensus(mnc_pileup *pu, int rid, int64_t start, int64_t end, int32_t min_depth, char *out)
{
	if (!pu) return MNC_ERR_ARG;
	if (int rc = accum_interval(pu->off, rid, start, end)) return rc;
	if (end == start) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(pu->device));
	char *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, (size_t)(end - start)));
	pile_tile_sums(pu, pu->off[rid], end, false);
	pile_launch<3>(pu, pu->off[rid], end, false, rid, start, PileThr{min_depth, 0, 0}, nullptr, nullptr, 0, tmp);
	return pu->finish(hipSuccess, tmp, {out, tmp, (size_t)(end - start)}, {}, "pileup consensus");
}

extern "C" int mnc_pileup_call_variants(mnc_pileup *pu, int rid, int32_t min_depth, int32_t min_count, int32_t min_permille, mnc_variant_t *out, int64_t cap, int64_t *n)
{
	if (!pu || !n) return MNC_ERR_ARG;
	*n = 0;
	if (rid < -1 || rid >= pu->n_contigs) { set_error("contig %d out of range", rid); return MNC_ERR_ARG; }
	const bool all = rid < 0;
	const int64_t w0 = all ? 0 : pu->off[rid], len = all ? pu->n_words : pu->off[rid + 1] - w0;
	if (len == 0) return MNC_OK;
	HIP_TRY(hipSetDevice(pu->device));
	const PileThr thr{min_depth, min_count, min_permille};
	const int64_t nb = (len + SC_TILE - 1) / SC_TILE;
	// ---- count, scan
	pile_tile_sums(pu, w0, len, all);
	pile_launch<1>(pu, w0, len, all, rid, 0, thr, nullptr, nullptr, 0, nullptr);
	exclusive_scan(ScanInPlain<int64_t>{pu->tile_cnt}, nb, pu->tile_voff, pu->sums2, pu->st);
	HIP_TRY(hipGetLastError());
	int64_t total = 0;
	HIP_TRY(hipMemcpyAsync(&total, pu->tile_voff + nb, 8, hipMemcpyDeviceToHost, pu->st));
	HIP_TRY(hipStreamSynchronize(pu->st));
	*n = total;
	if (cap < total) { set_error("%lld variants, room for %lld", (long long)total, (long long)cap); return MNC_ERR_RANGE; }
	if (total == 0) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	// ---- write (read-outs are for one thread at a time; should an add slip in between the passes all the same, no tile
	// writes beyond `total`)
	mnc_variant_t *tmp = nullptr;
	HIP_TRY(hipMalloc((void**)&tmp, (size_t)total * sizeof(mnc_variant_t)));
	pile_launch<2>(pu, w0, len, all, rid, 0, thr, nullptr, tmp, total, nullptr);
	return pu->finish(hipSuccess, tmp, {out, tmp, (size_t)total * sizeof(mnc_variant_t)}, {}, "pileup variants");
}
