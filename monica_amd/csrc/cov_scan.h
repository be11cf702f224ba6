// The launches in front of a read-out's pass over a depth-difference track (k_coverage.hip, k_pileup.hip).  Apart from
// cov_common.h, so that a unit that wants the selectors alone (k_abundance.hip) instantiates no scan kernel.
#pragma once

#include "cov_common.h"

namespace mnc {

// tile sums of track[0 .. n) (exclusive, in place) and, where track is the whole track of n_contigs contigs (cbase given),
// the sum in front of every contig
static void cov_tile_sums(const int32_t *track, int64_t n, int64_t *tile_sums, const int64_t *d_off, int n_contigs, long long *cbase, hipStream_t st)
{
	const int64_t nb = (n + SC_TILE - 1) / SC_TILE;
	hipLaunchKernelGGL(mnc_scan_reduce<ScanInPlain<int32_t>>, dim3((unsigned)nb), dim3(SC_THREADS), 0, st, ScanInPlain<int32_t>{track}, n, tile_sums);
	hipLaunchKernelGGL(mnc_scan_sums, dim3(1), dim3(64), 0, st, tile_sums, nb);
	if (cbase) hipLaunchKernelGGL(mnc_cov_contig_base, dim3((unsigned)((n_contigs + 3) / 4)), dim3(256), 0, st, track, d_off, n_contigs, tile_sums, cbase);
}

} // namespace mnc
