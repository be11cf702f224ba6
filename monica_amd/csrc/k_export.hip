// Alignment records of a whole batch (mnc_engine_export_alignments): what index.map() yields per hit -- positions,
// strand, scores, the CIGAR and, on request, minimap2's cs (short form) and MD strings -- made on the device from the last
// batch as it stands in HBM.  Runs only when asked for; nothing here is on the classification path.
//
//   mnc_export_records   one lane per record: the live region slots of every read (reg_slot(r) .. + n_reg[r]) squeezed
//                        into the dense record array, the read found by bisection of the scanned n_reg
//   mnc_export_strings   one wave per record, twice: a COUNT pass (string lengths; the engine scans them, so the pools are
//                        sized exactly) and a WRITE pass (CIGAR words and string bytes to their scanned places)
//
// The strings.  A region's CIGAR is walked 64 operations at a time (one lane each; base offsets by prefix sums, as the
// stitch kernel does), and the columns of those operations 64 at a time, ONE LANE PER COLUMN: a lane finds its operation by
// bisecting the operations' inclusive column counts through cross-lane reads, fetches its two bases (query on the hit's
// strand, target from the 4-bit contig store) and classifies its column.  What is left is tokenisation -- match runs
// become decimal numbers of varying width -- and that is done across the wave, not by a loop over bases:
//   break flags     ballots of "this column is not a match", "this match starts an operation" (cs: a run ends with its M
//                   operation), "this column resets MD's counter" (a mismatch or a deleted base)
//   run lengths     a lane that closes a run looks for the highest break below it in the ballot mask (one clz) and counts
//                   the matches in between (one popcount); a run that began before the 64 columns at hand adds a carried
//                   scalar -- for MD across insertions and across CIGAR chunks, for cs within its M operation
//   byte offsets    inclusive prefix sum of the lanes' token widths (0 for a column inside a run) on top of a running base
// Neighbouring lanes write neighbouring bytes, so the pool writes of a wave are one contiguous stretch per step.
//
// Strand: mnc_reg_t.qs / qe are forward-strand read coordinates; the alignment ran on the hit's strand, i.e. for rev = 1 on
// the reverse complement, where the region starts at qlen - qe.  Column p of the query side is therefore read base
// qs + p for rev = 0 and the complement of read base qe - 1 - p for rev = 1 -- what mm_write_cs / write_MD build as qseq.
#include <hip/hip_runtime.h>
#include "device.h"
#include "scan.h"

namespace mnc {

static_assert(sizeof(mnc_aln_t) == 104, "mnc_aln_t is 18 int32, 3 int64, 2 int32 without padding (monica_amd/_capi.py: ALN_DTYPE)");

__device__ __forceinline__ int ex_incl_add(int x)
{
	const int lane = lane_id();
	for (int d = 1; d < 64; d <<= 1) {
		const int o = __shfl_up(x, d);
		if (lane >= d) x += o;
	}
	return x;
}

__device__ __forceinline__ int ex_digits(int x)
{
	return x < 10 ? 1 : x < 100 ? 2 : x < 1000 ? 3 : x < 10000 ? 4 : x < 100000 ? 5 : x < 1000000 ? 6 : x < 10000000 ? 7 : x < 100000000 ? 8 : x < 1000000000 ? 9 : 10;
}

// bytes [at, at + nd) of a string of `cap` bytes: the decimal form of x
__device__ __forceinline__ void ex_put_num(char *s, int at, int cap, int x, int nd)
{
	for (int k = nd - 1; k >= 0; --k) {
		if (at + k < cap) s[at + k] = (char)('0' + x % 10);
		x /= 10;
	}
}

__device__ __forceinline__ void ex_put(char *s, int at, int cap, char c) { if (at >= 0 && at < cap) s[at] = c; }

__global__ __launch_bounds__(256) void mnc_export_records(Batch B, const int64_t *aln_off, mnc_aln_t *alns, int64_t n_aln)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_aln) return;
	// the read: the last r with aln_off[r] <= i (reads without regions repeat their neighbour's offset)
	uint32_t lo = 0, hi = B.n_reads;                           // aln_off[lo] <= i < aln_off[hi]
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (aln_off[mid] <= i) lo = mid; else hi = mid;
	}
	const uint32_t rd = lo;
	const int64_t slot = reg_slot(B, rd) + (i - aln_off[rd]);
	const mnc_reg_t r = B.regs[slot];
	const bool dp = B.contract == MNC_CONTRACT_DP;
	mnc_aln_t a;
	a.read = (int32_t)rd, a.rid = r.rid, a.rev = r.rev;
	a.qs = r.qs, a.qe = r.qe, a.rs = r.rs, a.re = r.re;
	a.mapq = r.mapq, a.mlen = r.mlen, a.blen = r.blen, a.nm = r.blen - r.mlen + r.n_ambi;
	a.score = r.score, a.cnt = r.cnt;
	a.dp_score = r.dp_score, a.dp_max = r.dp_max, a.n_ambi = r.n_ambi;
	const int primary = r.id == r.parent;
	a.flags = primary | ((primary && r.mapq >= B.min_mapq) ? 2 : 0) | (int32_t)((uint32_t)r.flags << 8);
	a.n_cigar = dp && r.n_cigar > 0 ? r.n_cigar : 0;
	a.cigar_off = a.n_cigar ? B.regdp[slot].cig_off : 0;       // for now: where the words are in the region pool (mnc_export_strings<true> puts the record's own offset)
	a.cs_off = a.md_off = 0, a.cs_len = a.md_len = 0;
	alns[i] = a;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void mnc_export_strings(Batch B, mnc_aln_t *alns, int64_t n_aln, const int64_t *cig_off, const int64_t *cs_off,
                                                          const int64_t *md_off, uint32_t *cigar, char *cs_pool, char *md_pool, int what)
{
	const int lane = lane_id();
	const int64_t rec = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (rec >= n_aln) return;                                  // (whole waves; the kernel has no workgroup barrier)
	const mnc_aln_t a = alns[rec];
	const int n_c = a.n_cigar;
	const uint32_t *src = B.cig_reg + a.cigar_off;             // (read only when n_c > 0)
	const bool want_cs = (what & MNC_ALN_CS) != 0, want_md = (what & MNC_ALN_MD) != 0;
	const int64_t dst_c = WRITE ? cig_off[rec] : 0, dst_cs = WRITE && want_cs ? cs_off[rec] : 0, dst_md = WRITE && want_md ? md_off[rec] : 0;
	char *cs = cs_pool + dst_cs, *md = md_pool + dst_md;
	const int cs_cap = WRITE ? a.cs_len : 0, md_cap = WRITE ? a.md_len : 0;
	// the two sequences: read bytes (clamped to the read), contig codes (clamped to the contig)
	const int64_t read_off = B.offsets[a.read];
	const int qlen = (int)(B.offsets[a.read + 1] - read_off);
	const uint8_t *read = B.bases + read_off;
	const int64_t coff = B.seq_off ? B.seq_off[a.rid] : 0;
	const int tlen = B.seq_off ? (int)(B.seq_off[a.rid + 1] - coff) : 0;
	auto Q = [&](int p) -> int {                               // column p of the query side, on the hit's strand
		int at = a.rev ? a.qe - 1 - p : a.qs + p;
		at = at < 0 ? 0 : at >= qlen ? qlen - 1 : at;
		const int c = base_nt4(read[at]);
		return a.rev ? (c < 4 ? 3 - c : 4) : c;
	};
	auto T = [&](int p) -> int {
		int at = a.rs + p;
		at = at < 0 ? 0 : at >= tlen ? tlen - 1 : at;
		const int64_t o = coff + at;
		const int c = (int)(B.seq4[o >> 3] >> ((o & 7) * 4) & 15u);
		return c < 4 ? c : 4;
	};
	int qoff = 0, toff = 0;                                    // bases of the region before the chunk at hand
	int cs_at = 0, md_at = 0;                                  // bytes so far
	int carry_cs = 0, carry_md = 0;                            // matches of the open run before the columns at hand
	const bool strings = (want_cs || want_md) && n_c > 0 && qlen > 0 && tlen > 0;
	for (int k0 = 0; k0 < n_c; k0 += 64) {
		const int k = k0 + lane;
		const uint32_t wd = k < n_c ? src[k] : 0u;
		if (WRITE && k < n_c) cigar[dst_c + k] = wd;
		if (!strings) continue;
		const int op = (int)(wd & 0xfu);
		const int len = k < n_c && op <= 2 ? (int)(wd >> 4) : 0;
		const int dq = op != 2 ? len : 0, dt = op != 1 ? len : 0;
		const int iq = ex_incl_add(dq), it = ex_incl_add(dt), ie = ex_incl_add(len);
		const int total = __shfl(ie, 63);
		const int my_q0 = qoff + iq - dq, my_t0 = toff + it - dt;
		for (int c0 = 0; c0 < total; c0 += 64) {
			const bool valid = c0 + lane < total;
			const int c = valid ? c0 + lane : total - 1;
			// this column's operation: the first one whose inclusive column count exceeds c
			int o = 0;
			for (int step = 32; step > 0; step >>= 1) {
				const int e = __shfl(ie, o + step - 1);
				if (e <= c) o += step;
			}
			const int o_end = __shfl(ie, o), o_len = __shfl(len, o), o_op = __shfl(op, o);
			const int q0 = __shfl(my_q0, o), t0 = __shfl(my_t0, o);
			const int x = c - (o_end - o_len);                    // column within the operation
			const bool is_M = valid && o_op == 0, is_I = valid && o_op == 1, is_D = valid && o_op == 2;
			const int qc = o_op != 2 ? Q(q0 + x) : 4, tc = o_op != 1 ? T(t0 + x) : 4;
			const bool match = is_M && qc == tc, mism = is_M && qc != tc;
			const unsigned long long lt = (1ull << lane) - 1ull, le = lt | 1ull << lane;
			const unsigned long long m_match = __ballot(match);
			int w_cs = 0, w_md = 0, run = 0, l = 0;
			bool cs_close = false;
			if (want_cs) {
				// a run ends with its operation or before a mismatch (the next column of the same operation, read here: the lane
				// that holds it may be in the next 64)
				cs_close = match && (x == o_len - 1 || Q(q0 + x + 1) != T(t0 + x + 1));
				const unsigned long long m_non = __ballot(valid && !match), m_first = __ballot(match && x == 0);
				const unsigned long long s = m_non & lt, b = m_first & le;
				const int hs = s ? 63 - __clzll((long long)s) : -1, hb = b ? 63 - __clzll((long long)b) : -1;
				const int start = hs + 1 > hb ? hs + 1 : hb;
				run = hs < 0 && hb < 0 ? lane + 1 + carry_cs : lane - start + 1;
				w_cs = cs_close ? 1 + ex_digits(run) : mism ? 3 : (is_I || is_D) ? (x == 0 ? 2 : 1) : 0;
			}
			if (want_md) {
				const unsigned long long m_reset = __ballot(mism || is_D);
				const unsigned long long r = m_reset & lt;
				if (r) {
					const int h = 63 - __clzll((long long)r);
					l = __popcll(m_match & lt & ~((2ull << h) - 1ull));
				} else l = __popcll(m_match & lt) + carry_md;
				w_md = mism ? ex_digits(l) + 1 : is_D ? (x == 0 ? ex_digits(l) + 2 : 1) : 0;
				if (m_reset) {
					const int h = 63 - __clzll((long long)m_reset);
					carry_md = __popcll(m_match & ~((2ull << h) - 1ull));
				} else carry_md += __popcll(m_match);
			}
			if (want_cs) {
				const int inc = ex_incl_add(w_cs);
				if (WRITE) {
					const int at = cs_at + inc - w_cs;
					if (cs_close) ex_put(cs, at, cs_cap, ':'), ex_put_num(cs, at + 1, cs_cap, run, w_cs - 1);
					else if (mism) ex_put(cs, at, cs_cap, '*'), ex_put(cs, at + 1, cs_cap, "acgtn"[tc]), ex_put(cs, at + 2, cs_cap, "acgtn"[qc]);
					else if (is_I || is_D) {
						if (x == 0) ex_put(cs, at, cs_cap, is_I ? '+' : '-');
						ex_put(cs, at + w_cs - 1, cs_cap, "acgtn"[is_I ? qc : tc]);
					}
				}
				cs_at += __shfl(inc, 63);
				// the run the last column leaves open (it goes on in the same M operation)
				const int last = total - c0 < 64 ? total - c0 - 1 : 63;
				carry_cs = __shfl(match && !cs_close ? run : 0, last);
			}
			if (want_md) {
				const int inc = ex_incl_add(w_md);
				if (WRITE) {
					const int at = md_at + inc - w_md;
					if (mism) ex_put_num(md, at, md_cap, l, w_md - 1), ex_put(md, at + w_md - 1, md_cap, "ACGTN"[tc]);
					else if (is_D) {
						if (x == 0) ex_put_num(md, at, md_cap, l, w_md - 2), ex_put(md, at + w_md - 2, md_cap, '^');
						ex_put(md, at + w_md - 1, md_cap, "ACGTN"[tc]);
					}
				}
				md_at += __shfl(inc, 63);
			}
		}
		qoff += __shfl(iq, 63), toff += __shfl(it, 63);
	}
	if (strings && want_md && carry_md > 0) {                  // MD's last run
		const int nd = ex_digits(carry_md);
		if (WRITE && lane == 0) ex_put_num(md, md_at, md_cap, carry_md, nd);
		md_at += nd;
	}
	if (lane == 0) {
		if (WRITE) alns[rec].cigar_off = dst_c, alns[rec].cs_off = dst_cs, alns[rec].md_off = dst_md;
		else alns[rec].cs_len = cs_at, alns[rec].md_len = md_at;
	}
}

// ---------------------------------------------------------------- launches
struct ScanInAln {
	const mnc_aln_t *a;
	int field;                                                 // 0 n_cigar, 1 cs_len, 2 md_len
	__device__ long long operator()(int64_t i) const { return field == 0 ? a[i].n_cigar : field == 1 ? a[i].cs_len : a[i].md_len; }
};

void launch_export_records(const Batch &B, const int64_t *aln_off, mnc_aln_t *alns, int64_t n_aln, hipStream_t st)
{
	if (n_aln <= 0) return;
	hipLaunchKernelGGL(mnc_export_records, dim3((unsigned)((n_aln + 255) / 256)), dim3(256), 0, st, B, aln_off, alns, n_aln);
}

void launch_export_scan(const mnc_aln_t *alns, int64_t n_aln, int field, int64_t *out, int64_t *sums, hipStream_t st)
{
	exclusive_scan(ScanInAln{alns, field}, n_aln, out, sums, st);
}

void launch_export_strings(const Batch &B, bool write, mnc_aln_t *alns, int64_t n_aln, const int64_t *cig_off, const int64_t *cs_off,
                           const int64_t *md_off, uint32_t *cigar, char *cs, char *md, int what, hipStream_t st)
{
	if (n_aln <= 0) return;
	const dim3 grid((unsigned)((n_aln + 3) / 4)), block(256);
	if (write) hipLaunchKernelGGL(mnc_export_strings<true>, grid, block, 0, st, B, alns, n_aln, cig_off, cs_off, md_off, cigar, cs, md, what);
	else hipLaunchKernelGGL(mnc_export_strings<false>, grid, block, 0, st, B, alns, n_aln, cig_off, cs_off, md_off, cigar, cs, md, what);
}

} // namespace mnc
