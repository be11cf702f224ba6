// The insertion store of a pileup (include/monica_amd.h, "pileup": insertion alleles; pile_ins.h: the table, the hashes,
// the claim): the add kernels that fill it, its read-outs and its C-ABI.  The planes, and a pileup without the store, are
// k_pileup.hip's; the walk of a read's records is shared (pileup.h).
//   mnc_pile_add_ins   mnc_pile_add's walk with the store on: the lane of an I column also hands the operation's bases to
//                      the allele table -- the short ones itself, the long ones with the whole wave
//   mnc_pile_add_list  a caller's alleles through the same routes, a lane per row
#include <hip/hip_runtime.h>
#include <algorithm>
#include <new>
#include <vector>
#include "pileup.h"

using namespace mnc;

static_assert(sizeof(mnc_insertion_t) == 32, "mnc_insertion_t is 6 int32 and an int64 (monica_amd/_capi.py: INSERTION_DTYPE)");

namespace mnc {

__global__ __launch_bounds__(256) void mnc_pile_add_ins(Batch B, int sel, const int64_t *off, int n_contigs, int64_t n_words, int32_t *track, int32_t *alt, InsTable T)
{
	pile_add_read<true>(B, sel, off, n_contigs, n_words, track, alt, T);
}

// alleles made by the caller (mnc_pileup_add_insertion_list), already checked: one wave takes 64 rows, a lane its row,
// through the same short and long routes.  The bases are ASCII, on the hit's strand as given.
__global__ __launch_bounds__(256) void mnc_pile_add_list(InsTable T, int64_t n, const int64_t *place, const int32_t *len, const int32_t *count, const int64_t *base_off,
                                                         const uint8_t *bases)
{
	const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool have = row < n;                                // (whole waves go on: ins_wave_add is the wave's)
	int claims = 0;
	ins_wave_add(T, have, have ? place[row] : 0, have ? len[row] : 0, have ? count[row] : 0, have ? (long long)base_off[row] : 0,
	             [&](long long s, int j) { return base_nt4(bases[s + j]); }, ins_full(T), claims);
	ins_flush(T, claims);
}

// ---------------------------------------------------------------- read-outs of the insertion store
// All of them walk the slots with one thread per slot; stream order has put them behind the adds, so a slot whose
// fingerprint is set has its payload.  The order of what they hand out is made here and owes nothing to the slots:
//   mnc_ins_info     the totals, and the collision check of every slot: sum == count * h2(payload) mod 2^64
//   MODE 4 above     span per base of the range, -1 where nothing may be called
//   mnc_ins_select   <0> counts the selected alleles per base (and their bases in all), scan.h turns the counts into every
//                    base's segment, <1> scatters the slots into the segments
//   mnc_ins_sort     one thread per base sorts a segment of two or more by (length, bases): the segments are small
//   mnc_ins_write    the records and their bases, behind scan.h's offsets over the records' lengths
//   mnc_ins_best / mnc_ins_cons_write   the consensus: per base the first allele of the largest count and the output length,
//                    scan.h, one write pass
enum { IR_ALLELES, IR_EVENTS, IR_POOL_BASES, IR_COLLISIONS, IR_CTR, IR_N = IR_CTR + INC_N };
struct InsRule { int cons, min_count, min_permille; };        // cons: 2 * count > span; otherwise the rule of the variants

__global__ __launch_bounds__(256) void mnc_ins_info(InsTable T, unsigned long long *res)
{
	unsigned long long v[IR_CTR] = {0, 0, 0, 0};
	for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < T.slots; s += (int64_t)gridDim.x * blockDim.x) {
		if (!T.fp[s]) continue;
		const int64_t place = T.place[s];
		const uint32_t lw = T.len[s];
		const unsigned long long cnt = (unsigned long long)(unsigned)T.count[s];
		++v[IR_ALLELES], v[IR_EVENTS] += cnt;
		if (lw & INS_NOBASES) continue;                          // (no bases to check the sum against)
		const int len = (int)(lw & INS_LEN);
		if (lw & INS_POOLED) v[IR_POOL_BASES] += 2ull * (unsigned long long)((len + 1) / 2);
		const unsigned long long pay = T.pay[s];
		unsigned long long s2 = 0;
		for (int j = 0; j < len; ++j) s2 += ins_mix2(j, ins_base(T, lw, pay, j));
		if (T.sum[s] != cnt * ins_h2(place, len, s2)) ++v[IR_COLLISIONS];
	}
	for (int k = 0; k < IR_CTR; ++k) {
		const unsigned long long x = ins_wave_sum(v[k]);
		if (lane_id() == 0 && x) (void)__hip_atomic_fetch_add(res + k, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	if (blockIdx.x == 0 && threadIdx.x < INC_N) res[IR_CTR + threadIdx.x] = T.ctr[threadIdx.x];
}

// the index within [g0, g0 + m) of the base that slot s's allele is selected at, or -1
__device__ __forceinline__ int64_t ins_selected(const InsTable &T, int64_t s, int64_t g0, int64_t m, const int32_t *spanq, const InsRule &rule)
{
	if (!T.fp[s]) return -1;
	const int64_t place = T.place[s];
	if (place < g0 || place >= g0 + m) return -1;
	const long long span = spanq[place - g0], c = T.count[s];
	if (span < 0) return -1;
	const bool yes = rule.cons ? 2 * c > span : c >= rule.min_count && c * 1000 >= (long long)rule.min_permille * span;
	return yes ? place - g0 : -1;
}

template <int PASS>
__global__ __launch_bounds__(256) void mnc_ins_select(InsTable T, int64_t g0, int64_t m, const int32_t *spanq, InsRule rule, int32_t *cnt, const int64_t *offs, int64_t *sel,
                                                      unsigned long long *n_bases)
{
	unsigned long long nb = 0;
	for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < T.slots; s += (int64_t)gridDim.x * blockDim.x) {
		const int64_t i = ins_selected(T, s, g0, m, spanq, rule);
		if (i < 0) continue;
		if (PASS == 0) {
			(void)__hip_atomic_fetch_add(cnt + i, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			nb += T.len[s] & INS_LEN;
		} else {                                                  // any place of the base's segment: the sort makes the order
			const int k = __hip_atomic_fetch_add(cnt + i, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
			if (k >= 0 && offs[i] + k < offs[i + 1]) sel[offs[i] + k] = s;
		}
	}
	if (PASS == 0) {                                            // (every thread is here again: one atomic a wave)
		nb = ins_wave_sum(nb);
		if (lane_id() == 0 && nb) (void)__hip_atomic_fetch_add(n_bases, nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// (length, bases) of slot a before those of slot b; the bases as codes A < C < G < T < N
__device__ __forceinline__ bool ins_before(const InsTable &T, int64_t a, int64_t b)
{
	const uint32_t la = T.len[a], lb = T.len[b];
	const int na = (int)(la & INS_LEN), nb = (int)(lb & INS_LEN);
	if (na != nb) return na < nb;
	if ((la | lb) & INS_NOBASES) return a < b;                   // (no read-out that orders runs while there is one)
	const unsigned long long pa = T.pay[a], pb = T.pay[b];
	for (int j = 0; j < na; ++j) {
		const int ca = ins_base(T, la, pa, j), cb = ins_base(T, lb, pb, j);
		if (ca != cb) return ca < cb;
	}
	return false;
}

__global__ __launch_bounds__(256) void mnc_ins_sort(InsTable T, int64_t m, const int64_t *offs, int64_t *sel)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= m) return;
	const int64_t lo = offs[i], hi = offs[i + 1];
	for (int64_t k = lo; k < hi; ++k) if (sel[k] < 0) return;       // (a place left empty by an add between the passes: see ins_order)
	for (int64_t k = lo + 1; k < hi; ++k) {                       // insertion sort
		const int64_t x = sel[k];
		int64_t j = k;
		for (; j > lo && ins_before(T, x, sel[j - 1]); --j) sel[j] = sel[j - 1];
		sel[j] = x;
	}
}

struct InsLenIn {                                              // scan.h's input: the length of the k-th selected allele
	const uint32_t *len;
	const int64_t *sel;
	__device__ long long operator()(int64_t k) const { return sel[k] < 0 ? 0 : (long long)(len[sel[k]] & INS_LEN); }
};

__device__ __forceinline__ void ins_put_bases(const InsTable &T, int64_t s, char *out, const char *letters)
{
	const uint32_t lw = T.len[s];
	const unsigned long long pay = T.pay[s];
	const int len = (int)(lw & INS_LEN);
	for (int j = 0; j < len; ++j) {
		const int c = ins_base(T, lw, pay, j);
		out[j] = letters[c < 4 ? c : 4];
	}
}

__global__ __launch_bounds__(256) void mnc_ins_write(InsTable T, int64_t total, const int64_t *sel, const int64_t *boff, const int32_t *spanq, int64_t g0, const int64_t *off,
                                                     int n_contigs, mnc_insertion_t *out, char *bases)
{
	const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= total) return;
	const int64_t s = sel[k];
	if (s < 0) { out[k] = mnc_insertion_t{-1, 0, 0, 0, 0, 0, boff[k]}; return; }
	const int64_t place = T.place[s];
	int lo = 0, hi = n_contigs;                                 // the contig: the last c with off[c] <= place
	while (hi - lo > 1) {
		const int mid = lo + (hi - lo) / 2;
		if (off[mid] <= place) lo = mid; else hi = mid;
	}
	mnc_insertion_t r;
	r.rid = lo, r.pos = (int32_t)(place - off[lo]), r.span = spanq[place - g0], r.count = T.count[s], r.len = (int32_t)(T.len[s] & INS_LEN), r.pad = 0;
	r.base_off = boff[k];
	out[k] = r;
	ins_put_bases(T, s, bases + boff[k], "ACGTN");
}

// per base of the range: the slot of the first allele (in segment order) of the largest count, or -1, and the characters
// the base writes -- itself and that allele's bases
__global__ __launch_bounds__(256) void mnc_ins_best(InsTable T, int64_t m, const int64_t *offs, const int64_t *sel, int64_t *best, int32_t *out_len)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= m) return;
	int64_t b = -1;
	int top = 0;
	for (int64_t k = offs[i]; k < offs[i + 1]; ++k) {
		const int c = sel[k] < 0 ? 0 : T.count[sel[k]];
		if (c > top) top = c, b = sel[k];
	}
	best[i] = b;
	out_len[i] = 1 + (b >= 0 ? (int)(T.len[b] & INS_LEN) : 0);
}

__global__ __launch_bounds__(256) void mnc_ins_cons_write(InsTable T, int64_t m, const char *cons, const int64_t *best, const int64_t *ooff, char *out)
{
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= m) return;
	out[ooff[i]] = cons[i];
	if (best[i] >= 0) ins_put_bases(T, best[i], out + ooff[i] + 1, "acgtn");
}

static unsigned ins_grid(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 1 << 16); }

// clears the table (the payloads are behind the fingerprints: they need no clearing); on `st`
hipError_t ins_clear(mnc_pileup *pu)
{
	const InsTable &T = pu->ins;
	hipError_t he = hipMemsetAsync(T.fp, 0, (size_t)T.slots * 8, pu->st);
	if (he == hipSuccess) he = hipMemsetAsync(T.sum, 0, (size_t)T.slots * 8, pu->st);
	if (he == hipSuccess) he = hipMemsetAsync(T.count, 0, (size_t)T.slots * 4, pu->st);
	if (he == hipSuccess) he = hipMemsetAsync(T.ctr, 0, INC_N * 8, pu->st);
	return he;
}

// the totals of the store, on the host (waits for the work queued so far)
static int ins_totals(mnc_pileup *pu, unsigned long long r[IR_N])
{
	if (!pu->ins_on) { set_error("the pileup stores no insertions (mnc_pileup_store_insertions was not called)"); return MNC_ERR_ARG; }
	HIP_TRY(hipSetDevice(pu->device));
	unsigned long long *d = nullptr;
	HIP_TRY(hipMalloc((void**)&d, IR_N * 8));
	const hipError_t he = hipMemsetAsync(d, 0, IR_N * 8, pu->st);       // (finish frees d whatever he is)
	if (he == hipSuccess) hipLaunchKernelGGL(mnc_ins_info, dim3(ins_grid(pu->ins.slots)), dim3(256), 0, pu->st, pu->ins, d);
	return pu->finish(he, d, {r, d, IR_N * 8}, {}, "insertion totals");
}

// what every read-out but the info call begins with: MNC_ERR_RANGE while an event was dropped (which one depends on the
// order of arrival), two alleles share a fingerprint, or -- for a read-out that hands out bases -- an allele has none
static int ins_readable(mnc_pileup *pu)
{
	unsigned long long r[IR_N];
	if (int rc = ins_totals(pu, r)) return rc;
	const unsigned long long dropped = r[IR_CTR + INC_DROPPED];
	if (dropped) { set_error("%llu insertion(s) found no slot among cap_alleles = %lld: reset and add again with more room", dropped, (long long)pu->ins.cap_alleles); return MNC_ERR_RANGE; }
	if (r[IR_CTR + INC_POOL_DROPPED]) { set_error("the bases of %llu allele(s) did not fit the pool of %lld bytes", r[IR_CTR + INC_POOL_DROPPED], (long long)pu->ins.pool_bytes); return MNC_ERR_RANGE; }
	if (r[IR_COLLISIONS]) { set_error("%llu slot(s) hold two alleles of one fingerprint", r[IR_COLLISIONS]); return MNC_ERR_RANGE; }
	return MNC_OK;
}

// A slab of device memory cut into pieces of 8-byte alignment
struct Slab {
	char *p = nullptr;
	size_t used = 0;
	template <class T> size_t want(size_t n) { const size_t at = used; used += (n * sizeof(T) + 7) / 8 * 8; return at; }
	template <class T> T *at(size_t o) const { return (T*)(p + o); }
};

// The span of every base of [w0 + start, w0 + n) into spanq, the selected alleles counted into cnt and scanned into offs
// (m + 1 words), the sum of their lengths in n_bases[0]; *total = their number, on the host (one wait)
static int ins_segments(mnc_pileup *pu, int64_t w0, int64_t n, bool all, int rid, int64_t start, PileThr thr, InsRule rule, int32_t *spanq, int32_t *cnt, int64_t *offs,
                        unsigned long long *n_bases, int64_t *total, unsigned long long *h_bases)
{
	const int64_t m = n - start;
	pile_tile_sums(pu, w0, n, all);
	HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)m * 4, pu->st));
	HIP_TRY(hipMemsetAsync(n_bases, 0, 8, pu->st));
	pile_launch<4>(pu, w0, n, all, rid, start, thr, spanq, nullptr, 0, nullptr);
	hipLaunchKernelGGL(mnc_ins_select<0>, dim3(ins_grid(pu->ins.slots)), dim3(256), 0, pu->st, pu->ins, w0 + start, m, spanq, rule, cnt, nullptr, nullptr, n_bases);
	exclusive_scan(ScanInPlain<int32_t>{cnt}, m, offs, pu->tile_cnt, pu->st);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(total, offs + m, 8, hipMemcpyDeviceToHost, pu->st));
	HIP_TRY(hipMemcpyAsync(h_bases, n_bases, 8, hipMemcpyDeviceToHost, pu->st));
	HIP_TRY(hipStreamSynchronize(pu->st));
	return MNC_OK;
}

// ... and the slots of the selected alleles in `sel` (`total` of them), base by base, each base's by (length, bases).
// Read-outs are for one thread at a time; should an add slip in between the passes all the same, a place of `sel` that the
// second pass does not fill stays -1 and is read as no allele, and nothing is written beyond `total`.
static hipError_t ins_order(mnc_pileup *pu, int64_t g0, int64_t m, InsRule rule, const int32_t *spanq, int32_t *cnt, const int64_t *offs, int64_t *sel, int64_t total)
{
	const hipError_t he = hipMemsetAsync(sel, 0xff, (size_t)total * 8, pu->st);
	if (he != hipSuccess) return he;
	hipLaunchKernelGGL(mnc_ins_select<1>, dim3(ins_grid(pu->ins.slots)), dim3(256), 0, pu->st, pu->ins, g0, m, spanq, rule, cnt, offs, sel, nullptr);
	hipLaunchKernelGGL(mnc_ins_sort, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, pu->st, pu->ins, m, offs, sel);
	return hipGetLastError();
}

void pileup_add_ins_launch(mnc_pileup *pu, const Batch &B, int sel, hipStream_t st)
{
	hipLaunchKernelGGL(mnc_pile_add_ins, dim3((B.n_reads + 3) / 4), dim3(256), 0, st, B, sel, pu->d_off, pu->n_contigs, pu->n_words, pu->track, pu->alt, pu->ins);
}

} // namespace mnc

// ---------------------------------------------------------------- C-ABI: the insertion store
extern "C" int mnc_pileup_store_insertions(mnc_pileup *pu, int64_t cap_alleles, int64_t cap_pool_bases)
{
	if (!pu) return MNC_ERR_ARG;
	if (cap_alleles <= 0 || cap_alleles > ((int64_t)1 << 30) || cap_pool_bases < 0) { set_error("cap_alleles %lld (1 .. 2^30), cap_pool_bases %lld (0 or more)", (long long)cap_alleles, (long long)cap_pool_bases); return MNC_ERR_ARG; }
	HIP_TRY(hipSetDevice(pu->device));
	std::lock_guard<std::mutex> lk(pu->mu);
	if (pu->ins_on || pu->added) { set_error("mnc_pileup_store_insertions comes once, before the first add"); return MNC_ERR_ARG; }
	InsTable T{};
	T.cap_alleles = cap_alleles, T.pool_bytes = (cap_pool_bases + 1) / 2;
	for (T.slots = 64; T.slots < 2 * cap_alleles; T.slots <<= 1) {}
	const size_t ns = (size_t)T.slots;
	const size_t n_bufs = pu->bufs.size();
	const int64_t bytes0 = pu->bytes;
	hipError_t he = hipSuccess;
	pu->alloc(he, (void**)&T.fp, ns * 8);
	pu->alloc(he, (void**)&T.sum, ns * 8);
	pu->alloc(he, (void**)&T.pay, ns * 8);
	pu->alloc(he, (void**)&T.place, ns * 8);
	pu->alloc(he, (void**)&T.count, ns * 4);
	pu->alloc(he, (void**)&T.len, ns * 4);
	pu->alloc(he, (void**)&T.pool, (size_t)T.pool_bytes);
	pu->alloc(he, (void**)&T.ctr, INC_N * 8);
	if (he == hipSuccess) {
		pu->ins = T;
		he = ins_clear(pu);
		if (he == hipSuccess) he = pu->own_done();                // an add comes behind the clearing
	}
	if (he != hipSuccess) {
		set_error("insertion store of %lld alleles (40 bytes a slot, %lld slots) and %lld pool bytes: %s", (long long)cap_alleles, (long long)T.slots, (long long)T.pool_bytes, hipGetErrorString(he));
		(void)hipStreamSynchronize(pu->st);
		while (pu->bufs.size() > n_bufs) { (void)hipFree(pu->bufs.back()); pu->bufs.pop_back(); }
		pu->bytes = bytes0, pu->ins = InsTable{};
		return Accum::failed(he);
	}
	pu->ins_on = true;
	return MNC_OK;
}

extern "C" int mnc_pileup_add_insertion_list(mnc_pileup *pu, int64_t n, const int32_t *rid, const int32_t *pos, const int32_t *len, const int32_t *count,
                                             const int64_t *base_off, const uint8_t *bases)
{
	if (!pu || n < 0 || (n && (!rid || !pos || !len || !count || !base_off || !bases))) return MNC_ERR_ARG;
	if (!pu->ins_on) { set_error("the pileup stores no insertions (mnc_pileup_store_insertions was not called)"); return MNC_ERR_ARG; }
	if (n == 0) return MNC_OK;
	// ---- every check on the host, before anything is touched
	std::vector<int64_t> place;
	try {
		place.resize((size_t)n);
	} catch (const std::bad_alloc &) { return MNC_ERR_NOMEM; }
	int64_t end = 0;                                             // the bases of the rows so far end here
	for (int64_t i = 0; i < n; ++i) {
		if (rid[i] < 0 || rid[i] >= pu->n_contigs) { set_error("row %lld: contig %d out of range", (long long)i, rid[i]); return MNC_ERR_ARG; }
		const int64_t clen = pu->off[rid[i] + 1] - pu->off[rid[i]];
		if (pos[i] < 0 || pos[i] >= clen) { set_error("row %lld: position %d outside contig %d of %lld bases", (long long)i, pos[i], rid[i], (long long)clen); return MNC_ERR_ARG; }
		if (len[i] <= 0 || (uint32_t)len[i] > INS_LEN || count[i] <= 0) { set_error("row %lld: length %d, count %d (each 1 or more)", (long long)i, len[i], count[i]); return MNC_ERR_ARG; }
		if (base_off[i] < end) { set_error("row %lld: base offset %lld before the end of the row in front (%lld)", (long long)i, (long long)base_off[i], (long long)end); return MNC_ERR_ARG; }
		end = base_off[i] + len[i];
		place[(size_t)i] = pu->off[rid[i]] + pos[i];
	}
	HIP_TRY(hipSetDevice(pu->device));
	Slab d;
	const size_t o_place = d.want<int64_t>((size_t)n), o_boff = d.want<int64_t>((size_t)n), o_len = d.want<int32_t>((size_t)n), o_cnt = d.want<int32_t>((size_t)n),
	             o_bases = d.want<uint8_t>((size_t)end);
	HIP_TRY(hipMalloc((void**)&d.p, d.used));
	std::lock_guard<std::mutex> lk(pu->mu);
	hipError_t he = hipMemcpyAsync(d.at<int64_t>(o_place), place.data(), (size_t)n * 8, hipMemcpyHostToDevice, pu->st);
	if (he == hipSuccess) he = hipMemcpyAsync(d.at<int64_t>(o_boff), base_off, (size_t)n * 8, hipMemcpyHostToDevice, pu->st);
	if (he == hipSuccess) he = hipMemcpyAsync(d.at<int32_t>(o_len), len, (size_t)n * 4, hipMemcpyHostToDevice, pu->st);
	if (he == hipSuccess) he = hipMemcpyAsync(d.at<int32_t>(o_cnt), count, (size_t)n * 4, hipMemcpyHostToDevice, pu->st);
	if (he == hipSuccess) he = hipMemcpyAsync(d.at<uint8_t>(o_bases), bases, (size_t)end, hipMemcpyHostToDevice, pu->st);
	if (he == hipSuccess) {
		pu->added = true;
		hipLaunchKernelGGL(mnc_pile_add_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, pu->st, pu->ins, n, d.at<int64_t>(o_place), d.at<int32_t>(o_len),
		                   d.at<int32_t>(o_cnt), d.at<int64_t>(o_boff), d.at<uint8_t>(o_bases));
		he = hipGetLastError();
	}
	if (he == hipSuccess) he = pu->own_done();                   // an engine's add comes behind it
	const hipError_t hs = hipStreamSynchronize(pu->st);          // the host arrays are read until here
	if (he == hipSuccess) he = hs;
	(void)hipFree(d.p);
	if (he != hipSuccess) { set_error("pileup add_insertion_list: %s", hipGetErrorString(he)); return MNC_ERR_HIP; }
	return MNC_OK;
}

extern "C" int mnc_pileup_insertion_info(mnc_pileup *pu, int64_t *n_alleles, int64_t *n_events, int64_t *n_dropped, int64_t *n_pool_bases, int64_t *n_pool_dropped,
                                         int64_t *n_collisions)
{
	if (!pu) return MNC_ERR_ARG;
	unsigned long long r[IR_N];
	if (int rc = ins_totals(pu, r)) return rc;
	if (n_alleles) *n_alleles = (int64_t)r[IR_ALLELES];
	if (n_events) *n_events = (int64_t)r[IR_EVENTS];
	if (n_dropped) *n_dropped = (int64_t)r[IR_CTR + INC_DROPPED];
	if (n_pool_bases) *n_pool_bases = (int64_t)r[IR_POOL_BASES];
	if (n_pool_dropped) *n_pool_dropped = (int64_t)r[IR_CTR + INC_POOL_DROPPED];
	if (n_collisions) *n_collisions = (int64_t)r[IR_COLLISIONS];
	return MNC_OK;
}

extern "C" int mnc_pileup_call_insertions(mnc_pileup *pu, int rid, int32_t min_depth, int32_t min_count, int32_t min_permille, mnc_insertion_t *out, int64_t cap, int64_t *n,
                                          char *bases, int64_t cap_bases, int64_t *n_bases)
{
	if (!pu || !n || !n_bases) return MNC_ERR_ARG;
	*n = *n_bases = 0;
	if (rid < -1 || rid >= pu->n_contigs) { set_error("contig %d out of range", rid); return MNC_ERR_ARG; }
	if (int rc = ins_readable(pu)) return rc;
	const bool all = rid < 0;
	const int64_t w0 = all ? 0 : pu->off[rid], len = all ? pu->n_words : pu->off[rid + 1] - w0;
	if (len == 0) return MNC_OK;
	const InsRule rule{0, min_count, min_permille};
	// ---- spans, counts per base, scan
	Slab a;
	const size_t o_span = a.want<int32_t>((size_t)len), o_cnt = a.want<int32_t>((size_t)len), o_offs = a.want<int64_t>((size_t)len + 1), o_nb = a.want<int64_t>(1);
	HIP_TRY(hipMalloc((void**)&a.p, a.used));
	int64_t total = 0;
	unsigned long long nb = 0;
	int rc = ins_segments(pu, w0, len, all, rid, 0, PileThr{min_depth, 0, 0}, rule, a.at<int32_t>(o_span), a.at<int32_t>(o_cnt), a.at<int64_t>(o_offs),
	                      a.at<unsigned long long>(o_nb), &total, &nb);
	if (rc == MNC_OK) {
		*n = total, *n_bases = (int64_t)nb;
		if (cap < total || cap_bases < (int64_t)nb) {
			set_error("%lld insertion alleles of %lld bases, room for %lld and %lld", (long long)total, (long long)nb, (long long)cap, (long long)cap_bases);
			rc = MNC_ERR_RANGE;
		} else if (total && (!out || (nb && !bases))) rc = MNC_ERR_ARG;
	}
	if (rc != MNC_OK || total == 0) { (void)hipFree(a.p); return rc; }
	// ---- scatter, sort, the records' base offsets, write
	Slab b;
	const size_t o_sel = b.want<int64_t>((size_t)total), o_boff = b.want<int64_t>((size_t)total + 1), o_sums = b.want<int64_t>((size_t)total / SC_TILE + 2),
	             o_rec = b.want<mnc_insertion_t>((size_t)total), o_chr = b.want<char>((size_t)nb);
	if (hipMalloc((void**)&b.p, b.used) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(a.p); set_error("%lld insertion alleles: out of device memory", (long long)total); return MNC_ERR_NOMEM; }
	int64_t *sel = b.at<int64_t>(o_sel), *boff = b.at<int64_t>(o_boff);
	const hipError_t he = ins_order(pu, w0, len, rule, a.at<int32_t>(o_span), a.at<int32_t>(o_cnt), a.at<int64_t>(o_offs), sel, total);
	if (he == hipSuccess) exclusive_scan(InsLenIn{pu->ins.len, sel}, total, boff, b.at<int64_t>(o_sums), pu->st);
	if (he == hipSuccess) hipLaunchKernelGGL(mnc_ins_write, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, pu->st, pu->ins, total, sel, boff, a.at<int32_t>(o_span), w0, pu->d_off, pu->n_contigs,
	                   b.at<mnc_insertion_t>(o_rec), b.at<char>(o_chr));
	rc = pu->finish(he, b.p, {out, b.at<mnc_insertion_t>(o_rec), (size_t)total * sizeof(mnc_insertion_t)}, {nb ? bases : nullptr, b.at<char>(o_chr), (size_t)nb},
	                "insertion alleles");
	(void)hipFree(a.p);
	return rc;
}

extern "C" int mnc_pileup_consensus_ins(mnc_pileup *pu, int rid, int64_t start, int64_t end, int32_t min_depth, char *out, int64_t cap, int64_t *n)
{
	if (!pu || !n) return MNC_ERR_ARG;
	*n = 0;
	if (int rc = accum_interval(pu->off, rid, start, end)) return rc;
	if (int rc = ins_readable(pu)) return rc;
	const int64_t m = end - start, w0 = pu->off[rid];
	if (m == 0) return MNC_OK;
	const InsRule rule{1, 0, 0};
	// ---- the bases' own characters and spans; the alleles of more than half a base's span, base by base
	Slab a;
	const size_t o_span = a.want<int32_t>((size_t)m), o_cnt = a.want<int32_t>((size_t)m), o_offs = a.want<int64_t>((size_t)m + 1), o_nb = a.want<int64_t>(1),
	             o_best = a.want<int64_t>((size_t)m), o_cons = a.want<char>((size_t)m);
	HIP_TRY(hipMalloc((void**)&a.p, a.used));
	int32_t *cnt = a.at<int32_t>(o_cnt);
	int64_t *offs = a.at<int64_t>(o_offs);
	int64_t total = 0, out_len = 0;
	unsigned long long nb = 0;
	int rc = ins_segments(pu, w0, end, false, rid, start, PileThr{min_depth, 0, 0, true}, rule, a.at<int32_t>(o_span), cnt, offs, a.at<unsigned long long>(o_nb), &total, &nb);
	if (rc != MNC_OK) { (void)hipFree(a.p); return rc; }
	pile_launch<3>(pu, w0, end, false, rid, start, PileThr{min_depth, 0, 0}, nullptr, nullptr, 0, a.at<char>(o_cons));
	int64_t *sel = nullptr;
	if (hipMalloc((void**)&sel, (size_t)(total ? total : 1) * 8) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(a.p); set_error("consensus with insertions: out of device memory"); return MNC_ERR_NOMEM; }
	hipError_t he = total ? ins_order(pu, w0 + start, m, rule, a.at<int32_t>(o_span), cnt, offs, sel, total) : hipSuccess;
	// ---- per base the allele and the output length; scan; write
	if (he == hipSuccess) {
		hipLaunchKernelGGL(mnc_ins_best, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, pu->st, pu->ins, m, offs, sel, a.at<int64_t>(o_best), cnt);
		exclusive_scan(ScanInPlain<int32_t>{cnt}, m, offs, pu->tile_cnt, pu->st);   // (the segments are used up: their offsets make room)
		he = hipGetLastError();
	}
	if (he == hipSuccess) he = hipMemcpyAsync(&out_len, offs + m, 8, hipMemcpyDeviceToHost, pu->st);
	if (he == hipSuccess) he = hipStreamSynchronize(pu->st);
	(void)hipFree(sel);
	if (he != hipSuccess) { (void)hipFree(a.p); set_error("consensus with insertions: %s", hipGetErrorString(he)); return MNC_ERR_HIP; }
	*n = out_len;
	if (cap < out_len) { (void)hipFree(a.p); set_error("a consensus of %lld characters, room for %lld", (long long)out_len, (long long)cap); return MNC_ERR_RANGE; }
	if (!out) { (void)hipFree(a.p); return MNC_ERR_ARG; }
	char *tmp = nullptr;
	if (hipMalloc((void**)&tmp, (size_t)out_len) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(a.p); return MNC_ERR_NOMEM; }
	hipLaunchKernelGGL(mnc_ins_cons_write, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, pu->st, pu->ins, m, a.at<char>(o_cons), a.at<int64_t>(o_best), offs, tmp);
	rc = pu->finish(hipSuccess, tmp, {out, tmp, (size_t)out_len}, {}, "consensus with insertions");
	(void)hipFree(a.p);
	return rc;
}
