// What the two accumulators over a caller's site list share (k_linkage.hip: the pair tables and the phase; k_haplotag.hip:
// the reads' votes per phase block): the list as it is checked on the host and held on the device, and the walk of one
// read's records with one lane per SITE -- k_linkage.hip's header comment describes the merge of the site walk with the
// CIGAR walk.  link_walk hands every 64 sites' statements to its caller; what is done with them is the caller's.  The votes
// of those statements by phase block (hap_segment) are here too: k_haplotag.hip counts them, k_pile_phase.hip routes a
// record's columns by them.
#pragma once

#include <hip/hip_runtime.h>
#include <vector>
#include "pileup.h"

namespace mnc {

// a site's allele is held as the pileup numbers its channels (pileup.h): 0 .. 3 = A C G T, CH_DEL = deleted

// ---------------------------------------------------------------- the list on the host
struct LinkSitesHost {
	std::vector<int32_t> pos, rid, first;      // [n_sites] each; first: [n_contigs + 1] the first site of every contig
	std::vector<uint8_t> alt;                  // [n_sites]
	std::vector<int64_t> off;                  // [n_contigs + 1] the contigs' first bases in the 4-bit store
	int n_contigs = 0;
};

// a site's allele as the kernels hold it; -1: none of A C G T -
inline int link_allele(uint8_t c)
{
	switch (c) {
	case 'A': return 0;
	case 'C': return 1;
	case 'G': return 2;
	case 'T': return 3;
	case '-': return CH_DEL;
	default: return -1;
	}
}

// The checks of mnc_linkage_create on its site list (include/monica_amd.h, "linkage"), before any device is looked at
inline int link_sites_check(const mnc_index *idx, const mnc_variant_t *sites, int64_t n_sites, LinkSitesHost &H)
{
	if (n_sites < 0 || (n_sites && !sites)) return MNC_ERR_ARG;
	if (n_sites > MNC_LINKAGE_MAX_SITES) { set_error("%lld sites, at most %lld", (long long)n_sites, (long long)MNC_LINKAGE_MAX_SITES); return MNC_ERR_ARG; }
	if (idx->seq_off.size() != idx->contig_len.size() + 1) { set_error("the index holds no contig bases"); return MNC_ERR_ARG; }
	const int n_contigs = H.n_contigs = (int)idx->contig_len.size();
	std::vector<int32_t> &pos = H.pos, &rid = H.rid, &first = H.first;
	std::vector<uint8_t> &alt = H.alt;
	std::vector<int64_t> &off = H.off;
	try {
		pos.resize((size_t)n_sites), rid.resize((size_t)n_sites), alt.resize((size_t)n_sites), first.assign((size_t)n_contigs + 1, 0);
		off.assign(idx->seq_off.begin(), idx->seq_off.end());
	} catch (const std::bad_alloc &) { return MNC_ERR_NOMEM; }
	for (int64_t i = 0; i < n_sites; ++i) {
		const mnc_variant_t &v = sites[i];
		const int a = link_allele(v.alt);
		if (v.alt == '+') set_error("site %lld is an insertion allele ('+'): linkage takes A C G T and '-'", (long long)i);
		else if (a < 0) set_error("site %lld: allele 0x%02x is none of A C G T -", (long long)i, (unsigned)v.alt);
		else if (v.rid < 0 || v.rid >= n_contigs || v.pos < 0 || v.pos >= off[v.rid + 1] - off[v.rid])
			set_error("site %lld: position %d of contig %d is outside the index", (long long)i, (int)v.pos, (int)v.rid);
		else if (i && (v.rid < rid[i - 1] || (v.rid == rid[i - 1] && (v.pos < pos[i - 1] || (v.pos == pos[i - 1] && a <= (int)alt[i - 1])))))
			set_error("site %lld does not ascend strictly in (rid, pos, allele A C G T -)", (long long)i);
		else {
			pos[i] = v.pos, rid[i] = v.rid, alt[i] = (uint8_t)a, first[v.rid + 1] += 1;
			continue;
		}
		return MNC_ERR_ARG;
	}
	for (int c = 0; c < n_contigs; ++c) first[c + 1] += first[c];
	return MNC_OK;
}

// ---------------------------------------------------------------- ... and on the device
struct LinkSites {
	const int32_t *pos, *first;                // [n_sites], [n_contigs + 1]
	const uint8_t *alt;                        // [n_sites]
	const int64_t *off;                        // [n_contigs + 1]
	int n_contigs;
};

// the list's four arrays: allocated with the accumulator's other buffers, filled once
struct LinkSitesDev {
	int32_t *pos = nullptr, *first = nullptr;
	uint8_t *alt = nullptr;
	int64_t *off = nullptr;
	void alloc(Accum &a, hipError_t &he, const LinkSitesHost &H)
	{
		a.alloc(he, (void**)&pos, H.pos.size() * 4);
		a.alloc(he, (void**)&alt, H.alt.size());
		a.alloc(he, (void**)&first, H.first.size() * 4);
		a.alloc(he, (void**)&off, H.off.size() * 8);
	}
	void fill(hipError_t &he, const LinkSitesHost &H) const
	{
		if (he == hipSuccess && H.pos.size()) he = hipMemcpy(pos, H.pos.data(), H.pos.size() * 4, hipMemcpyHostToDevice);
		if (he == hipSuccess && H.alt.size()) he = hipMemcpy(alt, H.alt.data(), H.alt.size(), hipMemcpyHostToDevice);
		if (he == hipSuccess) he = hipMemcpy(first, H.first.data(), H.first.size() * 4, hipMemcpyHostToDevice);
		if (he == hipSuccess) he = hipMemcpy(off, H.off.data(), H.off.size() * 8, hipMemcpyHostToDevice);
	}
	LinkSites view(int n_contigs) const { return LinkSites{pos, first, alt, off, n_contigs}; }
};

__device__ __forceinline__ void link_put(int32_t *w, int v) { (void)__hip_atomic_fetch_add(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the first site of [lo, hi) whose position is not below p (the same answer in every lane)
__device__ __forceinline__ int link_lower(const int32_t *pos, int lo, int hi, int p)
{
	while (lo < hi) {
		const int mid = lo + (hi - lo) / 2;
		if (pos[mid] < p) lo = mid + 1; else hi = mid;
	}
	return lo;
}

// The walk of ONE record r (region slot `slot`, n_cigar > 0) of a read of qlen > 0 bases whose sites are [s_lo, s_hi) of the
// list, s_lo < s_hi: for c0 = s_lo, s_lo + 64, .., chunk(c0, s, valid, stmt): this lane's site s = c0 + lane, whether it lies
// below s_hi, and what the record says there (0: nothing, 1: REF, 2: ALT; 0 where !valid).  Every lane of the wave reaches
// every call.
template <class C>
__device__ __forceinline__ void link_walk_record(const Batch &B, const mnc_reg_t &r, int64_t slot, const uint8_t *read, int qlen, const LinkSites &L,
                                                 int s_lo, int s_hi, C chunk)
{
	const int lane = lane_id();
	const int n_c = r.n_cigar;
	const int64_t coff = L.off[r.rid];
	const uint32_t *src = B.cig_reg + B.regdp[slot].cig_off;
	auto Q = [&](int p) -> int {                            // column p of the query side, on the hit's strand (pile_add_read)
		int at = r.rev ? r.qe - 1 - p : r.qs + p;
		at = at < 0 ? 0 : at >= qlen ? qlen - 1 : at;
		const int c = base_nt4(read[at]);
		return r.rev ? (c < 4 ? 3 - c : 4) : c;
	};
	// ---- the chunk of 64 operations at hand
	int k0 = 0, qoff = 0;                                   // its first operation; query columns before it
	int64_t toff = r.rs;                                    // reference position before it
	int op = 0, it = 0, my_t0 = 0, my_q0 = 0, tot_t = 0, tot_q = 0;
	auto load = [&] {
		const int k = k0 + lane;
		const uint32_t wd = k < n_c ? src[k] : 0u;
		op = (int)(wd & 0xfu);
		const int l = k < n_c && op <= 2 ? (int)(wd >> 4) : 0;
		const int dt = op != 1 ? l : 0, dq = op != 2 ? l : 0;
		it = cov_incl_add(dt);
		const int iq = cov_incl_add(dq);
		my_t0 = it - dt, my_q0 = qoff + iq - dq;
		tot_t = __shfl(it, 63), tot_q = __shfl(iq, 63);
	};
	load();
	for (int c0 = s_lo; c0 < s_hi; c0 += 64) {
		const int s = c0 + lane;
		const bool valid = s < s_hi;
		const int p = valid ? L.pos[s] : 0, al = valid ? (int)L.alt[s] : 0;
		int stmt = 0;                                         // 1: REF, 2: ALT
		bool done = !valid;
		for (;;) {                                            // (every lane of the wave runs it: the exits are the wave's)
			const bool mine = !done && p < toff + tot_t;        // (p >= toff: the chunks before have been left behind by this lane)
			const int rel = mine ? (int)(p - toff) : 0;
			int o = 0;                                          // this site's operation: the first whose inclusive advance exceeds rel
			for (int step = 32; step > 0; step >>= 1) {
				const int e = __shfl(it, o + step - 1);
				if (e <= rel) o += step;
			}
			const int o_op = __shfl(op, o), t0 = __shfl(my_t0, o), q0 = __shfl(my_q0, o);
			if (mine) {
				if (o_op == 0) {
					const int qc = Q(q0 + rel - t0), tc = pile_ref(B.seq4, coff + p);
					stmt = al < 4 && qc == al ? 2 : tc < 4 && qc == tc ? 1 : 0;
				} else if (o_op == 2) stmt = al == CH_DEL ? 2 : 0;
				done = true;
			}
			if (!__ballot(!done)) break;
			toff += tot_t, qoff += tot_q, k0 += 64;
			if (k0 >= n_c) { tot_t = tot_q = 0; break; }        // (a site behind the CIGAR's end: none, re is its end)
			load();
		}
		chunk(c0, s, valid, stmt);
	}
}

// The walk of read `rd` (a whole wave's; rd < B.n_reads): for every record that `sel` selects and that has a site under it,
// record(s_lo, s_hi) -- its sites are [s_lo, s_hi) of the list -- and then link_walk_record's chunks.
template <class R, class C>
__device__ __forceinline__ void link_walk(const Batch &B, uint32_t rd, int sel, const LinkSites &L, R record, C chunk)
{
	const int64_t read_off = B.offsets[rd];
	const int qlen = (int)(B.offsets[rd + 1] - read_off);
	if (qlen <= 0) return;
	const uint8_t *read = B.bases + read_off;
	cov_for_records(B, rd, sel, L.n_contigs, [&](const mnc_reg_t &r, int64_t slot) {
		if (r.n_cigar <= 0) return;
		const int s_lo = link_lower(L.pos, L.first[r.rid], L.first[r.rid + 1], r.rs);
		const int s_hi = link_lower(L.pos, s_lo, L.first[r.rid + 1], r.re);
		if (s_lo >= s_hi) return;                               // no site under this record
		record(s_lo, s_hi);
		link_walk_record(B, r, slot, read, qlen, L, s_lo, s_hi, chunk);
	});
}

// ---------------------------------------------------------------- the votes per phase block (k_haplotag.hip, k_pile_phase.hip)
// what a haplotag accumulator holds, as its kernel and the phased pileup's see it (the latter reads the first five alone)
struct HapView {
	LinkSites list;
	const int32_t *block;
	const uint8_t *phase;
	int min_votes, min_permille;
	int32_t *blk, *tag, *votes;
};

HapView haplotag_view(const mnc_haplotag *ht);              // k_haplotag.hip

// bits [lo, hi) of a 64-bit mask, 0 <= lo < hi <= 64
__device__ __forceinline__ unsigned long long hap_bits(int lo, int hi) { return (hi < 64 ? (1ull << hi) - 1ull : ~0ull) & ~((1ull << lo) - 1ull); }

// the decision of include/monica_amd.h, "haplotag", for the votes (n0, n1) of one (record, block)
__device__ __forceinline__ bool hap_decided(int n0, int n1, int min_votes, int min_permille)
{
	const int tot = n0 + n1, diff = n0 > n1 ? n0 - n1 : n1 - n0;
	return tot >= min_votes && diff && (long long)diff * 1000 >= (long long)min_permille * tot;
}

// One link_walk chunk's votes by block (k_haplotag.hip's header comment): this lane's segment -- its block b and its votes
// n0 / n1, with what was carried in where the segment continues it -- and whether it CLOSES here with a vote in it.  A lane
// that owns no segment never closes.  (cb, cn0, cn1): the open block carried over the border, wave-uniform; -1, 0, 0 at a
// record's start.  s_hi: the end of the record's sites.
struct HapSeg {
	int b, n0, n1;
	bool closes;
};
__device__ __forceinline__ HapSeg hap_segment(const int32_t *block, const uint8_t *phase, int c0, int s, bool valid, int stmt, int s_hi, int &cb, int &cn0, int &cn1)
{
	const int lane = lane_id();
	const int b = valid ? block[s] : -1;
	const int hap = stmt ? (stmt - 1) ^ (int)phase[s] : -1;
	const unsigned long long v0 = __ballot(hap == 0), v1 = __ballot(hap == 1);
	const int below = __shfl_up(b, 1);
	const bool head = valid && b != (lane ? below : cb);
	const unsigned long long heads = __ballot(head), starts = heads | 1ull;   // (lane 0 is valid: c0 < s_hi)
	// ---- this lane's segment, if it owns one: [lane, the next head)
	const unsigned long long above = lane < 63 ? heads & (~0ull << (lane + 1)) : 0ull;
	const bool owner = valid && (head || lane == 0);
	const bool more = c0 + 64 < s_hi && block[c0 + 64] == block[c0 + 63];   // wave-uniform: the last segment stays open
	const unsigned long long seg = hap_bits(lane, above ? __ffsll((long long)above) - 1 : 64);
	const int n0 = __popcll(v0 & seg) + (lane == 0 && !head ? cn0 : 0), n1 = __popcll(v1 & seg) + (lane == 0 && !head ? cn1 : 0);
	const bool closes = owner && (above || !more) && n0 + n1 > 0;   // (a block in which the record said nothing is not touched)
	// ---- what crosses the border: the last segment's counts, from the masks (the same in every lane)
	if (more) {
		const int ls = 63 - __clzll((long long)starts);
		const unsigned long long last = hap_bits(ls, 64);
		const bool joins = ls == 0 && !(heads & 1ull);          // the whole 64 sites continue the block carried in
		cn0 = __popcll(v0 & last) + (joins ? cn0 : 0), cn1 = __popcll(v1 & last) + (joins ? cn1 : 0);
		cb = block[c0 + 63];
	} else cb = -1, cn0 = cn1 = 0;
	return HapSeg{b, n0, n1, closes};
}

} // namespace mnc
