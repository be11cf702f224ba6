// The insertion store of a pileup (include/monica_amd.h, "pileup": insertion alleles): a device hash table of alleles --
// (place, length, bases) -> count -- that the add kernels of k_pile_ins.hip fill and its read-outs walk.  Here: the table's
// layout, the ONE definition of the two hashes, the claim, and the wave-wide add that the engine's walk and the caller's
// lists share.
//
// No lane ever waits on another.  A slot is claimed by one 64-bit compare-and-swap on the fingerprint (0: free), probing is
// linear and bounded, the count is one int32 atomic add and the check sum one uint64 atomic add.  The winner of the claim
// alone writes the payload (place, length, packed bases or a pool offset); nobody reads a payload before the read-outs,
// which stream order puts behind the adds.  There is no spin, no lock and no "busy" state: a lane that finds no slot counts
// its event as dropped and goes on.
//
// The hashes are position-wise: a wrapping sum of mix(index, code) over the bases, folded with the place and the length at
// the end.  A sum commutes, so one lane over all bases and a wave with one base per lane (a cross-lane sum) get the same
// value.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include "device.h"

namespace mnc {

constexpr int INS_SHORT = 32;                     // bases that fit one word at two bits each (no N among them)
constexpr int INS_PROBE = 128;                    // slots looked at before an event counts as dropped
constexpr uint32_t INS_POOLED = 1u << 30;         // len word: the bases are in the pool (4-bit codes) from byte `pay` on
constexpr uint32_t INS_NOBASES = 1u << 31;        // ... they did not fit the pool: the count is exact, the bases are unknown
constexpr uint32_t INS_LEN = INS_POOLED - 1;
enum { INC_ALLELES, INC_DROPPED, INC_POOL, INC_POOL_DROPPED, INC_N };   // the counters: claims, events without a slot, pool bytes reserved, alleles without bases

struct InsTable {
	unsigned long long *fp;                       // [slots] fingerprint, 0: free
	unsigned long long *sum;                      // [slots] wrapping sum of h2 over the events
	unsigned long long *pay;                      // [slots] the bases, two bits each from bit 0 on -- or the pool byte offset
	int64_t *place;                               // [slots] global word of the base on the insertion's left
	int32_t *count;                               // [slots]
	uint32_t *len;                                // [slots] length | INS_POOLED | INS_NOBASES
	uint8_t *pool;                                // [pool_bytes] two 4-bit codes a byte, the first base in the low half
	unsigned long long *ctr;                      // [INC_N]
	int64_t slots, cap_alleles, pool_bytes;       // slots: a power of two, at least 2 * cap_alleles
};

__host__ __device__ __forceinline__ unsigned long long ins_mix(unsigned long long x)
{
	x += 0x9e3779b97f4a7c15ull;
	x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
	x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
	return x ^ (x >> 31);
}
// the share of base `i` with code `c` (0 .. 4) in the two hashes; the hashes differ in their seeds only
__host__ __device__ __forceinline__ unsigned long long ins_mix1(int i, int c) { return ins_mix(((unsigned long long)(unsigned)i << 3 | (unsigned)c) ^ 0x243f6a8885a308d3ull); }
__host__ __device__ __forceinline__ unsigned long long ins_mix2(int i, int c) { return ins_mix(((unsigned long long)(unsigned)i << 3 | (unsigned)c) ^ 0x13198a2e03707344ull); }
// the fingerprint (never 0) and the check hash of an allele, from the sums of its bases' shares
__host__ __device__ __forceinline__ unsigned long long ins_fp(int64_t place, int len, unsigned long long s1)
{
	const unsigned long long h = ins_mix(s1 ^ ins_mix((unsigned long long)place * 0xa4093822299f31d1ull + (unsigned)len));
	return h ? h : 1ull;
}
__host__ __device__ __forceinline__ unsigned long long ins_h2(int64_t place, int len, unsigned long long s2)
{
	return ins_mix(s2 + ins_mix((unsigned long long)place ^ (unsigned long long)(unsigned)len << 40 ^ 0x082efa98ec4e6c89ull));
}

#ifdef __HIPCC__
// One event of `cnt` observations.  Returns the slot if this lane claimed it (the caller then counts the claim with
// ins_wave_add's `claims` and writes the payload), -1 otherwise: the allele was there, or the event was dropped.  At most
// INS_PROBE slots are looked at, each once.  full: the table holds cap_alleles alleles (ins_full) and takes no new one.
__device__ __forceinline__ int64_t ins_claim(const InsTable &T, unsigned long long fp, unsigned long long h2, int cnt, bool full)
{
	const unsigned long long mask = (unsigned long long)T.slots - 1ull;
	const int limit = T.slots < INS_PROBE ? (int)T.slots : INS_PROBE;
	unsigned long long s = fp & mask;
	for (int i = 0; i < limit; ++i, s = (s + 1ull) & mask) {
		unsigned long long cur = __hip_atomic_load(T.fp + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		bool won = false;
		if (cur == 0ull) {
			// a free slot: the allele is not in the table (nothing is ever taken out).  A full table takes no new allele
			if (full) break;
			won = __hip_atomic_compare_exchange_strong(T.fp + s, &cur, fp, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		if (!won && cur != fp) continue;                       // somebody else's: the next slot
		(void)__hip_atomic_fetch_add(T.count + s, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		(void)__hip_atomic_fetch_add(T.sum + s, (unsigned long long)cnt * h2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		return won ? (int64_t)s : -1;
	}
	(void)__hip_atomic_fetch_add(T.ctr + INC_DROPPED, (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	return -1;
}

// The counter of alleles is kept off the hot path: one address for every claim of every wave would serialise the adds.  A
// wave counts its claims in a register (`claims` of ins_wave_add), adds them with ONE atomic when it is through with its
// record or its rows (ins_flush), and looks at the counter once per chunk of its walk (ins_full).  cap_alleles is therefore
// kept with the lag of the records in flight; the slots (at least twice cap_alleles) and the probe limit bound what that
// lag can add, and the read-outs count the alleles that are there.
__device__ __forceinline__ bool ins_full(const InsTable &T)
{
	return __hip_atomic_load(T.ctr + INC_ALLELES, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned long long)T.cap_alleles;
}
__device__ __forceinline__ void ins_flush(const InsTable &T, int claims)
{
	if (claims && lane_id() == 0) (void)__hip_atomic_fetch_add(T.ctr + INC_ALLELES, (unsigned long long)claims, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned long long ins_wave_sum(unsigned long long x)
{
	for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
	return x;
}

// The insertions of the 64 lanes of a WHOLE wave, at most one each: `have`, at global word `place`, `len` bases, `cnt`
// observations; code(src, j) is base j as a code A C G T N = 0 .. 4, `src` whatever tells one lane's bases from another's.
//   short   (len <= INS_SHORT) the lane gathers its own bases, packs and hashes them and claims; lanes diverge over the
//           gather only.  One with an N among its bases goes the long way.
//   long    a ballot of the lanes that have one, then the wave takes them one after the other: the fields come from the
//           owning lane, the bases are walked 64 at a time with one base per lane, two cross-lane sums give the hashes,
//           lane 0 claims and reserves pool bytes with one atomic add, and the wave writes the 4-bit codes, a byte per lane.
// Every lane of the wave must call it (ballot, shuffles); nothing here waits.  `full` and `claims` are the wave's: see above.
template <class Code>
__device__ __forceinline__ void ins_wave_add(const InsTable &T, bool have, int64_t place, int len, int cnt, long long src, Code code, bool full, int &claims)
{
	const int lane = lane_id();
	bool wide = have && len > INS_SHORT;
	int64_t mine = -1;                                        // the slot this lane claimed the short way
	unsigned long long pk = 0;
	if (have && len <= INS_SHORT) {
		unsigned long long s1 = 0, s2 = 0;
		bool has_n = false;
		for (int j = 0; j < len; ++j) {
			const int c = code(src, j);
			has_n |= c > 3;
			pk |= (unsigned long long)(c & 3) << (2 * j);
			s1 += ins_mix1(j, c), s2 += ins_mix2(j, c);
		}
		if (has_n) wide = true;
		else mine = ins_claim(T, ins_fp(place, len, s1), ins_h2(place, len, s2), cnt, full);
		if (mine >= 0) T.place[mine] = place, T.len[mine] = (uint32_t)len, T.pay[mine] = pk;
	}
	claims += __popcll(__ballot(mine >= 0));
	unsigned long long todo = __ballot(wide);
	while (todo) {                                            // (wave-uniform)
		const int owner = __ffsll((long long)todo) - 1;
		todo &= todo - 1ull;
		const int64_t P = __shfl((long long)place, owner);
		const long long S = __shfl(src, owner);
		const int L = __shfl(len, owner), N = __shfl(cnt, owner);
		unsigned long long s1 = 0, s2 = 0;
		for (int j0 = 0; j0 < L; j0 += 64) {
			const int j = j0 + lane;
			if (j < L) {
				const int c = code(S, j);
				s1 += ins_mix1(j, c), s2 += ins_mix2(j, c);
			}
		}
		s1 = ins_wave_sum(s1), s2 = ins_wave_sum(s2);
		const int64_t bytes = ((int64_t)L + 1) / 2;
		long long slot = -1, at = -1;
		if (lane == 0) {
			slot = ins_claim(T, ins_fp(P, L, s1), ins_h2(P, L, s2), N, full);
			if (slot >= 0) {
				at = (long long)__hip_atomic_fetch_add(T.ctr + INC_POOL, (unsigned long long)bytes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if (at < 0 || at > T.pool_bytes - bytes) {
					at = -1;
					(void)__hip_atomic_fetch_add(T.ctr + INC_POOL_DROPPED, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				}
			}
		}
		slot = __shfl(slot, 0), at = __shfl(at, 0);
		claims += slot >= 0;
		if (slot >= 0 && at >= 0)
			for (int64_t k0 = 0; k0 < bytes; k0 += 64) {
				const int64_t k = k0 + lane;
				if (k < bytes) {
					const int j = (int)(2 * k);
					T.pool[at + k] = (uint8_t)(code(S, j) | (j + 1 < L ? code(S, j + 1) : 0) << 4);
				}
			}
		if (lane == 0 && slot >= 0)
			T.place[slot] = P, T.len[slot] = (uint32_t)L | INS_POOLED | (at < 0 ? INS_NOBASES : 0u), T.pay[slot] = (unsigned long long)(at < 0 ? 0 : at);
	}
}

// base j of an allele with length word lw and payload pay (the read-outs; not for INS_NOBASES)
__device__ __forceinline__ int ins_base(const InsTable &T, uint32_t lw, unsigned long long pay, int j)
{
	if (!(lw & INS_POOLED)) return (int)(pay >> (2 * j) & 3ull);
	return T.pool[pay + (unsigned long long)(j >> 1)] >> ((j & 1) * 4) & 15;
}
#endif

} // namespace mnc
