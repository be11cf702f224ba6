// Lowest common ancestor (include/monica_amd.h, "lca"): a read that fits several genomes about equally well is placed on the
// lowest node of the caller's taxonomy that covers all of them, and counted there -- at the species or the genus -- instead
// of being dropped.  The candidates are the abundance's (ab_common.h): the records that count, best = the largest dp_max, a
// record LIVE iff best - dp_max <= max_delta.  An accumulator of accum.h, the seventh consumer of a batch as it stands in
// HBM; runs only when asked for.
//
//   the tree        The host checks parent[] and numbers the nodes by one DFS, children in ascending id: tin[v] = v's place in
//                   pre-order, tout[v] = tin[v] + the size of v's subtree.  u is an ancestor of v (or v) iff
//                   tin[u] <= tin[v] < tout[u], so the LCA of a set is the deepest node whose [tin, tout) holds the set's
//                   smallest and largest tin.  Only parent / tin / tout travel to the device.
//   mnc_lca_add     PERSISTENT workgroups: two per CU, whatever the batch holds; a wave takes reads in a strided loop, one
//                   wave per READ, no barrier inside the loop.  The lanes hold the read's RECORDS (looping past 64): ab_best,
//                   then a live record offers tin[g] << 32 | g of its genome, and two butterflies give the smallest key and the
//                   largest tin.  "Its genome is a candidate" and "the record is live" are the same set, because s_g is a
//                   maximum: no per-genome extraction as in mnc_ab_collect.  The wave then climbs from the key's node while
//                   tout[v] <= hi: at most MNC_LCA_MAX_DEPTH - 1 wave-uniform steps, two loads each.  Lane 0 writes node[r].
//     SRC           0: the batch's region lists.  1: the rows of a candidate carry (k_carry.hip) -- a row is one slot per lane
//                   already, head[r].x = best; no loop.
//     LDS           the cut-off.  gfx950 has 160 KiB of LDS per CU.  A node costs 16 bytes: parent, tin, tout and a private
//                   uint32 direct.  MNC_LCA_LDS_NODES = 4 096 nodes are 64 KiB a workgroup, so the two workgroups of a CU hold
//                   128 KiB and 32 KiB stay free; 5 120 nodes would fill the CU to the last byte, and one workgroup per CU of
//                   8 192 would halve the waves that hide the region loads.  Staged once per workgroup -- that is what
//                   persistence buys: 48 KiB of L2 reads per WORKGROUP, not per four reads -- and flushed at its end with
//                   one 64-bit global atomic per NON-ZERO node: a sample of few taxa costs each workgroup a handful of
//                   atomics, not one per read on the same sixty HBM words (DESIGN.md K7 tells that story for
//                   mnc_count_taxa).  Above the cut-off the tree is read through L2 and every read is one agent-scope atomic.
//                   A workgroup's private count is at most the reads of one launch: below 2^31 (cap_reads).
//   the counts      placed / unplaced / truncated are wave-uniform: a wave keeps them in registers and adds the non-zero ones
//                   at its end, three global atomics a wave at most.
//   mnc_lca_clade   direct is scattered into tin order (mnc_lca_scatter), scan.h's exclusive_scan runs over it, and
//                   clade[v] = S[tout[v]] - S[tin[v]]: a subtree is a run of the pre-order.  Three small launches and no tree
//                   walk, whatever the depth.
// Integer arithmetic throughout; no host wait in an add.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <new>
#include <vector>
#include "ab_common.h"
#include "scan.h"

using namespace mnc;

constexpr int LCA_WG_PER_CU = 2;               // (see LDS above)
constexpr int LCA_PLACED = 0, LCA_UNPLACED = 1, LCA_TRUNCATED = 2, LCA_N = 4;   // uint64 words of `ctr`
constexpr int64_t LCA_MAX_READS = (1LL << 31) - 1;

struct mnc_lca : mnc::Accum {
	int n_contigs = 0, G = 0, n_nodes = 0, n_cu = 1;
	int32_t max_delta = 0;
	int64_t cap_reads = 0;
	int32_t *parent = nullptr, *tin = nullptr, *tout = nullptr;   // [n_nodes] each, one allocation
	int64_t *direct = nullptr;                 // [n_nodes]
	int32_t *node = nullptr;                   // [cap_reads]
	unsigned long long *ctr = nullptr;         // [LCA_N]
	// scratch of the clade read-out
	int64_t *euler = nullptr;                  // [n_nodes] direct in tin order
	int64_t *runs = nullptr;                   // [n_nodes + 1] its exclusive scan
	int64_t *sums = nullptr;                   // the scan's tile sums
	int64_t *clade = nullptr;                  // [n_nodes]
};

namespace mnc {

struct LcaView {
	const int32_t *parent, *tin, *tout;
	int n_nodes, n_genomes, max_delta;
	int64_t *direct;
	int32_t *node;
	unsigned long long *ctr;
};

struct LcaCarry {
	const int2 *head, *slots;
	int width;
	int64_t first, n;
};

template <int SRC, bool LDS>
__global__ __launch_bounds__(256) void mnc_lca_add(Batch B, int n_contigs, LcaCarry C, LcaView T)
{
	__shared__ int32_t s_parent[LDS ? MNC_LCA_LDS_NODES : 1], s_tin[LDS ? MNC_LCA_LDS_NODES : 1], s_tout[LDS ? MNC_LCA_LDS_NODES : 1];
	__shared__ uint32_t s_direct[LDS ? MNC_LCA_LDS_NODES : 1];
	if (LDS) {
		for (int v = threadIdx.x; v < T.n_nodes; v += blockDim.x) s_parent[v] = T.parent[v], s_tin[v] = T.tin[v], s_tout[v] = T.tout[v], s_direct[v] = 0;
		__syncthreads();
	}
	const int32_t *parent = LDS ? s_parent : T.parent, *tin = LDS ? s_tin : T.tin, *tout = LDS ? s_tout : T.tout;
	const int lane = lane_id();
	const int64_t n_reads = SRC ? C.n : (int64_t)B.n_reads, stride = (int64_t)gridDim.x * (blockDim.x >> 6);
	unsigned long long n_placed = 0, n_unplaced = 0, n_truncated = 0;   // of this wave (wave-uniform)
	for (int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_reads; r += stride) {   // (whole waves; no barrier inside)
		unsigned long long lo = ~0ull;
		int hi = -1;
		bool truncated = false;
		if (SRC) {
			const int2 h = C.head[C.first + r];
			if (h.y & CARRY_USED) {
				const int2 p = lane < C.width ? C.slots[(C.first + r) * C.width + lane] : make_int2(-1, 0);
				if (p.x >= 0 && p.x < T.n_genomes && (long long)h.x - p.y <= T.max_delta) {
					hi = tin[p.x];
					lo = (unsigned long long)(uint32_t)hi << 32 | (uint32_t)p.x;
				}
				truncated = (h.y & CARRY_TRUNCATED) != 0;
			}
		} else {
			const int n = B.n_reg[r];
			const int64_t slot0 = reg_slot(B, (uint32_t)r);
			int best;
			if (n > 0 && ab_best(B, slot0, n, n_contigs, T.n_genomes, best)) {
				for (int i = lane; i < n; i += 64) {
					const mnc_reg_t &x = B.regs[slot0 + i];
					if (!ab_counted(B, x, n_contigs) || (long long)best - x.dp_max > T.max_delta) continue;
					const int g = B.contig_genome[x.rid];
					if (g < 0 || g >= T.n_genomes) continue;
					const int t = tin[g];
					const unsigned long long k = (unsigned long long)(uint32_t)t << 32 | (uint32_t)g;
					lo = k < lo ? k : lo, hi = t > hi ? t : hi;
				}
			}
		}
		lo = ab_wave_min(lo);
		for (int d = 32; d > 0; d >>= 1) {
			const int o = __shfl_xor(hi, d);
			hi = o > hi ? o : hi;
		}
		// ---- the climb: from the node of the smallest tin to the first ancestor whose subtree ends behind the largest
		int v = -1;
		if (lo != ~0ull) {
			v = (int)(uint32_t)lo;
			for (int s = 1; s < MNC_LCA_MAX_DEPTH && tout[v] <= hi; ++s) v = parent[v];   // (the root's tout is n_nodes: it ends the climb)
		}
		n_placed += v >= 0, n_unplaced += v < 0, n_truncated += truncated;
		if (lane == 0) {
			T.node[(SRC ? C.first : 0) + r] = v;
			if (v >= 0) {
				if (LDS) atomicAdd(&s_direct[v], 1u);
				else (void)__hip_atomic_fetch_add(T.direct + v, (int64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			}
		}
	}
	const unsigned long long mine = lane == LCA_PLACED ? n_placed : lane == LCA_UNPLACED ? n_unplaced : n_truncated;
	if (lane < 3 && mine) (void)__hip_atomic_fetch_add(T.ctr + lane, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (LDS) {
		__syncthreads();
		for (int v = threadIdx.x; v < T.n_nodes; v += blockDim.x)
			if (s_direct[v]) (void)__hip_atomic_fetch_add(T.direct + v, (int64_t)s_direct[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// ---------------------------------------------------------------- the clade read-out
__global__ __launch_bounds__(256) void mnc_lca_scatter(const int64_t *direct, const int32_t *tin, int n_nodes, int64_t *euler)
{
	const int v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v < n_nodes) euler[tin[v]] = direct[v];                // (tin is a permutation of 0 .. n_nodes - 1)
}

// runs: the exclusive scan over direct in tin order, runs[n_nodes] the total
__global__ __launch_bounds__(256) void mnc_lca_clade(const int64_t *runs, const int32_t *tin, const int32_t *tout, int n_nodes, int64_t *clade)
{
	const int v = blockIdx.x * blockDim.x + threadIdx.x;
	if (v < n_nodes) clade[v] = runs[tout[v]] - runs[tin[v]];
}

// ---------------------------------------------------------------- the engine's side (mnc_engine_add_lca, engine.hip)
const Accum *as_accum(const mnc_lca *lc) { return lc; }

// MNC_ERR_RANGE, before anything is touched, when the batch holds more reads than the node store
int lca_fits(const mnc_lca *lc, const Batch &B)
{
	if ((int64_t)B.n_reads <= lc->cap_reads) return MNC_OK;
	set_error("the batch holds %lld reads, the lca accumulator was created for %lld (cap_reads)", (long long)B.n_reads, (long long)lc->cap_reads);
	return MNC_ERR_RANGE;
}

// n reads from source SRC on `st`: the persistent grid, the instantiation by the tree's size
template <int SRC>
static void lca_launch(const mnc_lca *lc, const Batch &B, const LcaCarry &C, int64_t n, hipStream_t st)
{
	const LcaView T{lc->parent, lc->tin, lc->tout, lc->n_nodes, lc->G, (int)lc->max_delta, lc->direct, lc->node, lc->ctr};
	const unsigned wg = (unsigned)std::max<int64_t>(1, std::min<int64_t>((int64_t)lc->n_cu * LCA_WG_PER_CU, (n + 3) / 4));
	if (lc->n_nodes <= MNC_LCA_LDS_NODES) hipLaunchKernelGGL((mnc_lca_add<SRC, true>), dim3(wg), dim3(256), 0, st, B, lc->n_contigs, C, T);
	else hipLaunchKernelGGL((mnc_lca_add<SRC, false>), dim3(wg), dim3(256), 0, st, B, lc->n_contigs, C, T);
}

// the batch B, as it stands in HBM, on the engine's stream `st`; an empty batch is an add of no reads
int lca_add(mnc_lca *lc, const Batch &B, hipStream_t st)
{
	return lc->add(st, [&] {
		if (B.n_reads) lca_launch<0>(lc, B, LcaCarry{nullptr, nullptr, 0, 0, 0}, B.n_reads, st);
	});
}

} // namespace mnc

// ---------------------------------------------------------------- the tree, on the host
// parent[] checked (the message names the node), then numbered by one DFS from the root, children in ascending id
static int lca_tree(const int32_t *parent, int32_t n_genomes, int32_t n_nodes, std::vector<int32_t> &tin, std::vector<int32_t> &tout)
{
	if (n_genomes < 0 || n_nodes < n_genomes) { set_error("n_nodes %d below n_genomes %d (the genomes are nodes 0 .. n_genomes - 1)", n_nodes, n_genomes); return MNC_ERR_ARG; }
	if (n_nodes && !parent) return MNC_ERR_ARG;
	int root = -1;
	for (int v = 0; v < n_nodes; ++v) {
		if (parent[v] < -1 || parent[v] >= n_nodes) { set_error("node %d: parent %d outside -1 .. %d", v, parent[v], n_nodes - 1); return MNC_ERR_ARG; }
		if (parent[v] != -1) continue;
		if (root >= 0) { set_error("nodes %d and %d are both roots", root, v); return MNC_ERR_ARG; }
		root = v;
	}
	if (root < 0) { set_error("no node is the root (parent -1)"); return MNC_ERR_ARG; }
	// the children of every node, ascending: a counting sort by parent
	std::vector<int32_t> first((size_t)n_nodes + 1, 0), child((size_t)n_nodes), depth((size_t)n_nodes, 0);
	for (int v = 0; v < n_nodes; ++v)
		if (v != root) ++first[(size_t)parent[v] + 1];
	for (int v = 0; v < n_nodes; ++v) first[(size_t)v + 1] += first[(size_t)v];
	{
		std::vector<int32_t> at(first.begin(), first.end() - 1);
		for (int v = 0; v < n_nodes; ++v)
			if (v != root) child[(size_t)at[(size_t)parent[v]]++] = v;
	}
	tin.assign((size_t)n_nodes, -1), tout.assign((size_t)n_nodes, -1);
	std::vector<int32_t> stack{root}, next(first.begin(), first.end() - 1);
	int32_t clock = 0;
	tin[(size_t)root] = clock++, depth[(size_t)root] = 1;
	while (!stack.empty()) {
		const int v = stack.back();
		if (next[(size_t)v] < first[(size_t)v + 1]) {
			const int c = child[(size_t)next[(size_t)v]++];
			tin[(size_t)c] = clock++, depth[(size_t)c] = depth[(size_t)v] + 1;
			stack.push_back(c);
		} else {
			tout[(size_t)v] = clock;
			stack.pop_back();
		}
	}
	// a node the root does not reach hangs on a cycle: walk up into it (n_nodes steps are enough) and name its smallest node
	for (int v = 0; v < n_nodes; ++v) {
		if (tin[(size_t)v] >= 0) continue;
		int c = v;
		for (int s = 0; s < n_nodes; ++s) c = parent[c];
		int least = c;
		for (int x = parent[c]; x != c; x = parent[x]) least = std::min(least, x);
		set_error("node %d is its own ancestor", least);
		return MNC_ERR_ARG;
	}
	for (int v = 0; v < n_nodes; ++v)
		if (depth[(size_t)v] > MNC_LCA_MAX_DEPTH) {
			set_error("node %d lies %d levels deep, the root included; a line holds at most %d (MNC_LCA_MAX_DEPTH)", v, depth[(size_t)v], MNC_LCA_MAX_DEPTH);
			return MNC_ERR_ARG;
		}
	return MNC_OK;
}

// the counters as they stand behind everything queued so far
static int lca_counters(mnc_lca *lc, unsigned long long *c)
{
	HIP_TRY(hipSetDevice(lc->device));
	HIP_TRY(hipMemcpyAsync(c, lc->ctr, LCA_N * 8, hipMemcpyDeviceToHost, lc->st));
	HIP_TRY(hipStreamSynchronize(lc->st));
	return MNC_OK;
}

// ---------------------------------------------------------------- C-ABI
extern "C" void mnc_lca_free(mnc_lca *lc)
{
	if (!lc) return;
	lc->release();
	delete lc;
}

extern "C" int mnc_lca_create(mnc_index *idx, int device, int32_t n_genomes, const int32_t *parent, int32_t n_nodes, int32_t max_delta, int64_t cap_reads, mnc_lca **out)
{
	if (!out) return MNC_ERR_ARG;
	*out = nullptr;
	if (idx && n_genomes != (int32_t)idx->genome_name.size()) {
		set_error("n_genomes %d, the index holds %d genomes", n_genomes, (int)idx->genome_name.size());
		return MNC_ERR_ARG;
	}
	std::vector<int32_t> tin, tout;
	try {
		if (int rc = lca_tree(parent, n_genomes, n_nodes, tin, tout)) return rc;
	} catch (const std::bad_alloc &) { return MNC_ERR_NOMEM; }
	if (max_delta < 0) { set_error("max_delta %d: max_delta >= 0 is required", max_delta); return MNC_ERR_ARG; }
	if (cap_reads < 1 || cap_reads > LCA_MAX_READS) { set_error("cap_reads %lld outside 1 .. %lld", (long long)cap_reads, (long long)LCA_MAX_READS); return MNC_ERR_ARG; }
	mnc_lca *lc = new (std::nothrow) mnc_lca;
	if (!lc) return MNC_ERR_NOMEM;
	if (int rc = check_device(device)) { delete lc; return rc; }
	lc->n_contigs = idx ? (int)idx->contig_len.size() : 0, lc->G = n_genomes, lc->n_nodes = n_nodes;
	lc->max_delta = max_delta, lc->cap_reads = cap_reads;
	const size_t nn = (size_t)n_nodes;
	hipError_t he = lc->begin(idx, device);
	if (he == hipSuccess) he = hipDeviceGetAttribute(&lc->n_cu, hipDeviceAttributeMultiprocessorCount, device);
	lc->alloc(he, (void**)&lc->parent, nn * 12);
	lc->alloc(he, (void**)&lc->direct, nn * 8);
	lc->alloc(he, (void**)&lc->node, (size_t)cap_reads * 4);
	lc->alloc(he, (void**)&lc->ctr, LCA_N * 8);
	lc->alloc(he, (void**)&lc->euler, nn * 8);
	lc->alloc(he, (void**)&lc->runs, (nn + 1) * 8);
	lc->alloc(he, (void**)&lc->sums, (nn / SC_TILE + 2) * 8);
	lc->alloc(he, (void**)&lc->clade, nn * 8);
	lc->streams(he);
	if (he == hipSuccess) lc->tin = lc->parent + nn, lc->tout = lc->tin + nn, lc->n_cu = std::max(lc->n_cu, 1);
	if (he == hipSuccess) he = hipMemcpy(lc->parent, parent, nn * 4, hipMemcpyHostToDevice);
	if (he == hipSuccess) he = hipMemcpy(lc->tin, tin.data(), nn * 4, hipMemcpyHostToDevice);
	if (he == hipSuccess) he = hipMemcpy(lc->tout, tout.data(), nn * 4, hipMemcpyHostToDevice);
	if (he != hipSuccess) {
		set_error("lca accumulator of %d nodes (44 bytes each) and %lld reads (4 bytes each): %s", n_nodes, (long long)cap_reads, hipGetErrorString(he));
		const int rc = Accum::failed(he);
		mnc_lca_free(lc);
		return rc;
	}
	if (int rc = mnc_lca_reset(lc)) { mnc_lca_free(lc); return rc; }
	*out = lc;
	return MNC_OK;
}

extern "C" int mnc_lca_reset(mnc_lca *lc)
{
	if (!lc) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(lc->device));
	std::lock_guard<std::mutex> g(lc->mu);
	HIP_TRY(hipMemsetAsync(lc->direct, 0, (size_t)lc->n_nodes * 8, lc->st));
	HIP_TRY(hipMemsetAsync(lc->node, 0xff, (size_t)lc->cap_reads * 4, lc->st));
	HIP_TRY(hipMemsetAsync(lc->ctr, 0, LCA_N * 8, lc->st));
	HIP_TRY(lc->own_done());
	return MNC_OK;
}

extern "C" int mnc_lca_device_bytes(const mnc_lca *lc, int64_t *bytes) { return accum_device_bytes(lc, bytes); }

extern "C" int mnc_lca_info(mnc_lca *lc, int64_t *n_placed, int64_t *n_unplaced, int64_t *n_truncated)
{
	if (!lc) return MNC_ERR_ARG;
	unsigned long long c[LCA_N];
	if (int rc = lca_counters(lc, c)) return rc;
	if (n_placed) *n_placed = (int64_t)c[LCA_PLACED];
	if (n_unplaced) *n_unplaced = (int64_t)c[LCA_UNPLACED];
	if (n_truncated) *n_truncated = (int64_t)c[LCA_TRUNCATED];
	return MNC_OK;
}

// The rows [first_read, first_read + n_reads) of a carry, each as one read, as mnc_abundance_add_carry takes them: the one
// wait is for the carry's largest genome id (every check comes before anything is added); the add itself is queued on the
// accumulator's stream.
extern "C" int mnc_lca_add_carry(mnc_lca *lc, mnc_carry *cc, int64_t first_read, int64_t n_reads)
{
	if (!lc || !cc) return MNC_ERR_ARG;
	if (first_read < 0 || n_reads < 0) { set_error("rows [%lld, + %lld): a range of reads", (long long)first_read, (long long)n_reads); return MNC_ERR_ARG; }
	if (cc->device != lc->device) { set_error("the carry is on device %d, the accumulator on device %d", cc->device, lc->device); return MNC_ERR_ARG; }
	if (cc->max_delta != lc->max_delta) { set_error("the carry was cut at max_delta %d, the accumulator's is %d", cc->max_delta, lc->max_delta); return MNC_ERR_ARG; }
	if (n_reads > cc->cap || first_read > cc->cap - n_reads) {
		set_error("rows [%lld, %lld) of a carry of %lld", (long long)first_read, (long long)(first_read + n_reads), (long long)cc->cap);
		return MNC_ERR_RANGE;
	}
	if (n_reads > lc->cap_reads || first_read > lc->cap_reads - n_reads) {
		set_error("rows [%lld, %lld), the lca accumulator was created for %lld reads (cap_reads)", (long long)first_read, (long long)(first_read + n_reads), (long long)lc->cap_reads);
		return MNC_ERR_RANGE;
	}
	unsigned long long s[4];
	if (int rc = carry_stats(cc, s)) return rc;
	if ((int64_t)s[3] > lc->G) { set_error("the carry holds genome id %lld, the accumulator has %d genomes", (long long)s[3] - 1, lc->G); return MNC_ERR_ARG; }
	if (n_reads == 0) return MNC_OK;
	HIP_TRY(hipSetDevice(lc->device));
	std::lock_guard<std::mutex> lk(lc->mu);
	if (int rc = carry_read_begin(cc, lc->st)) return rc;
	lca_launch<1>(lc, Batch{}, LcaCarry{cc->head, cc->slots, (int)cc->width, first_read, n_reads}, n_reads, lc->st);
	HIP_TRY(hipGetLastError());
	HIP_TRY(lc->own_done());                                   // an engine's add, and whatever changes the carry, comes behind it
	return carry_read_end(cc, lc->ev_own);
}

extern "C" int mnc_lca_fetch(mnc_lca *lc, int64_t *direct, int64_t *clade)
{
	if (!lc) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(lc->device));
	const size_t b = (size_t)lc->n_nodes * 8;
	if (clade) {
		const unsigned wg = (unsigned)((lc->n_nodes + 255) / 256);
		hipLaunchKernelGGL(mnc_lca_scatter, dim3(wg), dim3(256), 0, lc->st, lc->direct, lc->tin, lc->n_nodes, lc->euler);
		exclusive_scan(ScanInPlain<int64_t>{lc->euler}, lc->n_nodes, lc->runs, lc->sums, lc->st);
		hipLaunchKernelGGL(mnc_lca_clade, dim3(wg), dim3(256), 0, lc->st, lc->runs, lc->tin, lc->tout, lc->n_nodes, lc->clade);
	}
	return lc->finish(hipSuccess, nullptr, {direct, lc->direct, b}, {clade, lc->clade, b}, "lca counts");
}

extern "C" int mnc_lca_fetch_nodes(mnc_lca *lc, int64_t first, int64_t n, int32_t *out)
{
	if (!lc) return MNC_ERR_ARG;
	if (first < 0 || n < 0 || first > lc->cap_reads || n > lc->cap_reads - first) {
		set_error("reads [%lld, %lld) outside the %lld of the accumulator (cap_reads)", (long long)first, (long long)(first + n), (long long)lc->cap_reads);
		return MNC_ERR_ARG;
	}
	if (n == 0) return MNC_OK;
	if (!out) return MNC_ERR_ARG;
	HIP_TRY(hipSetDevice(lc->device));
	return lc->finish(hipSuccess, nullptr, {out, lc->node + first, (size_t)n * 4}, {}, "lca nodes");
}

extern "C" int mnc_lca_device(mnc_lca *lc, const int64_t **d_direct, const int32_t **d_node)
{
	if (!lc) return MNC_ERR_ARG;
	if (d_direct) *d_direct = lc->direct;
	if (d_node) *d_node = lc->node;
	return MNC_OK;
}
