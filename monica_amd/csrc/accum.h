// The host side that the accumulators beside the engine share (k_coverage.hip, k_pileup.hip, k_abundance.hip): whose they
// are, what they hold on the device, and how their work is ordered against the engines'.  An accumulator is a struct that
// derives from Accum and adds its own buffers, kernels and read-outs.
//
// Ordering.  Adds run on the engines' streams, from the engines' threads; reset, the read-outs and whatever else the
// accumulator does on its own run on `st`, one thread at a time.  ev_add: the last add (`st` waits for it); ev_own: the last
// own work that an add must come behind (a reset; an add waits for it).  `mu` keeps one thread's record-and-wait of an
// event in one piece.  Nothing here waits on the host.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <new>
#include <vector>
#include "common.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
	mnc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
	return e_ == hipErrorOutOfMemory ? MNC_ERR_NOMEM : MNC_ERR_HIP; } } while (0)

namespace mnc {

int check_device(int device);                  // engine.hip

struct Accum {
	mnc_index *idx = nullptr;
	int device = 0;
	int64_t bytes = 0;                         // of the device allocations below
	std::mutex mu;
	hipStream_t st = nullptr;
	hipEvent_t ev_add = nullptr, ev_own = nullptr;
	std::vector<void*> bufs;                   // the device allocations, as `alloc` made them
	bool serial = false;                       // adds run one behind the other on the device: each waits for the last one's event

	// ---- creation: begin, alloc per buffer, streams.  `he`, the creating function's own, keeps the first failure and every
	// step behind it is skipped; release() undoes whatever was made
	hipError_t begin(mnc_index *index, int dev) { idx = index, device = dev; return hipSetDevice(dev); }
	void alloc(hipError_t &he, void **p, size_t n)
	{
		*p = nullptr;
		if (he != hipSuccess) return;
		n = n ? n : 8;
		try {
			bufs.reserve(bufs.size() + 1);
		} catch (const std::bad_alloc &) { he = hipErrorOutOfMemory; return; }
		he = hipMalloc(p, n);
		if (he == hipSuccess) bufs.push_back(*p), bytes += (int64_t)n; else *p = nullptr;
	}
	void streams(hipError_t &he)
	{
		if (he == hipSuccess) he = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
		if (he == hipSuccess) he = hipEventCreateWithFlags(&ev_add, hipEventDisableTiming);
		if (he == hipSuccess) he = hipEventCreateWithFlags(&ev_own, hipEventDisableTiming);
	}
	// the code of a creation that failed with `he` (the caller has set the message)
	static int failed(hipError_t he)
	{
		(void)hipGetLastError();
		return he == hipErrorOutOfMemory ? MNC_ERR_NOMEM : MNC_ERR_HIP;
	}
	void release()
	{
		(void)hipSetDevice(device);
		if (st) (void)hipStreamSynchronize(st);
		for (void *p : bufs) (void)hipFree(p);
		if (ev_add) (void)hipEventDestroy(ev_add);
		if (ev_own) (void)hipEventDestroy(ev_own);
		if (st) (void)hipStreamDestroy(st);
	}

	// ---- an engine's add: `launch` queues the kernels on the engine's stream `on`
	template <class F>
	int add(hipStream_t on, F launch)
	{
		std::lock_guard<std::mutex> lk(mu);
		HIP_TRY(hipStreamWaitEvent(on, ev_own, 0));             // behind the last reset
		if (serial) HIP_TRY(hipStreamWaitEvent(on, ev_add, 0)); // ... and behind the last add, whichever engine's it was
		launch();
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipEventRecord(ev_add, on));
		HIP_TRY(hipStreamWaitEvent(st, ev_add, 0));             // reset and the read-outs come after it
		return MNC_OK;
	}
	// own work that an add must come behind has been queued on `st` (the caller holds `mu`)
	hipError_t own_done() { return hipEventRecord(ev_own, st); }

	// ---- what a read-out leaves on the host: up to two pieces of the device buffer `tmp`, behind the kernels queued on
	// `st`; `tmp` is freed.  e: what queuing them gave so far.  A piece without a dst is left out.  The message is
	// "<fmt, ...>: <the HIP error>".
	struct Piece { void *dst; const void *src; size_t bytes; };
	__attribute__((format(printf, 6, 7))) int finish(hipError_t e, void *tmp, Piece a, Piece b, const char *fmt, ...)
	{
		if (e == hipSuccess) e = hipGetLastError();
		for (const Piece &p : { a, b })
			if (e == hipSuccess && p.dst) e = hipMemcpyAsync(p.dst, p.src, p.bytes, hipMemcpyDeviceToHost, st);
		const hipError_t hs = hipStreamSynchronize(st);
		if (e == hipSuccess) e = hs;
		(void)hipFree(tmp);
		if (e == hipSuccess) return MNC_OK;
		char what[128];
		va_list ap;
		va_start(ap, fmt);
		vsnprintf(what, sizeof(what), fmt, ap);
		va_end(ap);
		set_error("%s: %s", what, hipGetErrorString(e));
		return MNC_ERR_HIP;
	}
};

inline int accum_device_bytes(const Accum *a, int64_t *bytes)
{
	if (!a || !bytes) return MNC_ERR_ARG;
	*bytes = a->bytes;
	return MNC_OK;
}

// [start, end) of contig rid, the contigs' first words in `off` (one more than there are contigs)
inline int accum_interval(const std::vector<int64_t> &off, int rid, int64_t start, int64_t end)
{
	if (rid < 0 || rid >= (int)off.size() - 1) { set_error("contig %d out of range", rid); return MNC_ERR_ARG; }
	const int64_t len = off[rid + 1] - off[rid];
	if (start < 0 || end < start || end > len) {
		set_error("interval [%lld, %lld) outside contig %d of %lld bases", (long long)start, (long long)end, rid, (long long)len);
		return MNC_ERR_ARG;
	}
	return MNC_OK;
}

} // namespace mnc
