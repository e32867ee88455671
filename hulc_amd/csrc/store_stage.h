// hulc_amd/csrc/store_stage.h — hulc_store_stage / hulc_store_stage_join / hulc_store_stage_stats (include/hulc_hip.h): the host tier of a two-tier
// frame store.  The frames of a split that do not fit into HBM stay in pinned host memory; the windows of the NEXT batch that lie there are copied
// into staging slots at the tail of the store's device allocation while the current step computes, and conv1 gathers them from the slots by index
// like any resident window.
//
// The copies are hipMemcpyAsync calls on a private non-blocking stream, so they run on the SDMA engines and occupy no CU: the persistent recurrences
// (rnn_persist.h) need every CU co-resident, and a copy kernel on a side stream would hold CUs for milliseconds while it waits on PCIe.  The stream is
// ordered against the engine's by events only (the pattern of comm.h), never by a host synchronisation:
//   * stage(): the copy stream first waits for everything enqueued on the engine stream so far — the previous readers of the slots (forward AND
//     backward: conv1's weight gradient re-reads the frames) — then takes the n copies, then records the ticket's event,
//   * join(): the engine stream waits for that event.
// A bounded ring of event pairs backs the tickets; a ticket whose pair has been recycled cannot be joined any more.
//
// Errors.  Every argument is checked before anything is enqueued: a call refused for its arguments leaves nothing behind.  A RUNTIME failure (a
// hipMemcpyAsync or an event call that fails partway through the list) is different: the copies enqueued before it stay enqueued, the call returns
// -1 and issues no ticket, so the slots named by the list may be PARTLY overwritten and there is nothing to join.  What was enqueued still runs
// behind the gate, so no earlier reader is disturbed; the caller must not run a batch that reads those slots (FrameStore.stage releases the handle
// and raises).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hulc_hip.h"

void hulc_set_error(const char* fmt, ...);

struct StoreStager {
    enum { RING = HULC_STAGE_TICKETS };
    hipStream_t cs = nullptr;                                  // the copy stream
    hipEvent_t gate[RING] = {}, done[RING] = {};               // ticket t uses pair t % RING
    int64_t next_ticket = 1;                                   // tickets are > 0
    int64_t n_calls = 0, n_copies = 0, n_bytes = 0;

    ~StoreStager() {
        if (cs) hipStreamSynchronize(cs);
        for (int i = 0; i < RING; ++i) { if (gate[i]) hipEventDestroy(gate[i]); if (done[i]) hipEventDestroy(done[i]); }
        if (cs) hipStreamDestroy(cs);
    }
    bool prepare() {
        if (cs) return true;
        if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) { cs = nullptr; (void)hipGetLastError(); hulc_set_error("hulc_store_stage: stream creation failed"); return false; }
        return true;
    }
    // 0 = not usable, 1 = pinned host, 2 = device memory of device `dev`.  A pageable pointer is either unknown to the runtime (an error, cleared
    // here) or "unregistered"; memory of another device is not usable either: the slots and their readers live on the context's device
    static int kind_of(const void* p, int dev) {
        if (!p) return 0;
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
        if (a.type == hipMemoryTypeHost) return 1;
        if (a.type == hipMemoryTypeDevice) return a.device == dev ? 2 : 0;
        return 0;
    }
    // [p, p + bytes) inside ONE allocation known to the runtime (device memory, or a pinned host buffer)
    static bool range_ok(const void* p, int64_t bytes) {
        hipDeviceptr_t base = nullptr; size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return false; }
        const char* b = (const char*)base; const char* q = (const char*)p;
        return q >= b && (uint64_t)bytes <= (uint64_t)size && (uint64_t)(q - b) <= (uint64_t)size - (uint64_t)bytes;
    }
    // the device of the engine's stream (the null stream: the current device)
    static int device_of(hipStream_t st) {
        int dev = 0;
        if (hipStreamGetDevice(st, &dev) == hipSuccess) return dev;
        (void)hipGetLastError();
        if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return -1; }
        return dev;
    }
    int64_t stage(hipStream_t st, const hulc_stage_copy* c, int32_t n) {
        if (!c || n < 1) { hulc_set_error("hulc_store_stage: needs n >= 1 copies (got %d)", (int)n); return -1; }
        // every argument is checked before anything is enqueued
        int64_t total = 0;
        const int dev = device_of(st);
        for (int i = 0; i < n; ++i) {
            if (c[i].bytes <= 0) { hulc_set_error("hulc_store_stage: copy %d has bytes = %lld", i, (long long)c[i].bytes); return -1; }
            const int ks = kind_of(c[i].src, dev), kd = kind_of(c[i].dst, dev);
            if (ks == 0) { hulc_set_error("hulc_store_stage: src of copy %d is neither pinned host memory nor memory of the context's device", i); return -1; }
            if (kd != 2) { hulc_set_error("hulc_store_stage: dst of copy %d is not memory of the context's device", i); return -1; }
            if (!range_ok(c[i].dst, c[i].bytes) || !range_ok(c[i].src, c[i].bytes)) {
                hulc_set_error("hulc_store_stage: copy %d leaves its allocation (src: the pinned buffer or device allocation, dst: the device allocation)", i); return -1; }
            total += c[i].bytes;
        }
        if (!prepare()) return -1;
        const int k = (int)(next_ticket % RING);
        if (!gate[k] && (hipEventCreateWithFlags(&gate[k], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&done[k], hipEventDisableTiming) != hipSuccess)) {
            (void)hipGetLastError(); hulc_set_error("hulc_store_stage: event creation failed"); return -1; }
        if (hipEventRecord(gate[k], st) != hipSuccess || hipStreamWaitEvent(cs, gate[k], 0) != hipSuccess) { (void)hipGetLastError(); hulc_set_error("hulc_store_stage: gating the copy stream failed"); return -1; }
        hipError_t e = hipSuccess;
        for (int i = 0; i < n && e == hipSuccess; ++i) e = hipMemcpyAsync(c[i].dst, c[i].src, (size_t)c[i].bytes, hipMemcpyDefault, cs);
        // the event is recorded even after a failed copy, so that whatever was enqueued stays ordered before the ticket's readers
        const hipError_t er = hipEventRecord(done[k], cs);
        if (e != hipSuccess || er != hipSuccess) { (void)hipGetLastError(); hulc_set_error("hulc_store_stage: %s", hipGetErrorString(e != hipSuccess ? e : er)); return -1; }
        n_calls += 1; n_copies += n; n_bytes += total;
        return next_ticket++;
    }
    int join(hipStream_t st, int64_t ticket) {
        if (ticket < 1 || ticket >= next_ticket) { hulc_set_error("hulc_store_stage_join: ticket %lld was never issued", (long long)ticket); return 1; }
        if (ticket + RING <= next_ticket) { hulc_set_error("hulc_store_stage_join: ticket %lld has been recycled (the ring holds the last %d)", (long long)ticket, (int)RING); return 1; }
        if (hipStreamWaitEvent(st, done[ticket % RING], 0) != hipSuccess) { (void)hipGetLastError(); hulc_set_error("hulc_store_stage_join: stream wait failed"); return 1; }
        return 0;
    }
};
