// What the library's translation units share on the host side and the C-ABI does not show ("The modules
// beside tagdig.hip"): the hooks into the handle that tagdig.hip defines, the check macro for HIP calls, the owners of the
// device buffers, pinned buffers, events and streams that the handle keeps or an entry point holds while it runs (nothing
// else in the library frees one), and the base of a module's state on the handle.  Every module beside tagdig.hip includes
// this header; tagdig.hip includes it too, so that a hook's definition is checked against the declaration its callers see.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tagdig.h"

struct td_piece_sink;                             // piece_sink.hpp

#define TD_HIDDEN __attribute__((visibility("hidden")))
extern "C" {
// tagdig.hip: the calling thread's error slot (returns `code`) and the index td_last_bad_index reports
TD_HIDDEN int td_fail_internal(int code, const char *msg);
TD_HIDDEN void td_set_bad_index(uint32_t idx);
// tagdig.hip: the handle's device, work stream and CU count; its options "md5_piece" and "tagnet_max_compares"; the
// number of staging threads
TD_HIDDEN int td_handle_device(const td_handle *h);
TD_HIDDEN void *td_handle_work_stream(const td_handle *h);
TD_HIDDEN int td_handle_num_cu(const td_handle *h);
TD_HIDDEN uint64_t td_handle_md5_piece(const td_handle *h);
TD_HIDDEN uint64_t td_handle_tagnet_max_compares(const td_handle *h);
TD_HIDDEN int td_stage_thread_count(void);
// tagdig.hip: every launch enqueued through this handle (they may be on its own streams) has finished
TD_HIDDEN int td_handle_wait_work(td_handle *h);
// tagdig.hip, for the streaming modules (stream_pass.hpp): the barcode + cut-site index by td_set_index's rules; terminators
// before the end of every 16 KiB tile -> *prefix (the handle's scratch, good until its next launch), their total ->
// *d_total, asynchronous on `s`; a file's pieces through the handle's readers to `sink`; the option "max_grid" (0: not set)
TD_HIDDEN int td_barcut_blob(const char *const *barcut, uint32_t n_barcut, uint32_t barnum, const uint32_t *tagoff, std::vector<uint8_t> &blob,
                             uint32_t *off_bmeta, uint32_t *off_bdir);
TD_HIDDEN int td_line_prefix(td_handle *h, const void *d_fastq, uint64_t nbytes, void *s, const uint64_t **prefix, unsigned long long *d_total);
TD_HIDDEN int td_stream_file(td_handle *h, const char *path, uint64_t max_reads, const td_piece_sink *sink);
TD_HIDDEN uint32_t td_handle_max_grid(const td_handle *h);
// tagdig.hip: the options "qc_flush_tiles" (qc.hip), "place_max_compares" (place.hip) and "rescue_max_run" (rescue.hip); 0: not set
TD_HIDDEN uint32_t td_handle_qc_flush_tiles(const td_handle *h);
TD_HIDDEN uint64_t td_handle_place_max_compares(const td_handle *h);
TD_HIDDEN uint32_t td_handle_rescue_max_run(const td_handle *h);
}

// a failed HIP call ends the calling function with TD_E_HIP and "<the call as written>: <HIP's text>"
#define TD_HIPCHK(call)                                                                      \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return td_fail_internal(TD_E_HIP, (std::string(#call) + ": " + hipGetErrorString(e_)).c_str()); \
    } while (0)

namespace [[gnu::visibility("hidden")]] tdi {

// max(n, 1) elements of device memory, freed with the object unless released
template <typename T> struct DevBuf {
    T *p = nullptr; size_t n = 0;                 // n: the elements asked for
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t want) {               // (of an empty buffer)
        const hipError_t e = hipMalloc(&p, std::max<size_t>(want, 1) * sizeof(T));
        if (e == hipSuccess) n = want; else p = nullptr;
        return e;
    }
    // room for `want` elements: grows only, and what the buffer held is gone after a growth
    hipError_t ensure(size_t want) {
        if (want <= n && p) return hipSuccess;
        reset();
        return alloc(want);
    }
    void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }        // free now
    T *release() { T *q = p; p = nullptr; n = 0; return q; }              // hand off: the caller frees
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(n, o.n); }
};

// the same in pinned host memory
template <typename T> struct PinBuf {
    T *p = nullptr;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { reset(); }
    hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault) { return hipHostMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T), flags); }
    void reset() { if (p) (void)hipHostFree(p); p = nullptr; }
};

// one event, created with the flags its use needs; movable, for the handle's pool of timing events
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
};

// a non-blocking stream; its work is waited for before it goes, so an owner declared behind the buffers its work uses
// (and so destroyed before them) never lets one be freed under a running kernel or copy
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

// N events, destroyed with the object
template <int N> struct Events {
    hipEvent_t e[N] = {};
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    hipError_t create() {                         // in order; stops at the first error
        for (hipEvent_t &x : e) {
            const hipError_t err = hipEventCreate(&x);
            if (err != hipSuccess) return err;
        }
        return hipSuccess;
    }
    float elapsed(int a, int b) const {           // device ms from e[a] to e[b], both completed (0 where HIP cannot tell)
        float f = 0;
        return hipEventElapsedTime(&f, e[a], e[b]) == hipSuccess ? f : 0.0f;
    }
};

// What a module keeps on the handle between its entry points derives from this.  The handle holds one per slot in a
// std::unique_ptr declared behind its streams: td_destroy frees a state left open like every other member, and a module
// resets its slot at its end and at a second begin.
struct ModuleState { virtual ~ModuleState() = default; };
enum ModuleSlot { CENSUS, QC, PLACES, RESCUE, BCRESCUE, MODULE_SLOTS };
std::unique_ptr<ModuleState> &module_slot(td_handle *h, ModuleSlot which);      // tagdig.hip
template <typename T> T *state_of(td_handle *h, ModuleSlot which) { return h ? static_cast<T *>(module_slot(h, which).get()) : nullptr; }

}  // namespace tdi
