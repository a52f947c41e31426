// The streaming pass written once ("The modules beside tagdig.hip"): what census.hip, qc.hip, rescue.hip and
// bcrescue.hip share on the host side around their one persistent kernel over 16 KiB tiles.  A module's state derives from
// tdi::StreamPass and supplies its launch and its zeroing; everything a module does differently it passes as an argument
// or keeps in its own file -- nothing in here asks which module is calling.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "piece_sink.hpp"
#include "td_internal.hpp"

namespace [[gnu::visibility("hidden")]] tdi {

constexpr uint32_t STREAM_TILE = 16384;           // td_line_prefix's tile (the modules assert that theirs is this one)

// the device idle, then the slot empty: how td_<mod>_begin and td_<mod>_end start
inline int quiet_reset(td_handle *h, ModuleSlot which) {
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    TD_HIPCHK(hipDeviceSynchronize());
    module_slot(h, which).reset();
    return TD_OK;
}

// no state on the handle: TD_E_STATE, or TD_E_ARG with `arg_text` where it is an argument that is missing
inline int no_state(const char *mod, bool args_ok, const char *arg_text = "NULL argument") {
    if (!args_ok) return td_fail_internal(TD_E_ARG, arg_text);
    return td_fail_internal(TD_E_STATE, (std::string("td_") + mod + "_begin has not been called").c_str());
}

struct StreamPass : ModuleState {
    td_handle *h = nullptr;
    uint32_t bblob_bytes = 0, off_bmeta = 0, off_bdir = 0;
    DevBuf<uint32_t> d_bblob;                     // the barcode + cut-site index as the kernel copies it into LDS
    bool used = false;                            // something has been added since td_<mod>_begin
    int dead = 0;                                 // the code every call answers with after a failure, until td_<mod>_begin
    std::string dead_msg;

    // one buffer through the module's kernel (the readers' pieces come here too), and its results back to zero on `s`
    virtual int launch(const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, hipStream_t stream,
                       const unsigned long long *cursor_in, unsigned long long *cursor_out) = 0;
    virtual int zero(hipStream_t s) = 0;

    // ---- begin: the index by td_set_index's rules, refused beyond the module's share of a workgroup's LDS, in device memory
    int begin(td_handle *handle, const char *const *barcut, uint32_t n_barcut, uint32_t barnum, const uint32_t *tagoff, size_t lds_budget) {
        h = handle;
        std::vector<uint8_t> blob;
        const int rc = td_barcut_blob(barcut, n_barcut, barnum, tagoff, blob, &off_bmeta, &off_bdir); if (rc) return rc;
        if (blob.size() > lds_budget) return td_fail_internal(TD_E_LIMIT, "barcode index does not fit the LDS budget");
        return upload(blob);
    }
    // what the kernel copies into LDS, into device memory (a module that appends to the index calls this itself)
    int upload(const std::vector<uint8_t> &blob) {
        bblob_bytes = (uint32_t)blob.size();
        hipError_t e = d_bblob.alloc((blob.size() + 3) / 4);
        if (e == hipSuccess) e = hipMemcpy(d_bblob.p, blob.data(), blob.size(), hipMemcpyHostToDevice);
        return e == hipSuccess ? TD_OK : hip_failed(e);
    }
    static int hip_failed(hipError_t e) { (void)hipGetLastError(); return td_fail_internal(TD_E_HIP, hipGetErrorString(e)); }
    // the results zeroed and nothing added: the end of begin, and what a reader asks for before it reads a .gz file again
    int restart() {
        const hipStream_t s = (hipStream_t)td_handle_work_stream(h);
        const int rc = zero(s); if (rc) return rc;
        TD_HIPCHK(hipStreamSynchronize(s));
        used = false;
        return TD_OK;
    }

    // ---- launch: ntiles == 0 with TD_OK says that there is nothing to do; *d_total takes the buffer's terminators
    int prologue(const void *d_fastq, uint64_t nbytes, uint64_t &max_reads, hipStream_t stream, unsigned long long *d_total,
                 const uint64_t *&prefix, uint32_t &ntiles) {
        ntiles = 0;
        if (dead) return answer_dead();
        if (((uintptr_t)d_fastq & 15) != 0) return td_fail_internal(TD_E_ARG, "device FASTQ pointer must be 16-byte aligned");
        if (nbytes == 0) return TD_OK;
        if (max_reads == 0) max_reads = 1;
        used = true;
        const int rc = td_line_prefix(h, d_fastq, nbytes, (void *)stream, &prefix, d_total); if (rc) return rc;
        ntiles = (uint32_t)((nbytes + STREAM_TILE - 1) / STREAM_TILE);
        return TD_OK;
    }
    // last read line that is looked at: ordinal r (1-based) sits on line 4 (r - 1) + 1
    static uint64_t limit_line(uint64_t max_reads) { return max_reads >= (1ull << 60) ? ~0ull - 8 : 4 * (max_reads - 1) + 1; }
    // persistent workgroups: per_cu of them on every CU, no more than tiles, and where `capped` within the option "max_grid"
    uint32_t grid(uint32_t ntiles, uint32_t per_cu, bool capped) const {
        const uint32_t g = (uint32_t)std::min<uint64_t>(ntiles, (uint64_t)td_handle_num_cu(h) * per_cu), cap = capped ? td_handle_max_grid(h) : 0;
        return cap ? std::min(g, cap) : g;
    }

    // ---- the latch
    int answer_dead() const { return td_fail_internal(dead, dead_msg.c_str()); }
    int latch(int code, const std::string &msg) { dead = code; dead_msg = msg; return answer_dead(); }
    // after a synchronisation: the module's n words on the host, words[err_at] its error word; what else that word may say
    // the module reads itself
    int sync_words(unsigned long long *words, const unsigned long long *d_words, size_t n, size_t err_at) {
        if (dead) return answer_dead();
        TD_HIPCHK(hipDeviceSynchronize());
        TD_HIPCHK(hipMemcpy(words, d_words, n * 8, hipMemcpyDeviceToHost));
        return words[err_at] & tdk::ERR_NONASCII ? latch(TD_E_NONASCII, "non-ASCII byte in a sequence line") : TD_OK;
    }

    // ---- a file through the handle's readers, which are asked for reader_reads reads
    static int sink_piece(void *ctx, const void *d, uint64_t n, uint64_t first_line, uint64_t max_reads, hipStream_t s, const unsigned long long *cin,
                          unsigned long long *cout) {
        return ((StreamPass *)ctx)->launch(d, n, first_line, max_reads, s, cin, cout);
    }
    static int sink_restart(void *ctx) { return ((StreamPass *)ctx)->restart(); }
    int file(const char *path, uint64_t reader_reads) {
        if (dead) return answer_dead();
        const td_piece_sink sink{sink_piece, sink_restart, this, !used};
        const int rc = td_stream_file(h, path, reader_reads, &sink);
        if (rc && used && !dead) { dead = rc; dead_msg = td_last_error(); }      // the results hold a part of the file: never handed out
        return rc;
    }
};

// the end of td_<mod>_begin: the new state, zeroed, goes onto the handle
template <typename T> int install(std::unique_ptr<T> &state, ModuleSlot which) {
    const int rc = state->restart(); if (rc) return rc;
    module_slot(state->h, which) = std::move(state);
    return TD_OK;
}

}  // namespace tdi
