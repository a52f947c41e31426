// The seam between the file readers of tagdig.hip and a consumer other than the count kernels (csrc/census.hip):
// while a handle's sink is set (td_stream_file), every piece a reader has brought into device memory goes to
// `piece` instead of launch_count -- same arguments, same stream, the line index carried from piece to piece in
// device memory (cursor_in: lines consumed by the pieces before; cursor_out: that plus this piece's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct td_piece_sink {
    int (*piece)(void *ctx, const void *d_fastq, uint64_t nbytes, uint64_t first_line, uint64_t max_reads, hipStream_t stream,
                 const unsigned long long *cursor_in, unsigned long long *cursor_out);
    int (*restart)(void *ctx);                // forget what the pieces so far added (a .gz file is read again by the reference's rules)
    void *ctx;
    bool fresh;                               // nothing had been added before this file
};
