// MD5 (RFC 1321) of many messages at once (include/tagdig.h: td_md5_device, td_md5_files) -- the checksums that
// writeMD5sums (reference tagdigger_fun.py:1370-1386) computes for the files a split leaves behind.
//
// MD5 cannot be split inside one message: every 64-byte block starts from the state the block before left.  The
// messages are independent, so one lane owns one message.
//
// k_md5_update  lane j takes job j = (where its run of whole 64-byte blocks lies, how many, which message), loads the
//    message's state (4 x u32, resident on the device between launches), runs the blocks, stores the state.  The 64
//    steps are unrolled with their constants as literals; the next block's words are requested before the current
//    block's steps (two register sets, a scheduling barrier behind the loads) so that no load sits on the dependent chain.  MD5's words are little-endian, the device's order.
//    ALIGNED: the run starts on a 16-byte boundary (the slabs td_md5_files stages); otherwise dword loads of the
//    enclosing words and a funnel shift (a message anywhere in a caller's buffer, td_md5_device).
//    Workgroups are one wave: the waves of one launch spread over the CUs.
// k_md5_tail    td_md5_device only: lane i lays out message i's last len % 64 bytes, 0x80, the zeros and the bit length
//    as one or two more blocks in a scratch buffer (the bytes are on the device; the host knows only the lengths).
//
// td_md5_files pads on the host, where the file lengths are known: a file's padded stream is cut into pieces of P bytes
// (a multiple of 64), and a round carries one piece of every file that still has one through one of two pinned slots:
// staging threads read round r + 1 while round r is on the device, and the upload of round r + 1 (a stream of its own)
// runs beside the kernel of round r.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "td_internal.hpp"

namespace {

struct Md5Job {
    uint64_t off;       // bytes from the slab's start to the run's first block
    uint32_t nblocks;   // whole 64-byte blocks in the run
    uint32_t msg;       // whose state
};

constexpr uint32_t MD5_INIT[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
constexpr uint64_t MD5_PIECE = (uint64_t)1 << 20;          // bytes a file contributes per round
constexpr uint64_t MD5_SLOT_BUDGET = (uint64_t)384 << 20;  // a slot never exceeds this: longer lists take smaller pieces

__device__ __forceinline__ uint32_t rol(uint32_t x, int s) { return __builtin_rotateleft32(x, s); }
#define MD5_F(b, c, d) ((d) ^ ((b) & ((c) ^ (d))))
#define MD5_G(b, c, d) ((c) ^ ((d) & ((b) ^ (c))))
#define MD5_H(b, c, d) ((b) ^ (c) ^ (d))
#define MD5_I(b, c, d) ((c) ^ ((b) | ~(d)))
#define MD5_STEP(f, a, b, c, d, m, k, s) a = b + rol(a + f(b, c, d) + (m) + (k), s)

__device__ __forceinline__ void md5_block(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, const uint32_t (&m)[16]) {
    const uint32_t A = a, B = b, C = c, D = d;
    MD5_STEP(MD5_F, a, b, c, d, m[0], 0xd76aa478u, 7);   MD5_STEP(MD5_F, d, a, b, c, m[1], 0xe8c7b756u, 12);
    MD5_STEP(MD5_F, c, d, a, b, m[2], 0x242070dbu, 17);  MD5_STEP(MD5_F, b, c, d, a, m[3], 0xc1bdceeeu, 22);
    MD5_STEP(MD5_F, a, b, c, d, m[4], 0xf57c0fafu, 7);   MD5_STEP(MD5_F, d, a, b, c, m[5], 0x4787c62au, 12);
    MD5_STEP(MD5_F, c, d, a, b, m[6], 0xa8304613u, 17);  MD5_STEP(MD5_F, b, c, d, a, m[7], 0xfd469501u, 22);
    MD5_STEP(MD5_F, a, b, c, d, m[8], 0x698098d8u, 7);   MD5_STEP(MD5_F, d, a, b, c, m[9], 0x8b44f7afu, 12);
    MD5_STEP(MD5_F, c, d, a, b, m[10], 0xffff5bb1u, 17); MD5_STEP(MD5_F, b, c, d, a, m[11], 0x895cd7beu, 22);
    MD5_STEP(MD5_F, a, b, c, d, m[12], 0x6b901122u, 7);  MD5_STEP(MD5_F, d, a, b, c, m[13], 0xfd987193u, 12);
    MD5_STEP(MD5_F, c, d, a, b, m[14], 0xa679438eu, 17); MD5_STEP(MD5_F, b, c, d, a, m[15], 0x49b40821u, 22);

    MD5_STEP(MD5_G, a, b, c, d, m[1], 0xf61e2562u, 5);   MD5_STEP(MD5_G, d, a, b, c, m[6], 0xc040b340u, 9);
    MD5_STEP(MD5_G, c, d, a, b, m[11], 0x265e5a51u, 14); MD5_STEP(MD5_G, b, c, d, a, m[0], 0xe9b6c7aau, 20);
    MD5_STEP(MD5_G, a, b, c, d, m[5], 0xd62f105du, 5);   MD5_STEP(MD5_G, d, a, b, c, m[10], 0x02441453u, 9);
    MD5_STEP(MD5_G, c, d, a, b, m[15], 0xd8a1e681u, 14); MD5_STEP(MD5_G, b, c, d, a, m[4], 0xe7d3fbc8u, 20);
    MD5_STEP(MD5_G, a, b, c, d, m[9], 0x21e1cde6u, 5);   MD5_STEP(MD5_G, d, a, b, c, m[14], 0xc33707d6u, 9);
    MD5_STEP(MD5_G, c, d, a, b, m[3], 0xf4d50d87u, 14);  MD5_STEP(MD5_G, b, c, d, a, m[8], 0x455a14edu, 20);
    MD5_STEP(MD5_G, a, b, c, d, m[13], 0xa9e3e905u, 5);  MD5_STEP(MD5_G, d, a, b, c, m[2], 0xfcefa3f8u, 9);
    MD5_STEP(MD5_G, c, d, a, b, m[7], 0x676f02d9u, 14);  MD5_STEP(MD5_G, b, c, d, a, m[12], 0x8d2a4c8au, 20);

    MD5_STEP(MD5_H, a, b, c, d, m[5], 0xfffa3942u, 4);   MD5_STEP(MD5_H, d, a, b, c, m[8], 0x8771f681u, 11);
    MD5_STEP(MD5_H, c, d, a, b, m[11], 0x6d9d6122u, 16); MD5_STEP(MD5_H, b, c, d, a, m[14], 0xfde5380cu, 23);
    MD5_STEP(MD5_H, a, b, c, d, m[1], 0xa4beea44u, 4);   MD5_STEP(MD5_H, d, a, b, c, m[4], 0x4bdecfa9u, 11);
    MD5_STEP(MD5_H, c, d, a, b, m[7], 0xf6bb4b60u, 16);  MD5_STEP(MD5_H, b, c, d, a, m[10], 0xbebfbc70u, 23);
    MD5_STEP(MD5_H, a, b, c, d, m[13], 0x289b7ec6u, 4);  MD5_STEP(MD5_H, d, a, b, c, m[0], 0xeaa127fau, 11);
    MD5_STEP(MD5_H, c, d, a, b, m[3], 0xd4ef3085u, 16);  MD5_STEP(MD5_H, b, c, d, a, m[6], 0x04881d05u, 23);
    MD5_STEP(MD5_H, a, b, c, d, m[9], 0xd9d4d039u, 4);   MD5_STEP(MD5_H, d, a, b, c, m[12], 0xe6db99e5u, 11);
    MD5_STEP(MD5_H, c, d, a, b, m[15], 0x1fa27cf8u, 16); MD5_STEP(MD5_H, b, c, d, a, m[2], 0xc4ac5665u, 23);

    MD5_STEP(MD5_I, a, b, c, d, m[0], 0xf4292244u, 6);   MD5_STEP(MD5_I, d, a, b, c, m[7], 0x432aff97u, 10);
    MD5_STEP(MD5_I, c, d, a, b, m[14], 0xab9423a7u, 15); MD5_STEP(MD5_I, b, c, d, a, m[5], 0xfc93a039u, 21);
    MD5_STEP(MD5_I, a, b, c, d, m[12], 0x655b59c3u, 6);  MD5_STEP(MD5_I, d, a, b, c, m[3], 0x8f0ccc92u, 10);
    MD5_STEP(MD5_I, c, d, a, b, m[10], 0xffeff47du, 15); MD5_STEP(MD5_I, b, c, d, a, m[1], 0x85845dd1u, 21);
    MD5_STEP(MD5_I, a, b, c, d, m[8], 0x6fa87e4fu, 6);   MD5_STEP(MD5_I, d, a, b, c, m[15], 0xfe2ce6e0u, 10);
    MD5_STEP(MD5_I, c, d, a, b, m[6], 0xa3014314u, 15);  MD5_STEP(MD5_I, b, c, d, a, m[13], 0x4e0811a1u, 21);
    MD5_STEP(MD5_I, a, b, c, d, m[4], 0xf7537e82u, 6);   MD5_STEP(MD5_I, d, a, b, c, m[11], 0xbd3af235u, 10);
    MD5_STEP(MD5_I, c, d, a, b, m[2], 0x2ad7d2bbu, 15);  MD5_STEP(MD5_I, b, c, d, a, m[9], 0xeb86d391u, 21);
    a += A; b += B; c += C; d += D;
}

// the 16 words of the block at `p` (ALIGNED: p is 16-byte aligned; else any address: the words that enclose the block,
// shifted into place -- the 17th word is read only when the block does not end on a word boundary, so no byte beyond the
// word that holds the block's last byte is touched)
template <bool ALIGNED>
__device__ __forceinline__ void md5_load(const uint8_t *p, uint32_t (&m)[16]) {
    if (ALIGNED) {
        const uint4 *q = (const uint4 *)p;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint4 w = q[k];
            m[4 * k] = w.x; m[4 * k + 1] = w.y; m[4 * k + 2] = w.z; m[4 * k + 3] = w.w;
        }
    } else {
        const uint32_t sh = ((uint32_t)(uintptr_t)p & 3u) * 8u;
        const uint32_t *q = (const uint32_t *)(p - ((uintptr_t)p & 3u));
        uint32_t w[17];
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = q[k];
        w[16] = sh ? q[16] : 0u;
#pragma unroll
        for (int k = 0; k < 16; k++) m[k] = (uint32_t)((((uint64_t)w[k + 1] << 32) | w[k]) >> sh);
    }
}

template <bool ALIGNED>
__global__ __launch_bounds__(64) void k_md5_update(const uint8_t *__restrict__ slab, const Md5Job *__restrict__ jobs,
                                                   uint32_t njobs, uint32_t *__restrict__ state) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= njobs) return;
    const Md5Job job = jobs[j];
    if (job.nblocks == 0) return;
    uint32_t *st = state + 4 * (size_t)job.msg;
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
    // Two register sets take turns, the loop unrolled by two: while the steps run on one, the other receives the block
    // after it.  The loads are branch-free (past the run's end the last block is read again and not used) and there is no
    // exit between a load and the steps it overlaps, so the compiler has nowhere to sink it to; a scheduling barrier
    // behind the loads keeps the instruction scheduler from moving them down into the steps.  They are issued before
    // step 1 and have the whole block's ~1 400 cycles to arrive in.
    const uint8_t *p = slab + job.off;
    const uint8_t *const last = p + 64 * (size_t)(job.nblocks - 1);
    uint32_t x[16], y[16];
    uint32_t n = job.nblocks;
    md5_load<ALIGNED>(p, x);
    for (; n >= 2; n -= 2, p += 128) {
        md5_load<ALIGNED>(p + 64, y);
        __builtin_amdgcn_sched_barrier(0);
        md5_block(a, b, c, d, x);
        md5_load<ALIGNED>(p + 128 <= last ? p + 128 : last, x);
        __builtin_amdgcn_sched_barrier(0);
        md5_block(a, b, c, d, y);
    }
    if (n) md5_block(a, b, c, d, x);
    st[0] = a; st[1] = b; st[2] = c; st[3] = d;
}

// message i's last (len & 63) bytes and its padding -> tails[128 i ..): one block when the bytes leave room for 0x80 and
// the length (at most 55), else two; jobs[i] says how many
__global__ __launch_bounds__(64) void k_md5_tail(const uint8_t *__restrict__ data, const uint64_t *__restrict__ offs, uint32_t n,
                                                 uint8_t *__restrict__ tails, Md5Job *__restrict__ jobs) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint64_t len = offs[i + 1] - offs[i];
    const uint32_t rem = (uint32_t)(len & 63u), total = rem < 56u ? 64u : 128u;
    const uint8_t *src = data + offs[i] + (len - rem);
    uint8_t *dst = tails + 128 * (size_t)i;
    const uint64_t bits = len << 3;
    for (uint32_t k = 0; k < total; k++) {
        uint8_t v = 0;
        if (k < rem) v = src[k];
        else if (k == rem) v = 0x80;
        else if (k >= total - 8u) v = (uint8_t)(bits >> (8u * (k - (total - 8u))));
        dst[k] = v;
    }
    jobs[i] = Md5Job{128 * (uint64_t)i, total / 64u, i};
}

hipError_t init_states(uint32_t *d_state, uint32_t n) {
    std::vector<uint32_t> init(4 * (size_t)n);
    for (size_t i = 0; i < n; i++) memcpy(&init[4 * i], MD5_INIT, 16);
    return hipMemcpy(d_state, init.data(), init.size() * 4, hipMemcpyHostToDevice);
}

inline uint32_t waves(uint32_t lanes) { return (lanes + 63u) / 64u; }

// length of a message of `len` bytes once padded: the next multiple of 64 that leaves room for 0x80 and 8 length bytes
inline uint64_t padded_len(uint64_t len) { return (len + 8) / 64 * 64 + 64; }

// bytes [a, b) of the padded stream of a message of `len` bytes that lie behind its data (a >= len) -> dst
void fill_padding(uint8_t *dst, uint64_t a, uint64_t b, uint64_t len) {
    const uint64_t total = padded_len(len), bits = len << 3;
    memset(dst, 0, (size_t)(b - a));
    if (a <= len && len < b) dst[len - a] = 0x80;
    for (uint64_t k = std::max(a, total - 8); k < b; k++) dst[k - a] = (uint8_t)(bits >> (8 * (k - (total - 8))));
}

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

extern "C" int td_md5_device(td_handle *h, const void *d_data, const uint64_t *offs, uint32_t n, uint8_t *digests, double *ms) {
    if (!h || !offs || (n && !digests)) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (ms) *ms = 0.0;
    if (n == 0) return TD_OK;
    bool aligned = ((uintptr_t)d_data & 15u) == 0;
    uint64_t whole = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (offs[i + 1] < offs[i]) return td_fail_internal(TD_E_ARG, "offsets decrease");
        if ((offs[i + 1] - offs[i]) >> 61) return td_fail_internal(TD_E_LIMIT, "message of 2^61 bytes or more");
        if (offs[i] & 15u) aligned = false;
        whole += (offs[i + 1] - offs[i]) / 64;
    }
    if (offs[n] && !d_data) return td_fail_internal(TD_E_ARG, "NULL data");
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    std::vector<Md5Job> jobs(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t nb = (offs[i + 1] - offs[i]) / 64;
        if (nb > 0xffffffffull) return td_fail_internal(TD_E_LIMIT, "message of 256 GiB or more");
        jobs[i] = Md5Job{offs[i], (uint32_t)nb, i};
    }
    tdi::DevBuf<uint32_t> d_state; tdi::DevBuf<Md5Job> d_jobs, d_tjobs; tdi::DevBuf<uint64_t> d_offs; tdi::DevBuf<uint8_t> d_tails;
    tdi::Events<2> ev;
    TD_HIPCHK(d_state.alloc(4 * (size_t)n));
    TD_HIPCHK(d_jobs.alloc(n));
    TD_HIPCHK(d_tjobs.alloc(n));
    TD_HIPCHK(d_offs.alloc((size_t)n + 1));
    TD_HIPCHK(d_tails.alloc(128 * (size_t)n));
    TD_HIPCHK(ev.create());
    TD_HIPCHK(init_states(d_state.p, n));
    TD_HIPCHK(hipMemcpy(d_jobs.p, jobs.data(), n * sizeof(Md5Job), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(d_offs.p, offs, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    if (whole) {
        if (aligned) k_md5_update<true><<<waves(n), 64, 0, 0>>>((const uint8_t *)d_data, d_jobs.p, n, d_state.p);
        else k_md5_update<false><<<waves(n), 64, 0, 0>>>((const uint8_t *)d_data, d_jobs.p, n, d_state.p);
        TD_HIPCHK(hipGetLastError());
    }
    k_md5_tail<<<waves(n), 64, 0, 0>>>((const uint8_t *)d_data, d_offs.p, n, d_tails.p, d_tjobs.p);
    TD_HIPCHK(hipGetLastError());
    k_md5_update<true><<<waves(n), 64, 0, 0>>>(d_tails.p, d_tjobs.p, n, d_state.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[1]));
    if (ms) *ms = ev.elapsed(0, 1);
    TD_HIPCHK(hipMemcpy(digests, d_state.p, 16 * (size_t)n, hipMemcpyDeviceToHost));
    return TD_OK;
}

extern "C" int td_md5_files(td_handle *h, const char *const *paths, uint32_t n, uint8_t *digests, uint32_t *bad_index,
                            double ms[3]) {
    if (!h || (n && (!paths || !digests))) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (ms) ms[0] = ms[1] = ms[2] = 0.0;
    if (bad_index) *bad_index = 0;
    if (n == 0) return TD_OK;
    auto io_fail = [&](uint32_t i, const char *what, int err) {
        if (bad_index) *bad_index = i;
        return td_fail_internal(TD_E_IO, (std::string(what) + " " + paths[i] + ": " + strerror(err)).c_str());
    };
    // lengths first: the first file that cannot be opened ends the call before any work
    std::vector<uint64_t> len(n), total(n), done(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (!paths[i]) return td_fail_internal(TD_E_ARG, "NULL path");
        const int fd = open(paths[i], O_RDONLY | O_CLOEXEC);
        if (fd < 0) return io_fail(i, "cannot open", errno);
        struct stat sb;
        const int rc = fstat(fd, &sb), err = errno;
        close(fd);
        if (rc != 0) return io_fail(i, "cannot stat", err);
        if (S_ISDIR(sb.st_mode)) return io_fail(i, "cannot read", EISDIR);
        len[i] = (uint64_t)sb.st_size;
        total[i] = padded_len(len[i]);
    }
    uint64_t P = td_handle_md5_piece(h);
    if (!P) P = std::max<uint64_t>(64, std::min(MD5_PIECE, MD5_SLOT_BUDGET / n / 64 * 64));
    uint64_t cap = 0;                       // the largest round: every file's first piece
    for (uint32_t i = 0; i < n; i++) cap += std::min(P, total[i]);

    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    struct Slot {
        tdi::PinBuf<uint8_t> pin; tdi::PinBuf<Md5Job> pin_jobs; tdi::DevBuf<uint8_t> dev; tdi::DevBuf<Md5Job> dev_jobs;
        tdi::Event up; tdi::Events<2> k; bool busy = false;         // up: no timing; k: around the kernel
    } slot[2];
    tdi::DevBuf<uint32_t> d_state;
    // two streams: the upload of round r + 1 runs beside the kernel of round r (an event orders a round's kernel
    // behind its upload; a slot is refilled only after its kernel is through)
    tdi::Stream kernel_stream, copy_stream;     // (declared behind the buffers: waited for and destroyed before those are freed)
    TD_HIPCHK(kernel_stream.create());
    TD_HIPCHK(copy_stream.create());
    const hipStream_t st = kernel_stream.s, sc = copy_stream.s;
    TD_HIPCHK(d_state.alloc(4 * (size_t)n));
    TD_HIPCHK(init_states(d_state.p, n));
    for (auto &s : slot) {
        TD_HIPCHK(s.pin.alloc(cap));
        TD_HIPCHK(s.pin_jobs.alloc(n));
        TD_HIPCHK(s.dev.alloc(cap));
        TD_HIPCHK(s.dev_jobs.alloc(n));
        TD_HIPCHK(s.up.create(hipEventDisableTiming));
        TD_HIPCHK(s.k.create());
    }
    auto retire = [&](Slot &s) -> hipError_t {          // wait until the slot's kernel is through; book its time
        if (!s.busy) return hipSuccess;
        const double t0 = now_ms();
        const hipError_t e = hipEventSynchronize(s.k.e[1]);
        if (ms) { ms[1] += now_ms() - t0; ms[2] += s.k.elapsed(0, 1); }
        s.busy = false;
        return e;
    };

    struct Task { uint32_t file; uint64_t a, b; uint8_t *dst; };     // bytes [a, b) of the file's padded stream
    std::vector<Task> tasks;
    std::atomic<uint32_t> bad{UINT32_MAX};
    std::atomic<int> bad_errno{0};
    auto run_task = [&](const Task &t) {
        const uint64_t data_end = std::min(t.b, std::max(t.a, len[t.file]));
        if (data_end > t.a) {
            const int fd = open(paths[t.file], O_RDONLY | O_CLOEXEC);
            int err = fd < 0 ? errno : 0;
            uint64_t at = t.a;
            while (fd >= 0 && at < data_end) {
                const ssize_t got = pread(fd, t.dst + (at - t.a), (size_t)(data_end - at), (off_t)at);
                if (got < 0 && errno == EINTR) continue;
                if (got <= 0) { err = got < 0 ? errno : EIO; break; }      // (0: the file shrank under us)
                at += (uint64_t)got;
            }
            if (fd >= 0) close(fd);
            if (err) {
                uint32_t seen = bad.load();
                while (t.file < seen && !bad.compare_exchange_weak(seen, t.file)) {}
                if (bad.load() == t.file) bad_errno = err;
                return;
            }
        }
        if (t.b > data_end) fill_padding(t.dst + (data_end - t.a), data_end, t.b, len[t.file]);
    };

    const int nthreads = td_stage_thread_count();
    for (uint32_t round = 0;; round++) {
        Slot &s = slot[round & 1];
        TD_HIPCHK(retire(s));
        tasks.clear();
        uint64_t used = 0;
        uint32_t njobs = 0;
        for (uint32_t i = 0; i < n; i++) {
            if (done[i] == total[i]) continue;
            const uint64_t a = done[i], b = std::min(total[i], a + P);
            s.pin_jobs.p[njobs++] = Md5Job{used, (uint32_t)((b - a) / 64), i};
            tasks.push_back(Task{i, a, b, s.pin.p + used});
            used += b - a;
            done[i] = b;
        }
        if (!njobs) break;
        const double t0 = now_ms();
        std::atomic<size_t> next{0};
        auto worker = [&]() { for (size_t k; (k = next.fetch_add(1)) < tasks.size();) run_task(tasks[k]); };
        std::vector<std::thread> pool;
        const int nt = (int)std::min<uint64_t>({(uint64_t)nthreads, (uint64_t)tasks.size(), (used >> 20) + 1});
        for (int t = 1; t < nt; t++) pool.emplace_back(worker);
        worker();
        for (auto &th : pool) th.join();
        if (ms) ms[0] += now_ms() - t0;
        if (bad.load() != UINT32_MAX) return io_fail(bad.load(), "cannot read", bad_errno.load());
        TD_HIPCHK(hipMemcpyAsync(s.dev.p, s.pin.p, used, hipMemcpyHostToDevice, sc));
        TD_HIPCHK(hipMemcpyAsync(s.dev_jobs.p, s.pin_jobs.p, njobs * sizeof(Md5Job), hipMemcpyHostToDevice, sc));
        TD_HIPCHK(hipEventRecord(s.up.e, sc));
        TD_HIPCHK(hipStreamWaitEvent(st, s.up.e, 0));
        TD_HIPCHK(hipEventRecord(s.k.e[0], st));
        k_md5_update<true><<<waves(njobs), 64, 0, st>>>(s.dev.p, s.dev_jobs.p, njobs, d_state.p);
        TD_HIPCHK(hipGetLastError());
        TD_HIPCHK(hipEventRecord(s.k.e[1], st));
        s.busy = true;
    }
    for (auto &s : slot) TD_HIPCHK(retire(s));
    TD_HIPCHK(hipMemcpyAsync(digests, d_state.p, 16 * (size_t)n, hipMemcpyDeviceToHost, st));
    TD_HIPCHK(hipStreamSynchronize(st));
    return TD_OK;
}
