// Tag Manager on the GPU (include/tagdig.h: td_tagset_load, td_tagset_lookup, td_tagset_varsites, td_tagset_free).
//
// K1 k_tag_pack: one thread per tag turns its ASCII bases into W = ceil(maxlen / 32) 64-bit words, 2 bits per base
//    (A 0, C 1, G 2, T 3), first base in the top bits, padded with A; plus the length.  With the length as a tie-break
//    the order of (words, length) is Python's str order on ACGT strings ("AC" < "ACA" < "ACAA").  A byte outside ACGT
//    is flagged, not packed.  Keys are word-major (key[w * n + i]) so a lane's reads of one word coalesce.
// K2 the stable LSD radix sort of the tag permutation by (words, length), 8 bits per pass (radix_sort.hpp, shared with
//    tagnet.hip).  The permutation starts in the names' code-point order (the host ranks the names), so stability gives
//    sorted(zip(seqs, names)).  k_rs_gather then lays the keys out in sorted order for K3.
// K3 k_tag_lookup: one thread per query, the reference's lookupMarkerByTag walk (tagdigger_fun.py:1674-1706) as four
//    indices f, a, b, c (see the header).  Every block the walk crosses is contiguous in the sorted set (a run of
//    duplicates, the strings that start with q, each run of prefixes of q), so each is one binary search: at most
//    len(q) + 4 searches of log2(n) steps, whatever the duplicates.
// K4 k_tag_varsites: one wave per group of tags; lane l owns columns l, l + 64, l + 128, l + 192 and ORs a one-hot of
//    the base each tag has there; a column is variable when two bits are set.  Ballots make the 4 x 64-bit mask.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "radix_sort.hpp"
#include "td_internal.hpp"

struct td_tagset {
    int device;
    uint32_t n, W;
    tdi::DevBuf<uint64_t> key;     // W * n words, sorted order, word-major
    tdi::DevBuf<uint16_t> len;     // n, sorted order
};

namespace {

constexpr int TS_MAXW = TD_TAGSET_MAX_LEN / 32;   // 8 words

// ------------------------------------------------------------------ K1
__device__ __forceinline__ uint32_t ts_code(uint32_t c, bool *bad) {
    const uint32_t v = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
    if (v == 4u) *bad = true;
    return v & 3u;
}

__global__ __launch_bounds__(256) void k_tag_pack(const uint8_t *seqs, const uint64_t *offs, uint32_t n, uint32_t W,
                                                  uint64_t *key, uint16_t *len, uint32_t *bad_first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = offs[i], e = offs[i + 1];
    const uint32_t L = (uint32_t)(e - s);          // <= 32 W, checked by the host
    bool bad = false;
    for (uint32_t w = 0; w < W; ++w) {
        uint64_t v = 0;
        const uint32_t b0 = w * 32;
        for (uint32_t k = 0; k < 32; ++k) {
            const uint32_t p = b0 + k;
            const uint64_t c = p < L ? ts_code(seqs[s + p], &bad) : 0u;
            v |= c << (62 - 2 * k);
        }
        key[(uint64_t)w * n + i] = v;
    }
    len[i] = (uint16_t)L;
    if (bad) atomicMin(bad_first, i);
}

// ------------------------------------------------------------------ K2 (the sort itself: radix_sort.hpp)
__global__ __launch_bounds__(256) void k_rs_gather(const uint64_t *key, const uint16_t *len, const uint32_t *perm, uint32_t n,
                                                   uint32_t W, uint64_t *skey, uint16_t *slen) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = perm[i];
    for (uint32_t w = 0; w < W; ++w) skey[(uint64_t)w * n + i] = key[(uint64_t)w * n + v];
    slen[i] = len[v];
}

// ------------------------------------------------------------------ K3
struct Query {
    uint64_t w[TS_MAXW];
    uint32_t L, W;
};

struct SetView {
    const uint64_t *key;
    const uint16_t *len;
    uint32_t n, W;
    __device__ __forceinline__ uint64_t word(uint32_t j, uint32_t w) const { return w < W ? key[(uint64_t)w * n + j] : 0ull; }
};

// the first L bases of S[j] and q agree (both are at least L long: the caller checks)
__device__ __forceinline__ bool pre_eq(const SetView &S, uint32_t j, const Query &q, uint32_t L) {
#pragma unroll
    for (int w = 0; w < TS_MAXW; ++w) {
        const uint32_t b0 = 32u * w;
        if (b0 >= L) break;
        const uint64_t x = S.word(j, w) ^ q.w[w];
        const uint32_t k = L - b0;
        const uint64_t m = k >= 32 ? ~0ull : ~0ull << (64 - 2 * k);
        if (x & m) return false;
    }
    return true;
}
// S[j] compared with q: -1, 0, 1
__device__ __forceinline__ int cmp_q(const SetView &S, uint32_t j, const Query &q) {
    const uint32_t W = S.W > q.W ? S.W : q.W;
#pragma unroll
    for (int w = 0; w < TS_MAXW; ++w) {
        if ((uint32_t)w >= W) break;
        const uint64_t a = S.word(j, w), b = q.w[w];
        if (a != b) return a < b ? -1 : 1;
    }
    const uint32_t l = S.len[j];
    return l < q.L ? -1 : l > q.L ? 1 : 0;
}
__device__ __forceinline__ bool eq_q(const SetView &S, uint32_t j, const Query &q) {
    return S.len[j] == q.L && pre_eq(S, j, q, q.L);
}
__device__ __forceinline__ bool starts_q(const SetView &S, uint32_t j, const Query &q) {   // S[j].startswith(q)
    return S.len[j] >= q.L && pre_eq(S, j, q, q.L);
}
__device__ __forceinline__ bool q_starts(const SetView &S, uint32_t j, const Query &q) {   // q.startswith(S[j])
    const uint32_t l = S.len[j];
    return l <= q.L && pre_eq(S, j, q, l);
}
__device__ __forceinline__ bool set_eq(const SetView &S, uint32_t i, uint32_t j) {
    if (S.len[i] != S.len[j]) return false;
    for (uint32_t w = 0; w < S.W; ++w)
        if (S.key[(uint64_t)w * S.n + i] != S.key[(uint64_t)w * S.n + j]) return false;
    return true;
}
// first index of the run of duplicates that ends at t (S[j] == S[t] is false, then true, on [0, t])
__device__ __forceinline__ uint32_t run_first(const SetView &S, uint32_t t) {
    uint32_t lo = 0, hi = t;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (set_eq(S, mid, t)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_tag_lookup(const uint64_t *skey, const uint16_t *slen, uint32_t n, uint32_t W,
                                                    const uint64_t *qkey, const uint16_t *qlen, uint32_t nq, uint32_t Wq,
                                                    int adl, int4 *out) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    const SetView S{skey, slen, n, W};
    Query q;
    q.L = qlen[qi];
    q.W = Wq;
#pragma unroll
    for (int w = 0; w < TS_MAXW; ++w) q.w[w] = (uint32_t)w < Wq ? qkey[(uint64_t)w * nq + qi] : 0ull;

    // lo = bisect_left(S, q)
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cmp_q(S, mid, q) < 0) lo = mid + 1; else hi = mid;
    }
    int32_t f = -1;
    uint32_t a = lo;
    if (lo < n && eq_q(S, lo, q)) {
        f = (int32_t)lo;
    } else if (adl) {
        if (lo > 0 && q_starts(S, lo - 1, q)) {          // the prefix branch: f the last duplicate, a the first
            f = (int32_t)(lo - 1);
            a = run_first(S, lo - 1);
        }
        // "more than one tag starts with q" looks at S[a + 1] only, and only when S[a] != S[a + 1]
        if (a < n && starts_q(S, a, q) &&
            !(a + 1 < n && !set_eq(S, a, a + 1) && starts_q(S, a + 1, q)))
            f = (int32_t)a;
    }
    if (f < 0) {
        out[qi] = make_int4(-1, -1, -1, -1);
        return;
    }
    // forward: duplicates of S[a], then (allowDiffLengths) the block of strings that start with q
    uint32_t b;
    if (!adl) {
        uint32_t l2 = a, h2 = n;                          // first index past the run of q
        while (l2 < h2) {
            const uint32_t mid = l2 + (h2 - l2) / 2;
            if (eq_q(S, mid, q)) l2 = mid + 1; else h2 = mid;
        }
        b = l2 - 1;
    } else if (lo < n && starts_q(S, lo, q)) {
        uint32_t l2 = lo, h2 = n;                         // first index past the block that starts with q
        while (l2 < h2) {
            const uint32_t mid = l2 + (h2 - l2) / 2;
            if (starts_q(S, mid, q)) l2 = mid + 1; else h2 = mid;
        }
        b = l2 - 1;
    } else {
        b = lo - 1;                                       // the prefix branch's run ends right before lo
    }
    // backward from b (allowDiffLengths): each run of prefixes of q, one binary search per run
    uint32_t c = b;
    if (adl) {
        for (uint32_t guard = 0; c > 0 && guard <= q.L + 1; ++guard) {
            if (!q_starts(S, c - 1, q)) break;
            c = run_first(S, c - 1);
        }
    }
    out[qi] = make_int4(f, (int32_t)a, (int32_t)b, (int32_t)c);
}

// ------------------------------------------------------------------ K4
__global__ __launch_bounds__(256) void k_tag_varsites(const uint8_t *seqs, const uint64_t *offs, const uint32_t *idx,
                                                      const uint64_t *goff, uint32_t ngroups, uint32_t ntags, int trim,
                                                      uint64_t *mask, uint8_t *nonacgt) {
    const uint32_t g = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= ngroups) return;                            // wave-uniform
    const uint64_t t0 = goff[g], t1 = goff[g + 1];
    uint32_t minlen = 0xffffffffu;
    for (uint64_t t = t0; t < t1; ++t) {
        const uint32_t k = idx[t];
        const uint32_t L = k < ntags ? (uint32_t)(offs[k + 1] - offs[k]) : 0u;
        minlen = L < minlen ? L : minlen;
    }
    uint32_t seen[4] = {0, 0, 0, 0};                       // one-hot of A C G T per owned column
    bool bad = false;
    for (uint64_t t = t0; t < t1; ++t) {
        const uint32_t k = idx[t];
        if (k >= ntags) { bad = true; continue; }
        const uint64_t s = offs[k];
        const uint32_t L = (uint32_t)(offs[k + 1] - s);
        const uint32_t lim = trim ? minlen : L;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t col = lane + 64 * r;
            if (col < L) {
                const uint32_t ch = seqs[s + col];
                const uint32_t v = ch == 'A' ? 1u : ch == 'C' ? 2u : ch == 'G' ? 4u : ch == 'T' ? 8u : 0u;
                if (!v) bad = true;
                if (col < lim) seen[r] |= v;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t m = __ballot(__popc(seen[r]) > 1);
        if (lane == 0) mask[4ull * g + r] = m;
    }
    const uint64_t anybad = __ballot(bad);
    if (lane == 0) nonacgt[g] = anybad ? 1 : 0;
}

int ts_check_tags(const uint64_t *offs, uint32_t n, uint32_t *maxlen) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (offs[i + 1] < offs[i]) return td_fail_internal(TD_E_ARG, "offsets must not decrease");
        const uint64_t L = offs[i + 1] - offs[i];
        if (L > TD_TAGSET_MAX_LEN)
            return td_fail_internal(TD_E_LIMIT, ("tag " + std::to_string(i) + " is longer than 256 bases").c_str());
        m = std::max<uint32_t>(m, (uint32_t)L);
    }
    *maxlen = m;
    return TD_OK;
}

// upload n tags and pack them (K1); W words per key
int ts_pack(const char *seqs, const uint64_t *offs, uint32_t n, uint32_t W, tdi::DevBuf<uint8_t> &dseq, tdi::DevBuf<uint64_t> &doff,
            tdi::DevBuf<uint64_t> &key, tdi::DevBuf<uint16_t> &len, tdi::DevBuf<uint32_t> &bad) {
    const uint64_t nbytes = offs[n] - offs[0];
    TD_HIPCHK(dseq.alloc(nbytes));
    TD_HIPCHK(doff.alloc(n + 1ull));
    TD_HIPCHK(key.alloc((uint64_t)W * n));
    TD_HIPCHK(len.alloc(n));
    TD_HIPCHK(bad.alloc(1));
    if (nbytes) TD_HIPCHK(hipMemcpy(dseq.p, seqs + offs[0], nbytes, hipMemcpyHostToDevice));
    std::vector<uint64_t> rel(n + 1ull);
    for (uint64_t i = 0; i <= n; ++i) rel[i] = offs[i] - offs[0];
    TD_HIPCHK(hipMemcpy(doff.p, rel.data(), (n + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemset(bad.p, 0xff, sizeof(uint32_t)));
    if (n) hipLaunchKernelGGL(k_tag_pack, dim3((n + 255) / 256), dim3(256), 0, 0, dseq.p, doff.p, n, W, key.p, len.p, bad.p);
    TD_HIPCHK(hipGetLastError());
    return TD_OK;
}

int ts_bad(const tdi::DevBuf<uint32_t> &bad) {
    uint32_t b = 0;
    TD_HIPCHK(hipMemcpy(&b, bad.p, sizeof b, hipMemcpyDeviceToHost));
    if (b != 0xffffffffu)
        return td_fail_internal(TD_E_ALPHABET, ("tag " + std::to_string(b) + " holds a byte outside ACGT").c_str());
    return TD_OK;
}

}  // namespace

extern "C" int td_tagset_load(td_handle *h, const char *seqs, const uint64_t *offs, uint32_t n, const uint32_t *order,
                              td_tagset **out, uint32_t *perm_out, uint32_t *passes, double *ms) {
    if (!h || !offs || !out || (n && (!seqs || !perm_out))) return td_fail_internal(TD_E_ARG, "NULL argument");
    *out = nullptr;
    if (passes) *passes = 0;
    if (ms) ms[0] = ms[1] = 0;
    if (n > TD_TAGSET_MAX_TAGS) return td_fail_internal(TD_E_LIMIT, "more than 2^30 tags");
    uint32_t maxlen = 0;
    int rc = ts_check_tags(offs, n, &maxlen);
    if (rc) return rc;
    if (order) {
        std::vector<uint8_t> seen(n, 0);
        for (uint32_t i = 0; i < n; ++i) {
            if (order[i] >= n || seen[order[i]]) return td_fail_internal(TD_E_ARG, "order is not a permutation");
            seen[order[i]] = 1;
        }
    }
    const uint32_t W = std::max<uint32_t>(1, (maxlen + 31) / 32);
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    tdi::Events<4> ev;
    TD_HIPCHK(ev.create());
    tdi::DevBuf<uint8_t> dseq;
    tdi::DevBuf<uint64_t> doff, key;
    tdi::DevBuf<uint16_t> len;
    tdi::DevBuf<uint32_t> bad, perm0, perm1, differ, hist;
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    if ((rc = ts_pack(seqs, offs, n, W, dseq, doff, key, len, bad))) return rc;
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    if ((rc = ts_bad(bad))) return rc;

    TD_HIPCHK(perm0.alloc(n));
    TD_HIPCHK(perm1.alloc(n));
    TD_HIPCHK(differ.alloc(3));
    std::vector<uint32_t> init(n);
    for (uint32_t i = 0; i < n; ++i) init[i] = order ? order[i] : i;
    if (n) TD_HIPCHK(hipMemcpy(perm0.p, init.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemset(differ.p, 0, 3 * sizeof(uint32_t)));
    TD_HIPCHK(hipEventRecord(ev.e[2], 0));
    uint32_t npass = 0;
    if (n > 1) {
        TD_HIPCHK(hist.alloc(256ull * tdrs::rs_blocks(n)));
        TD_HIPCHK(tdrs::rs_sort(key.p, len.p, n, W, &perm0.p, &perm1.p, differ.p, hist.p, &npass));
    }
    std::unique_ptr<td_tagset> set(new td_tagset{td_handle_device(h), n, W, {}, {}});      // the sorted set: the caller's once everything has succeeded
    tdi::DevBuf<uint64_t> &skey = set->key;
    tdi::DevBuf<uint16_t> &slen = set->len;
    const hipError_t e1 = skey.alloc((size_t)W * n), e2 = slen.alloc(n);
    if (e1 != hipSuccess || e2 != hipSuccess) return td_fail_internal(TD_E_HIP, "hipMalloc of the sorted set failed");
    if (n) hipLaunchKernelGGL(k_rs_gather, dim3((n + 255) / 256), dim3(256), 0, 0, key.p, len.p, perm0.p, n, W, skey.p, slen.p);
    hipError_t e3 = hipGetLastError();
    if (e3 == hipSuccess) e3 = hipEventRecord(ev.e[3], 0);
    if (e3 == hipSuccess) e3 = hipEventSynchronize(ev.e[3]);
    if (e3 == hipSuccess && n) e3 = hipMemcpy(perm_out, perm0.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e3 != hipSuccess) return td_fail_internal(TD_E_HIP, (std::string("td_tagset_load: ") + hipGetErrorString(e3)).c_str());
    if (ms) {
        ms[0] = ev.elapsed(0, 1);
        ms[1] = ev.elapsed(2, 3);
    }
    if (passes) *passes = npass;
    *out = set.release();
    return TD_OK;
}

extern "C" int td_tagset_free(td_handle *h, td_tagset *s) {
    (void)h;
    if (!s) return TD_OK;
    (void)hipSetDevice(s->device);
    delete s;
    return TD_OK;
}

extern "C" int td_tagset_lookup(td_handle *h, const td_tagset *s, const char *seqs, const uint64_t *offs, uint32_t nq,
                                int allow_diff_lengths, int32_t *out, double *ms) {
    if (!h || !s || !offs || (nq && (!seqs || !out))) return td_fail_internal(TD_E_ARG, "NULL argument");
    if (ms) *ms = 0;
    if (nq > TD_TAGSET_MAX_TAGS) return td_fail_internal(TD_E_LIMIT, "more than 2^30 queries");
    uint32_t maxlen = 0;
    int rc = ts_check_tags(offs, nq, &maxlen);
    if (rc) return rc;
    if (!nq) return TD_OK;
    const uint32_t Wq = std::max<uint32_t>(1, (maxlen + 31) / 32);
    TD_HIPCHK(hipSetDevice(s->device));
    tdi::Events<4> ev;
    TD_HIPCHK(ev.create());
    tdi::DevBuf<uint8_t> dseq;
    tdi::DevBuf<uint64_t> doff, key;
    tdi::DevBuf<uint16_t> len;
    tdi::DevBuf<uint32_t> bad;
    tdi::DevBuf<int4> dout;
    if ((rc = ts_pack(seqs, offs, nq, Wq, dseq, doff, key, len, bad))) return rc;
    if ((rc = ts_bad(bad))) return rc;
    TD_HIPCHK(dout.alloc(nq));
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    hipLaunchKernelGGL(k_tag_lookup, dim3((nq + 255) / 256), dim3(256), 0, 0, s->key.p, s->len.p, s->n, s->W, key.p, len.p, nq, Wq,
                       allow_diff_lengths ? 1 : 0, dout.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[1]));
    if (ms) *ms = ev.elapsed(0, 1);
    TD_HIPCHK(hipMemcpy(out, dout.p, nq * sizeof(int4), hipMemcpyDeviceToHost));
    return TD_OK;
}

extern "C" int td_tagset_varsites(td_handle *h, const char *seqs, const uint64_t *offs, uint32_t ntags, const uint32_t *idx,
                                  const uint64_t *goff, uint32_t ngroups, int trim, uint64_t *mask_out, uint8_t *nonacgt_out,
                                  double *ms) {
    if (!h || !offs || !goff || (ngroups && (!mask_out || !nonacgt_out)) || (ntags && !seqs))
        return td_fail_internal(TD_E_ARG, "NULL argument");
    if (ms) *ms = 0;
    uint32_t maxlen = 0;
    int rc = ts_check_tags(offs, ntags, &maxlen);
    if (rc) return rc;
    if (!ngroups) return TD_OK;
    if (goff[0] != 0) return td_fail_internal(TD_E_ARG, "group offsets must start at 0");
    for (uint32_t g = 0; g < ngroups; ++g)
        if (goff[g + 1] <= goff[g]) return td_fail_internal(TD_E_ARG, "every group needs a tag");
    const uint64_t nidx = goff[ngroups];
    if (!idx) return td_fail_internal(TD_E_ARG, "NULL argument");
    for (uint64_t t = 0; t < nidx; ++t)
        if (idx[t] >= ntags) return td_fail_internal(TD_E_ARG, "tag index out of range");
    TD_HIPCHK(hipSetDevice(td_handle_device(h)));
    tdi::Events<2> ev;
    TD_HIPCHK(ev.create());
    const uint64_t nbytes = offs[ntags] - offs[0];
    tdi::DevBuf<uint8_t> dseq, dbad;
    tdi::DevBuf<uint64_t> doff, dgoff, dmask;
    tdi::DevBuf<uint32_t> didx;
    TD_HIPCHK(dseq.alloc(nbytes));
    TD_HIPCHK(doff.alloc(ntags + 1ull));
    TD_HIPCHK(didx.alloc(nidx));
    TD_HIPCHK(dgoff.alloc(ngroups + 1ull));
    TD_HIPCHK(dmask.alloc(4ull * ngroups));
    TD_HIPCHK(dbad.alloc(ngroups));
    if (nbytes) TD_HIPCHK(hipMemcpy(dseq.p, seqs + offs[0], nbytes, hipMemcpyHostToDevice));
    std::vector<uint64_t> rel(ntags + 1ull);
    for (uint64_t i = 0; i <= ntags; ++i) rel[i] = offs[i] - offs[0];
    TD_HIPCHK(hipMemcpy(doff.p, rel.data(), (ntags + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(didx.p, idx, nidx * sizeof(uint32_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipMemcpy(dgoff.p, goff, (ngroups + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice));
    TD_HIPCHK(hipEventRecord(ev.e[0], 0));
    const uint32_t grid = (ngroups + 3) / 4;
    hipLaunchKernelGGL(k_tag_varsites, dim3(grid), dim3(256), 0, 0, dseq.p, doff.p, didx.p, dgoff.p, ngroups, ntags, trim ? 1 : 0,
                       dmask.p, dbad.p);
    TD_HIPCHK(hipGetLastError());
    TD_HIPCHK(hipEventRecord(ev.e[1], 0));
    TD_HIPCHK(hipEventSynchronize(ev.e[1]));
    if (ms) *ms = ev.elapsed(0, 1);
    TD_HIPCHK(hipMemcpy(mask_out, dmask.p, 4ull * ngroups * sizeof(uint64_t), hipMemcpyDeviceToHost));
    TD_HIPCHK(hipMemcpy(nonacgt_out, dbad.p, ngroups, hipMemcpyDeviceToHost));
    return TD_OK;
}
