// The cell of a VCF body line (vcf.hip): its fields, its length and its bytes, in integers only.  Plain C++
// that the kernels of vcf.hip compile for the device and san/vcf_san.cpp compiles for the host, where the sanitizers and
// snprintf can check it.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define VCF_HD __device__ __forceinline__
#else
#define VCF_HD inline
#endif

struct VcfTab {                                    // by value in the kernel arguments
    uint32_t ca[3], cb[3];
};

struct VcfCell {
    uint32_t a, b, code, gq;
    uint64_t n;
    uint32_t pl[3];
};

VCF_HD uint32_t dec_len32(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}
VCF_HD uint32_t dec_len64(uint64_t v) {       // v <= 2^33 - 2 < 10^10
    return v >= 1000000000ull ? 10u : dec_len32((uint32_t)v);
}

// GQ and PL of a called diploid cell (code <= 2)
VCF_HD void vcf_likelihoods(VcfCell &c, const VcfTab &tab) {
    uint32_t x = c.a, y = c.b;
    if (c.n > 127u) {
        x = (uint32_t)(127ull * c.a / c.n);
        y = (uint32_t)(127ull * c.b / c.n);
    }
    uint32_t cost[3], cmin = ~0u;                  // x + y <= 127, entries <= 2^23: below 2^30
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        cost[g] = y * tab.ca[g] + x * tab.cb[g];
        cmin = cost[g] < cmin ? cost[g] : cmin;
    }
    uint32_t gq = 99u;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const uint64_t q = ((uint64_t)(cost[g] - cmin) * 30103ull + 327680000ull) / 655360000ull;     // below 2^45
        c.pl[g] = q < 255u ? (uint32_t)q : 255u;
        if ((uint32_t)g != c.code && c.pl[g] < gq) gq = c.pl[g];
    }
    c.gq = gq;
}

template <bool LIK> VCF_HD VcfCell vcf_cell(uint32_t a, uint32_t b, uint32_t code, const VcfTab &tab) {
    VcfCell c;
    c.a = a;
    c.b = b;
    c.code = code;
    c.n = (uint64_t)a + b;
    c.gq = 0;
    c.pl[0] = c.pl[1] = c.pl[2] = 0;
    if (LIK && code <= 2u) vcf_likelihoods(c, tab);
    return c;
}

// the bytes of a cell with its tab
template <bool LIK> VCF_HD uint32_t vcf_cell_len(const VcfCell &c, uint32_t P) {
    uint32_t len = 1u + (2u * P - 1u) + 1u + dec_len32(c.a) + 1u + dec_len32(c.b) + 1u + dec_len64(c.n);
    if (LIK) len += c.code > 2u ? 4u : 1u + dec_len32(c.gq) + 1u + dec_len32(c.pl[0]) + 1u + dec_len32(c.pl[1]) + 1u + dec_len32(c.pl[2]);
    return len;
}

// `len` decimal digits of v, leading zeros where v has fewer; digits by division by a constant
VCF_HD uint8_t *put_dec32(uint8_t *p, uint32_t v, uint32_t len) {
    for (uint32_t i = len; i-- > 0;) {
        const uint32_t q = v / 10u;
        p[i] = (uint8_t)('0' + (v - q * 10u));
        v = q;
    }
    return p + len;
}
VCF_HD uint8_t *put_dec(uint8_t *p, uint32_t v) { return put_dec32(p, v, dec_len32(v)); }

// the cell into LDS at p: exactly vcf_cell_len bytes
template <bool LIK> VCF_HD void vcf_put_cell(uint8_t *p, const VcfCell &c, uint32_t P) {
    *p++ = '\t';
    for (uint32_t j = 0; j < P; ++j) {
        if (j) *p++ = '/';
        *p++ = c.code > P ? '.' : j < P - c.code ? '0' : '1';
    }
    *p++ = ':';
    p = put_dec(p, c.a);
    *p++ = ',';
    p = put_dec(p, c.b);
    *p++ = ':';
    if (c.n >= 1000000000ull) {
        const uint32_t hi = (uint32_t)(c.n / 1000000000ull);       // 1 .. 8
        *p++ = (uint8_t)('0' + hi);
        p = put_dec32(p, (uint32_t)(c.n - (uint64_t)hi * 1000000000ull), 9);
    } else {
        p = put_dec(p, (uint32_t)c.n);
    }
    if (LIK) {
        *p++ = ':';
        if (c.code > 2u) {
            *p++ = '.';
            *p++ = ':';
            *p++ = '.';
        } else {
            p = put_dec(p, c.gq);
            *p++ = ':';
            p = put_dec(p, c.pl[0]);
            *p++ = ',';
            p = put_dec(p, c.pl[1]);
            *p++ = ',';
            p = put_dec(p, c.pl[2]);
        }
    }
}
