// Text of one CSV cell as pandas' DataFrame.to_csv writes it with default arguments, shared by the device kernels
// (csvtext.hip) and the host check program (tools/csvtext_hostcheck.cpp); include/sequoia_hip.h ("CSV text") is the contract.
//   int64      plain decimal, '-' for negatives (at most 20 bytes).
//   float32    numpy.ndarray.astype(str) of the value (at most 19 bytes), NaN the empty cell:
//              digits    the shortest decimal inside the rounding interval of the float32 (half an ulp to either side; below
//                        an exact power of two a quarter of the upper ulp), the closest such decimal when there are several,
//                        a tie to the even digit.  The interval's bounds count as inside exactly when the mantissa is even
//                        (a decimal on the bound then reads back as this float32 under round-to-nearest-even): 38973928.0f,
//                        whose upper bound is 38973930, prints as "38973930.0", its odd neighbour 38973932.0f in full.  That is
//                        the choice of numpy's Dragon4 in unique mode, and 4304 of the 2 050 932 values of the host check
//                        print differently when the bounds are always excluded.  The digits come from Ryu's float32
//                        arithmetic (Adams 2018: one 32 x 64-bit product per bound against a table of powers of five).
//              layout    1e-4 <= |x| < 1e16: positional, integers with a trailing ".0", zero padded ("3333333500000000.0",
//                        "0.00012"); otherwise scientific, d[.ddd]e+XX with at least two exponent digits ("1e-05", "3e+16").
//                        -0.0 keeps its sign; "inf", "-inf".
// A cell is followed by ',' or, in the last column, by '\n': sqf_cell gives the length with that byte and, when it is handed
// a destination, writes exactly those bytes.  Nothing here reads or writes outside what it is handed, every loop has a
// constant bound (13 divisions by five, 10 removed digits, 20 digits written), and nothing is floating-point arithmetic
// except two comparisons.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define SQF_HD __host__ __device__ static __forceinline__
#else
#define SQF_HD static inline
#endif

#define SQF_MAX_I64 20                   // "-9223372036854775808"
#define SQF_MAX_F32 19                   // "-1000000000000000.0"
#define SQF_MAX_CELL 21                  // the longest cell with its ',' or '\n'

// one table of a call: row r holds index[r], ints[r * n_int + 0..n_int), f32[r * ld_f32 + 0..n_f32)
struct SqfTable {
    const int64_t* index;
    const int64_t* ints;
    const float* f32;
    int n_int, n_f32;
    long long ld_f32;
};

SQF_HD uint32_t sqf_pow5bits(uint32_t e) { return ((e * 1217359u) >> 19) + 1u; }       // ceil(log2(5^e)), e <= 3528
SQF_HD uint32_t sqf_log10pow2(uint32_t e) { return (e * 78913u) >> 18; }               // floor(log10(2^e)), e <= 1650
SQF_HD uint32_t sqf_log10pow5(uint32_t e) { return (e * 732923u) >> 20; }              // floor(log10(5^e)), e <= 2620

SQF_HD bool sqf_multiple_of_pow5(uint32_t v, uint32_t p) {      // v > 0
    uint32_t n = 0;
    for (int k = 0; k < 14 && v % 5u == 0; ++k) {
        v /= 5u;
        ++n;
    }
    return n >= p;
}

// (m * factor) >> shift, 32 < shift < 96, the result below 2^32
SQF_HD uint32_t sqf_mul_shift(uint32_t m, uint64_t factor, int shift) {
    const uint64_t lo = (uint64_t)m * (uint32_t)factor;
    const uint64_t hi = (uint64_t)m * (uint32_t)(factor >> 32);
    return (uint32_t)(((lo >> 32) + hi) >> (shift - 32));
}

#define SQF_POW5_INV_BITS 59
#define SQF_POW5_BITS 61
// floor(2^(pow5bits(i) - 1 + 59) / 5^i) + 1
SQF_HD uint64_t sqf_pow5_inv(uint32_t i) {
    const uint64_t t[31] = {
        0x0800000000000001ull, 0x0666666666666667ull, 0x051eb851eb851eb9ull, 0x04189374bc6a7efaull,
        0x068db8bac710cb2aull, 0x053e2d6238da3c22ull, 0x0431bde82d7b634eull, 0x06b5fca6af2bd216ull,
        0x055e63b88c230e78ull, 0x044b82fa09b5a52dull, 0x06df37f675ef6eaeull, 0x057f5ff85e592558ull,
        0x0465e6604b7a8447ull, 0x0709709a125da071ull, 0x05a126e1a84ae6c1ull, 0x0480ebe7b9d58567ull,
        0x0734aca5f6226f0bull, 0x05c3bd5191b525a3ull, 0x049c97747490eae9ull, 0x0760f253edb4ab0eull,
        0x05e72843249088d8ull, 0x04b8ed0283a6d3e0ull, 0x078e480405d7b966ull, 0x060b6cd004ac9452ull,
        0x04d5f0a66a23a9dbull, 0x07bcb43d769f762bull, 0x063090312bb2c4efull, 0x04f3a68dbc8f03f3ull,
        0x07ec3daf94180651ull, 0x065697bfa9acd1daull, 0x051212ffbaf0a7e2ull};
    return t[i < 31 ? i : 30];
}
// the leading 61 bits of 5^i
SQF_HD uint64_t sqf_pow5(uint32_t i) {
    const uint64_t t[48] = {
        0x1000000000000000ull, 0x1400000000000000ull, 0x1900000000000000ull, 0x1f40000000000000ull,
        0x1388000000000000ull, 0x186a000000000000ull, 0x1e84800000000000ull, 0x1312d00000000000ull,
        0x17d7840000000000ull, 0x1dcd650000000000ull, 0x12a05f2000000000ull, 0x174876e800000000ull,
        0x1d1a94a200000000ull, 0x12309ce540000000ull, 0x16bcc41e90000000ull, 0x1c6bf52634000000ull,
        0x11c37937e0800000ull, 0x16345785d8a00000ull, 0x1bc16d674ec80000ull, 0x1158e460913d0000ull,
        0x15af1d78b58c4000ull, 0x1b1ae4d6e2ef5000ull, 0x10f0cf064dd59200ull, 0x152d02c7e14af680ull,
        0x1a784379d99db420ull, 0x108b2a2c28029094ull, 0x14adf4b7320334b9ull, 0x19d971e4fe8401e7ull,
        0x1027e72f1f128130ull, 0x1431e0fae6d7217cull, 0x193e5939a08ce9dbull, 0x1f8def8808b02452ull,
        0x13b8b5b5056e16b3ull, 0x18a6e32246c99c60ull, 0x1ed09bead87c0378ull, 0x13426172c74d822bull,
        0x1812f9cf7920e2b6ull, 0x1e17b84357691b64ull, 0x12ced32a16a1b11eull, 0x178287f49c4a1d66ull,
        0x1d6329f1c35ca4bfull, 0x125dfa371a19e6f7ull, 0x16f578c4e0a060b5ull, 0x1cb2d6f618c878e3ull,
        0x11efc659cf7d4b8dull, 0x166bb7f0435c9e71ull, 0x1c06a5ec5433c60dull, 0x118427b3b4a05bc8ull};
    return t[i < 48 ? i : 47];
}

SQF_HD int sqf_digits_u32(uint32_t v) {      // v < 10^9
    return v >= 100000000u ? 9 : v >= 10000000u ? 8 : v >= 1000000u ? 7 : v >= 100000u ? 6 : v >= 10000u ? 5 : v >= 1000u ? 4
         : v >= 100u ? 3 : v >= 10u ? 2 : 1;
}

// The digits of a finite non-zero float32 (sign bit ignored): *digits (1 to 9 decimal digits, no trailing zero unless the
// interval forces one) and the power of ten of its last digit, value ~ *digits * 10^*exp10.
SQF_HD void sqf_shortest_f32(uint32_t bits, uint32_t* digits, int* exp10) {
    const uint32_t mant = bits & 0x7FFFFFu, expo = (bits >> 23) & 0xFFu;
    const int e2 = (expo ? (int)expo : 1) - 127 - 23 - 2;
    const uint32_t m2 = expo ? (mant | 0x800000u) : mant;
    const uint32_t shift_mm = (mant != 0 || expo <= 1) ? 1u : 0u;            // 0: an exact power of two, the lower half-gap is half as wide
    const uint32_t mv = 4u * m2, mp = 4u * m2 + 2u, mm = 4u * m2 - 1u - shift_mm;
    uint32_t vr, vp, vm, last = 0;
    int e10;
    const bool even = (m2 & 1u) == 0;                                        // an even mantissa: a tie rounds to it, the bounds are inside
    bool vr_zeros = false;                                                   // every digit removed from vr so far is 0
    bool vm_zeros = false;                                                   // ... from vm: the lower bound is exact so far
    if (e2 >= 0) {
        const uint32_t q = sqf_log10pow2((uint32_t)e2);
        e10 = (int)q;
        const int k = SQF_POW5_INV_BITS + (int)sqf_pow5bits(q) - 1;
        const int i = -e2 + (int)q + k;
        vr = sqf_mul_shift(mv, sqf_pow5_inv(q), i);
        vp = sqf_mul_shift(mp, sqf_pow5_inv(q), i);
        vm = sqf_mul_shift(mm, sqf_pow5_inv(q), i);
        if (q != 0 && (vp - 1u) / 10u <= vm / 10u) {                         // the loop below removes nothing: the digit behind vr
            const int l = SQF_POW5_INV_BITS + (int)sqf_pow5bits(q - 1u) - 1;
            last = sqf_mul_shift(mv, sqf_pow5_inv(q - 1u), -e2 + (int)q - 1 + l) % 10u;
        }
        if (q <= 9) {
            if (mv % 5u == 0) vr_zeros = sqf_multiple_of_pow5(mv, q);
            else if (even) vm_zeros = sqf_multiple_of_pow5(mm, q);
            else vp -= sqf_multiple_of_pow5(mp, q) ? 1u : 0u;                 // the upper bound itself is outside
        }
    } else {
        const uint32_t q = sqf_log10pow5((uint32_t)(-e2));
        e10 = (int)q + e2;
        const int i = -e2 - (int)q;
        const int k = (int)sqf_pow5bits((uint32_t)i) - SQF_POW5_BITS;
        int j = (int)q - k;
        vr = sqf_mul_shift(mv, sqf_pow5((uint32_t)i), j);
        vp = sqf_mul_shift(mp, sqf_pow5((uint32_t)i), j);
        vm = sqf_mul_shift(mm, sqf_pow5((uint32_t)i), j);
        if (q != 0 && (vp - 1u) / 10u <= vm / 10u) {
            j = (int)q - 1 - ((int)sqf_pow5bits((uint32_t)(i + 1)) - SQF_POW5_BITS);
            last = sqf_mul_shift(mv, sqf_pow5((uint32_t)(i + 1)), j) % 10u;
        }
        if (q <= 1) {
            vr_zeros = true;                                                 // mv = 4 m2 has at least two factors of two
            if (even) vm_zeros = shift_mm == 1u;                             // mm = mv - 2 has one factor of two
            else --vp;                                                       // mp = mv + 2 has one: vp is exact, and outside
        } else if (q < 31) {
            vr_zeros = (mv & ((1u << (q - 1u)) - 1u)) == 0;
        }
    }
    int removed = 0;
    for (int n = 0; n < 10 && vp / 10u > vm / 10u; ++n) {
        vm_zeros = vm_zeros && vm % 10u == 0;
        vr_zeros = vr_zeros && last == 0;
        last = vr % 10u;
        vr /= 10u;
        vp /= 10u;
        vm /= 10u;
        ++removed;
    }
    for (int n = 0; n < 10 && vm_zeros && vm % 10u == 0; ++n) {              // the exact lower bound is inside and shorter
        vr_zeros = vr_zeros && last == 0;
        last = vr % 10u;
        vr /= 10u;
        vp /= 10u;
        vm /= 10u;
        ++removed;
    }
    if (vr_zeros && last == 5 && vr % 2u == 0) last = 4;                     // exactly half: to the even digit
    *digits = vr + (((vr == vm && !(even && vm_zeros)) || last >= 5) ? 1u : 0u);      // vr == vm: rounding down would leave the interval
    *exp10 = e10 + removed;
}

// Text of an int64: the length; with WRITE, the bytes at out[0 .. length).
template <bool WRITE>
SQF_HD int sqf_i64(int64_t v, char* out) {
    const bool neg = v < 0;
    uint64_t u = neg ? 0ull - (uint64_t)v : (uint64_t)v;
    int nd = 1;
    for (uint64_t t = u; nd < 20 && t >= 10ull; ++nd) t /= 10ull;
    const int len = nd + (neg ? 1 : 0);
    if (WRITE) {
        if (neg) out[0] = '-';
        for (int p = len - 1, k = 0; k < nd; ++k, --p) {
            out[p] = (char)('0' + (int)(u % 10ull));
            u /= 10ull;
        }
    }
    return len;
}

// out[pos + 0 .. nd): the nd decimal digits of v
SQF_HD void sqf_put_digits(char* out, int pos, uint32_t v, int nd) {
    for (int k = nd - 1; k >= 0; --k) {
        out[pos + k] = (char)('0' + (int)(v % 10u));
        v /= 10u;
    }
}

// Text of a float32 given as its bits: the length (0 for NaN); with WRITE, the bytes at out[0 .. length).
template <bool WRITE>
SQF_HD int sqf_f32(uint32_t bits, char* out) {
    const uint32_t a = bits & 0x7FFFFFFFu;
    const int neg = (int)(bits >> 31);
    if (a > 0x7F800000u) return 0;                                           // NaN: the empty cell
    if (WRITE && neg) out[0] = '-';
    if (a == 0x7F800000u) {
        if (WRITE) { out[neg] = 'i'; out[neg + 1] = 'n'; out[neg + 2] = 'f'; }
        return neg + 3;
    }
    if (a == 0) {
        if (WRITE) { out[neg] = '0'; out[neg + 1] = '.'; out[neg + 2] = '0'; }
        return neg + 3;
    }
    uint32_t d;
    int e;
    sqf_shortest_f32(a, &d, &e);
    const int nd = sqf_digits_u32(d);
    const int sci = e + nd - 1;                                              // power of ten of the first digit
    float av;
    __builtin_memcpy(&av, &a, 4);
    if ((double)av >= 1e-4 && (double)av < 1e16) {
        if (sci < 0) {                                                       // 0.000ddd
            const int zeros = -sci - 1;
            if (WRITE) {
                out[neg] = '0';
                out[neg + 1] = '.';
                for (int k = 0; k < zeros; ++k) out[neg + 2 + k] = '0';
                sqf_put_digits(out, neg + 2 + zeros, d, nd);
            }
            return neg + 2 + zeros + nd;
        }
        const int whole = sci + 1;                                           // digits in front of the point
        if (nd <= whole) {                                                   // ddd000.0
            if (WRITE) {
                sqf_put_digits(out, neg, d, nd);
                for (int k = nd; k < whole; ++k) out[neg + k] = '0';
                out[neg + whole] = '.';
                out[neg + whole + 1] = '0';
            }
            return neg + whole + 2;
        }
        if (WRITE) {                                                         // dd.ddd
            uint32_t frac_unit = 1;
            for (int k = 0; k < nd - whole; ++k) frac_unit *= 10u;
            sqf_put_digits(out, neg, d / frac_unit, whole);
            out[neg + whole] = '.';
            sqf_put_digits(out, neg + whole + 1, d % frac_unit, nd - whole);
        }
        return neg + nd + 1;
    }
    const int body = nd + (nd > 1 ? 1 : 0);                                  // d or d.ddd
    if (WRITE) {
        uint32_t unit = 1;
        for (int k = 0; k < nd - 1; ++k) unit *= 10u;
        out[neg] = (char)('0' + (int)(d / unit));
        if (nd > 1) {
            out[neg + 1] = '.';
            sqf_put_digits(out, neg + 2, d % unit, nd - 1);
        }
        const int s = sci < 0 ? -sci : sci;                                  // at most 45: two digits
        out[neg + body] = 'e';
        out[neg + body + 1] = sci < 0 ? '-' : '+';
        out[neg + body + 2] = (char)('0' + s / 10);
        out[neg + body + 3] = (char)('0' + s % 10);
    }
    return neg + body + 4;
}

// Cell j of row r (0: the index, then the int columns, then the float columns) with the ',' or '\n' behind it: the
// length, 1 .. SQF_MAX_CELL; with WRITE, the bytes at out[0 .. length).
template <bool WRITE>
SQF_HD int sqf_cell(const SqfTable& t, long long r, int j, char* out) {
    int len;
    if (j == 0) {
        len = sqf_i64<WRITE>(t.index[r], out);
    } else if (j <= t.n_int) {
        len = sqf_i64<WRITE>(t.ints[r * (long long)t.n_int + (j - 1)], out);
    } else {
        uint32_t bits;
        __builtin_memcpy(&bits, t.f32 + r * t.ld_f32 + (j - 1 - t.n_int), 4);
        len = sqf_f32<WRITE>(bits, out);
    }
    if (WRITE) out[len] = j == t.n_int + t.n_f32 ? '\n' : ',';
    return len + 1;
}
