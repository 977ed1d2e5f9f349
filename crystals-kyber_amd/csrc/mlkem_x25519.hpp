// mlkem_x25519.hpp — batched X25519 (RFC 7748 section 5): the curve leg of the hybrid KEMs (mlkem_xwing.hpp).
//
// One item per SIMD lane.  A field element mod p = 2^255 - 19 is ten unsigned limbs of 26, 25, 26, 25, ... bits (radix 2^25.5) in
// ten VGPRs; a product accumulates in ten 64-bit sums of 32 x 32 -> 64-bit multiply-adds (v_mad_u64_u32), the factors 2 (both limbs
// odd) and 19 (wrap past limb 9) folded into one 32-bit operand beforehand.  Why this representation: LABNOTES "X25519".
// Bounds.  fe_mul / fe_sq / fe_mul_small leave limbs <= 2^26 + 2^18 (even index) and 2^25 + 2^18 (odd); they take operands with
// limbs up to 3 * 2^26 (even) / 3 * 2^25 + 2^18 (odd), which is what one fe_add or fe_sub of two such results gives:
//   19 * 3 * 2^26 < 2^32 (the folded operand fits 32 bits); one term <= 3 * 2^26 * 57 * 2^26 < 2^59.5; ten terms < 2^62.9 < 2^64.
// Constant time: the scalar and every field value live in registers only (no LDS, no scratch); the ladder's conditional swap is a
// mask; the inversion is a fixed addition chain; the final reduction selects with a carry, not a branch.  The only data-dependent
// control flow is the item bound `item < n` around loads and stores; loop bounds and addresses depend on n and the lane alone.
#pragma once
#include "mlkem_kernels.hpp"

namespace mlkem {

struct Fe { uint32_t v[10]; };

constexpr uint32_t FE_M26 = 0x3FFFFFFu, FE_M25 = 0x1FFFFFFu;
constexpr int fe_bits(int i) { return (i & 1) ? 25 : 26; }
constexpr uint32_t fe_mask(int i) { return (i & 1) ? FE_M25 : FE_M26; }

__device__ __forceinline__ void fe_set(Fe& h, uint32_t c) {
    h.v[0] = c;
#pragma unroll
    for (int i = 1; i < 10; i++) h.v[i] = 0;
}
__device__ __forceinline__ void fe_add(Fe& h, const Fe& f, const Fe& g) {
#pragma unroll
    for (int i = 0; i < 10; i++) h.v[i] = f.v[i] + g.v[i];
}
// f - g + 2p, limb by limb.  2p = (2^27 - 38, 2^26 - 2, 2^27 - 2, 2^26 - 2, ...) is above every limb of a carried product (g is
// always one here), so no limb goes negative, and f + 2p - g <= 2^26 + 2^18 + 2^27: within what a product takes.
__device__ __forceinline__ void fe_sub(Fe& h, const Fe& f, const Fe& g) {
    h.v[0] = f.v[0] + 0x7FFFFDAu - g.v[0];
#pragma unroll
    for (int i = 1; i < 10; i++) h.v[i] = f.v[i] + ((i & 1) ? 0x3FFFFFEu : 0x7FFFFFEu) - g.v[i];
}
// 32-bit carry pass: limbs below 2^31 in; limbs 1..9 tight and limb 0 < 2^26 + 19 * 64 out
__device__ __forceinline__ void fe_carry32(Fe& h) {
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const uint32_t t = h.v[i] + c;
        c = t >> fe_bits(i);
        h.v[i] = t & fe_mask(i);
    }
    h.v[0] += 19u * c;
}

// carry the ten 64-bit sums of a product into limbs: 0 -> 1 -> ... -> 9 -> (x 19) 0 -> 1
__device__ __forceinline__ void fe_carry64(Fe& h, uint64_t (&s)[10]) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const uint64_t t = s[i] + c;
        c = t >> fe_bits(i);
        h.v[i] = (uint32_t)t & fe_mask(i);
    }
    // c < 2^39: 19 c + limb 0 < 2^44
    const uint64_t t0 = (uint64_t)h.v[0] + 19u * c;
    h.v[0] = (uint32_t)t0 & FE_M26;
    h.v[1] += (uint32_t)(t0 >> 26);   // < 2^18
}

__device__ __forceinline__ void fe_mul(Fe& h, const Fe& f, const Fe& g) {
    uint32_t g19[10], f2[10];
#pragma unroll
    for (int i = 0; i < 10; i++) {
        g19[i] = 19u * g.v[i];
        f2[i] = (i & 1) ? 2u * f.v[i] : f.v[i];
    }
    uint64_t s[10];
#pragma unroll
    for (int k = 0; k < 10; k++) s[k] = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
#pragma unroll
        for (int j = 0; j < 10; j++) {
            const int k = i + j;
            const uint32_t a = ((i & 1) && (j & 1)) ? f2[i] : f.v[i];
            const uint32_t b = k >= 10 ? g19[j] : g.v[j];
            s[k % 10] += (uint64_t)a * b;
        }
    }
    fe_carry64(h, s);
}

__device__ __forceinline__ void fe_sq(Fe& h, const Fe& f) {
    uint32_t f19[10], f2[10], f4[10];
#pragma unroll
    for (int i = 0; i < 10; i++) {
        f19[i] = 19u * f.v[i];
        f2[i] = 2u * f.v[i];
        f4[i] = 4u * f.v[i];
    }
    uint64_t s[10];
#pragma unroll
    for (int k = 0; k < 10; k++) s[k] = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
#pragma unroll
        for (int j = i; j < 10; j++) {
            const int k = i + j;
            const bool odd = (i & 1) && (j & 1), cross = i != j;
            const uint32_t a = odd ? (cross ? f4[i] : f2[i]) : (cross ? f2[i] : f.v[i]);
            const uint32_t b = k >= 10 ? f19[j] : f.v[j];
            s[k % 10] += (uint64_t)a * b;
        }
    }
    fe_carry64(h, s);
}

// h = f * C for a small constant (121665, 9)
template <uint32_t C>
__device__ __forceinline__ void fe_mul_small(Fe& h, const Fe& f) {
    uint64_t s[10];
#pragma unroll
    for (int i = 0; i < 10; i++) s[i] = (uint64_t)f.v[i] * C;
    fe_carry64(h, s);
}

__device__ __forceinline__ void fe_cswap(Fe& a, Fe& b, uint32_t mask) {
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const uint32_t t = (a.v[i] ^ b.v[i]) & mask;
        a.v[i] ^= t;
        b.v[i] ^= t;
    }
}

__device__ __forceinline__ void fe_sq_n(Fe& h, int n) {
#pragma unroll 1
    for (int i = 0; i < n; i++) {
        Fe t;
        fe_sq(t, h);
        h = t;
    }
}

// z^(p - 2) = z^(2^255 - 21): the usual chain of 254 squarings and 11 products
__device__ __forceinline__ void fe_invert(Fe& out, const Fe& z) {
    Fe z2, z9, z11, a, b, c, t;
    fe_sq(z2, z);                       // 2
    t = z2; fe_sq_n(t, 2);              // 8
    fe_mul(z9, t, z);                   // 9
    fe_mul(z11, z9, z2);                // 11
    fe_sq(t, z11);                      // 22
    fe_mul(a, t, z9);                   // 2^5 - 1
    t = a; fe_sq_n(t, 5);
    fe_mul(a, t, a);                    // 2^10 - 1
    t = a; fe_sq_n(t, 10);
    fe_mul(b, t, a);                    // 2^20 - 1
    t = b; fe_sq_n(t, 20);
    fe_mul(t, t, b);                    // 2^40 - 1
    fe_sq_n(t, 10);
    fe_mul(a, t, a);                    // 2^50 - 1
    t = a; fe_sq_n(t, 50);
    fe_mul(b, t, a);                    // 2^100 - 1
    t = b; fe_sq_n(t, 100);
    fe_mul(c, t, b);                    // 2^200 - 1
    fe_sq_n(c, 50);
    fe_mul(t, c, a);                    // 2^250 - 1
    fe_sq_n(t, 5);
    fe_mul(out, t, z11);                // 2^255 - 21
}

// the 255 low bits of a little-endian 32-byte string: any value below 2^255 is accepted (RFC 7748: bit 255 ignored, u taken mod p)
__device__ __forceinline__ void fe_decode(Fe& h, const uint32_t (&w)[8]) {
    h.v[0] = w[0] & FE_M26;
    h.v[1] = ((w[0] >> 26) | (w[1] << 6)) & FE_M25;
    h.v[2] = ((w[1] >> 19) | (w[2] << 13)) & FE_M26;
    h.v[3] = ((w[2] >> 13) | (w[3] << 19)) & FE_M25;
    h.v[4] = (w[3] >> 6) & FE_M26;
    h.v[5] = w[4] & FE_M25;
    h.v[6] = ((w[4] >> 25) | (w[5] << 7)) & FE_M26;
    h.v[7] = ((w[5] >> 19) | (w[6] << 13)) & FE_M25;
    h.v[8] = ((w[6] >> 12) | (w[7] << 20)) & FE_M26;
    h.v[9] = (w[7] >> 6) & FE_M25;
}

// canonical (< p) little-endian encoding of any element with limbs below 2^31
__device__ __forceinline__ void fe_encode(uint32_t (&w)[8], const Fe& f) {
    Fe h = f;
    fe_carry32(h);   // limbs 1..9 tight, limb 0 < 2^26 + 19 * 64
    fe_carry32(h);   // all tight: a carry out of limb 9 means limbs 1..9 were all ones, limb 0 is then small.  Value < 2^255.
    // q = 1 iff value >= p, i.e. iff value + 19 >= 2^255
    uint32_t q = (h.v[0] + 19u) >> 26;
#pragma unroll
    for (int i = 1; i < 10; i++) q = (h.v[i] + q) >> fe_bits(i);
    // value - q p = value + 19 q - q 2^255: add, carry, drop bit 255
    uint32_t c = 19u * q;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const uint32_t t = h.v[i] + c;
        c = t >> fe_bits(i);
        h.v[i] = t & fe_mask(i);
    }
    w[0] = h.v[0] | (h.v[1] << 26);
    w[1] = (h.v[1] >> 6) | (h.v[2] << 19);
    w[2] = (h.v[2] >> 13) | (h.v[3] << 13);
    w[3] = (h.v[3] >> 19) | (h.v[4] << 6);
    w[4] = h.v[5] | (h.v[6] << 25);
    w[5] = (h.v[6] >> 7) | (h.v[7] << 19);
    w[6] = (h.v[7] >> 13) | (h.v[8] << 12);
    w[7] = (h.v[8] >> 20) | (h.v[9] << 6);
}

// The Montgomery ladder (RFC 7748 section 5, a24 = 121665) on the clamped scalar k and the u-coordinate x1; BASE: x1 = 9, so
// that the product by x1 is a product by a constant.  out = canonical encoding of x2 * z2^(p-2).
template <bool BASE>
__device__ __forceinline__ void x25519_ladder(uint32_t (&out)[8], const uint32_t (&k)[8], const uint32_t (&u)[8]) {
    Fe x1, x2, z2, x3, z3;
    if (BASE) fe_set(x1, 9);
    else fe_decode(x1, u);
    fe_set(x2, 1);
    fe_set(z2, 0);
    x3 = x1;
    fe_set(z3, 1);
    uint32_t swap = 0;
#pragma unroll 1
    for (int wi = 7; wi >= 0; wi--) {
        // the scalar word of this round: selected by the (public) loop counter, no indexed register access
        uint32_t kw = k[0];
#pragma unroll
        for (int j = 1; j < 8; j++) kw = (wi == j) ? k[j] : kw;
        if (wi == 7) kw = (kw & 0x7FFFFFFFu) | 0x40000000u;   // clamp: bit 255 clear, bit 254 set
        if (wi == 0) kw &= 0xFFFFFFF8u;                        //        bits 0..2 clear
#pragma unroll 1
        for (int b = (wi == 7 ? 30 : 31); b >= 0; b--) {
            const uint32_t bit = (kw >> b) & 1u;
            swap ^= bit;
            const uint32_t mask = 0u - swap;
            fe_cswap(x2, x3, mask);
            fe_cswap(z2, z3, mask);
            swap = bit;
            Fe A, B, C, D, AA, BB, E, DA, CB, t;
            fe_add(A, x2, z2);
            fe_sub(B, x2, z2);
            fe_add(C, x3, z3);
            fe_sub(D, x3, z3);
            fe_sq(AA, A);
            fe_sq(BB, B);
            fe_mul(DA, D, A);
            fe_mul(CB, C, B);
            fe_sub(E, AA, BB);
            fe_add(t, DA, CB);
            fe_sq(x3, t);
            fe_sub(t, DA, CB);
            fe_sq(t, t);
            if (BASE) fe_mul_small<9>(z3, t);
            else fe_mul(z3, x1, t);
            fe_mul(x2, AA, BB);
            fe_mul_small<121665>(t, E);
            fe_add(t, t, AA);
            fe_mul(z2, E, t);
        }
    }
    const uint32_t mask = 0u - swap;
    fe_cswap(x2, x3, mask);
    fe_cswap(z2, z3, mask);
    Fe zi, r;
    fe_invert(zi, z2);
    fe_mul(r, x2, zi);
    fe_encode(out, r);
}

// ------------------------------------------------------------------------------------------------
// k_x25519 — out0[i] = X25519(scalar[i], BASE0 ? 9 : u0[i]) in blocks [0, nblk), and, when the grid has 2 nblk blocks,
// out1[i] = X25519(scalar[i], u1[i]) in blocks [nblk, 2 nblk): the two multiplications of an Encaps item share the scalar and one
// launch (the block index, not data, picks the side).  Every array has its own row stride (wire rows are read and written in place).
// status (or null) belongs to side 0: MLKEM_ERR_LOW_ORDER (-7) where the output is all zero, else 0.
// ------------------------------------------------------------------------------------------------
constexpr int32_t X25519_LOW_ORDER = -7;

template <bool BASE0>
__global__ void __launch_bounds__(WAVE) k_x25519(size_t n, size_t nblk, const uint8_t* __restrict__ scalar, size_t scalar_stride,
                                                 const uint8_t* __restrict__ u0, size_t u0_stride, uint8_t* __restrict__ out0,
                                                 size_t out0_stride, const uint8_t* __restrict__ u1, size_t u1_stride,
                                                 uint8_t* __restrict__ out1, size_t out1_stride, int32_t* __restrict__ status) {
    const bool second = blockIdx.x >= nblk;   // wave-uniform
    const size_t item = ((size_t)blockIdx.x - (second ? nblk : 0)) * WAVE + lane_id();
    const size_t it = item < n ? item : n - 1;   // idle lanes repeat the last item and store nothing
    uint32_t k[8], u[8], r[8];
    load32(scalar, scalar_stride, it, k);
    if (second) {
        load32(u1, u1_stride, it, u);
        x25519_ladder<false>(r, k, u);
        if (item < n) store32(out1, out1_stride, item, r);
        return;
    }
    if (BASE0) {
#pragma unroll
        for (int i = 0; i < 8; i++) u[i] = 0;
    } else {
        load32(u0, u0_stride, it, u);
    }
    x25519_ladder<BASE0>(r, k, u);
    if (item < n) {
        store32(out0, out0_stride, item, r);
        if (status) {
            uint32_t any = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) any |= r[i];
            status[item] = any ? 0 : X25519_LOW_ORDER;
        }
    }
}

}   // namespace mlkem
