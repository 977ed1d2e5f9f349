// mlkem_check.hpp — key validation (mlkem_check_keys_dev): the structural check kernel k_check_keys.
//
// One checking wave per item reads the item's ek and dk once and ORs every check whose inputs are present into ONE status store:
//   EK_MODULUS   a ByteDecode_12 coefficient of ek's t-hat >= q                       (FIPS 203 §7.2)
//   DK_MODULUS   the same for the ek embedded in dk                                   (FIPS 203 §7.2 on dk.ek)
//   DK_HASH      H(dk.ek) != dk.h                                                     (FIPS 203 §7.3)
//   EK_MISMATCH  dk.ek != ek
//   SEED         the staged KeyGen_internal(d, z) output != ek / dk
//   PCT          the staged K of Encaps != the staged K' of Decaps
// Work of a wave (T = 16 K + 8 tasks over its 64 lanes, two rounds at K = 4):
//   tasks [0, 8K)     48-byte pieces of t-hat (16 ByteDecode_12 triples = 32 coefficients): ek, dk.ek, the staged ek
//   tasks [8K, 16K)   48-byte pieces of dk_pke against the staged dk (seed leg only)
//   tasks 16K + u     16-byte halves of rho (u = 0, 1), h (2, 3), z (4, 5), K against K' (6, 7)
// H(dk.ek): with HASH (calls of at most ws.wide_kem(K) items) a workgroup of two waves takes one item: wave 0 computes H on the
// one-sponge-per-wave Keccak (mlkem_wkeccak.hpp) straight from dk.ek, so that its chain of 9 / 12 / 13 permutations starts at
// once, while wave 1 runs the structural pass; one barrier and one LDS word join them before wave 1 stores the status.  dk.ek
// is then read twice, the second time from L2.  The LDS holds the round-constant table and that word, nothing of a key.
// Without HASH (four items per workgroup, one per wave), h_calc holds H(dk.ek) from the lane-sliced k_hash_batch<0>
// (mlkem_pipeline.hpp: check_keys_run).  dk_pke, z and K stay in registers in both forms.
#pragma once
#include "mlkem_wkeccak.hpp"
#include "mlkem_small.hpp"

namespace mlkem {

constexpr int32_t KEYCHECK_EK_MODULUS = 1, KEYCHECK_DK_MODULUS = 2, KEYCHECK_DK_HASH = 4, KEYCHECK_EK_MISMATCH = 8,
                  KEYCHECK_SEED = 16, KEYCHECK_PCT = 32;

__device__ __forceinline__ void load48(const uint8_t* p, uint4 (&v)[3]) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
}
__device__ __forceinline__ uint32_t diff48(const uint4 (&a)[3], const uint4 (&b)[3]) {
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 3; j++) d |= (a[j].x ^ b[j].x) | (a[j].y ^ b[j].y) | (a[j].z ^ b[j].z) | (a[j].w ^ b[j].w);
    return d;
}
__device__ __forceinline__ uint32_t diff16(const uint4& a, const uint4& b) { return (a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w); }
// any of the 32 ByteDecode_12 coefficients of 48 bytes >= q (coefficient c = bits [12 c, 12 c + 12) of the little-endian string)
__device__ __forceinline__ bool over_q48(const uint4 (&v)[3]) {
    const uint32_t w[13] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w, v[2].x, v[2].y, v[2].z, v[2].w, 0u};
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 32; c++) {
        const int b = 12 * c, i = b >> 5, s = b & 31;
        const uint32_t x = (s <= 20 ? (w[i] >> s) : __builtin_amdgcn_alignbit(w[i + 1], w[i], s)) & 0xFFFu;
        bad |= x >= (uint32_t)KQ;
    }
    return bad;
}

// ------------------------------------------------------------------------------------------------
// k_check_keys — ek / dk: n rows or nullptr; h_calc: H(dk.ek) per item (unused with HASH); sek / sdk: the staged KeyGen output of
// the seed leg or nullptr; Kc / Kd: the staged K of Encaps and K' of Decaps or nullptr; status: n words, written once per item.
// HASH: one item per workgroup of two waves (grid n); otherwise four items per workgroup, one per wave (grid ceil(n / 4)).
// ------------------------------------------------------------------------------------------------
struct CheckHashLds {
    uint2 rc[WK_RC_ENTRIES];   // the sponge wave's round-constant table
    int32_t bad;               // H(dk.ek) != dk.h, from the sponge wave to the checking wave
};
template <int K, bool HASH>
__global__ void __launch_bounds__(HASH ? 2 * WAVE : 4 * WAVE) k_check_keys(size_t n, const uint8_t* __restrict__ ek, const uint8_t* __restrict__ dk,
                                                                           const uint8_t* __restrict__ h_calc, const uint8_t* __restrict__ sek,
                                                                           const uint8_t* __restrict__ sdk, const uint8_t* __restrict__ Kc,
                                                                           const uint8_t* __restrict__ Kd, int32_t* __restrict__ status) {
    constexpr unsigned EK = 384 * K + 32, DK = 768 * K + 96, T = 16 * K + 8;
    __shared__ CheckHashLds hl;
    const int w = wave_id();
    const size_t item = HASH ? (size_t)blockIdx.x : (size_t)blockIdx.x * 4 + (size_t)w;
    if (item >= n) return;   // (HASH: the whole workgroup, before its barrier)
    const uint8_t* d = dk ? dk + item * DK : nullptr;
    if (HASH && w == 0) {    // the sponge wave: H(dk.ek) against dk.h (Keccak lanes 0..3)
        bool bad = false;
        if (d) {
            WkLane c;
            wk_lane_init(c, hl.rc);
            WkState a;
            wk_absorb<136, 0x06>(a, c, d + 384 * K, EK, d + 384 * K, EK);
            const int i = wk_index();
            if (wk_primary() && i < 4) {
                const uint2 h = reinterpret_cast<const uint2*>(d + 768 * K + 32)[i];
                bad = h.x != a.lo || h.y != a.hi;
            }
        }
        const bool any = __ballot(bad) != 0;
        if (lane_id() == 0) hl.bad = any ? 1 : 0;
#ifdef MLKEM_EMU_LDS_PROBE
        if (lane_id() == 0) MLKEM_EMU_LDS_PROBE(&hl, sizeof hl);   // the CPU tier reads it back: constants and one flag
#endif
        block_barrier();
        return;
    }
    const unsigned l = (unsigned)lane_id();
    const uint8_t* e = ek ? ek + item * EK : nullptr;
    const uint8_t* se = sek ? sek + item * EK : nullptr;
    const uint8_t* sd = sdk ? sdk + item * DK : nullptr;
    bool ek_mod = false, dk_mod = false, mism = false, seed = false, hash = false, pct = false;
#pragma unroll 1
    for (unsigned t = l; t < T; t += WAVE) {
        if (t < 8 * K) {                                    // t-hat: ek, dk.ek, staged ek
            const unsigned off = 48 * t;
            uint4 a[3], b[3], s[3];
            if (e) { load48(e + off, a); ek_mod |= over_q48(a); }
            if (d) { load48(d + 384 * K + off, b); dk_mod |= over_q48(b); }
            if (e && d) mism |= diff48(a, b) != 0;
            if (se) {
                load48(se + off, s);
                if (e) seed |= diff48(a, s) != 0;
                if (d) seed |= diff48(b, s) != 0;
            }
        } else if (t < 16 * K) {                            // dk_pke against the staged dk
            if (d && sd) {
                const unsigned off = 48 * (t - 8 * K);
                uint4 b[3], s[3];
                load48(d + off, b);
                load48(sd + off, s);
                seed |= diff48(b, s) != 0;
            }
        } else {
            const unsigned u = t - 16 * K, half = 16 * (u & 1);
            if (u < 2) {                                    // rho
                uint4 a{}, b{}, s{};
                if (e) a = *reinterpret_cast<const uint4*>(e + 384 * K + half);
                if (d) b = *reinterpret_cast<const uint4*>(d + 768 * K + half);
                if (e && d) mism |= diff16(a, b) != 0;
                if (se) {
                    s = *reinterpret_cast<const uint4*>(se + 384 * K + half);
                    if (e) seed |= diff16(a, s) != 0;
                    if (d) seed |= diff16(b, s) != 0;
                }
            } else if (u < 6) {                             // h (u = 2, 3), z (u = 4, 5)
                if (d && (sd || (!HASH && u < 4))) {
                    const unsigned off = 768 * K + 32 + 32 * ((u - 2) >> 1) + half;
                    const uint4 b = *reinterpret_cast<const uint4*>(d + off);
                    if (!HASH && u < 4) hash |= diff16(b, *reinterpret_cast<const uint4*>(h_calc + item * 32 + half)) != 0;
                    if (sd) seed |= diff16(b, *reinterpret_cast<const uint4*>(sd + off)) != 0;
                }
            } else if (Kc) {                                // K of Encaps against K' of Decaps
                pct |= diff16(*reinterpret_cast<const uint4*>(Kc + item * 32 + half), *reinterpret_cast<const uint4*>(Kd + item * 32 + half)) != 0;
            }
        }
    }
    int32_t v = 0;
    v |= __ballot(ek_mod) ? KEYCHECK_EK_MODULUS : 0;
    v |= __ballot(dk_mod) ? KEYCHECK_DK_MODULUS : 0;
    v |= __ballot(hash) ? KEYCHECK_DK_HASH : 0;
    v |= __ballot(mism) ? KEYCHECK_EK_MISMATCH : 0;
    v |= __ballot(seed) ? KEYCHECK_SEED : 0;
    v |= __ballot(pct) ? KEYCHECK_PCT : 0;
    if (HASH) {   // join the sponge wave
        block_barrier();
        v |= hl.bad ? KEYCHECK_DK_HASH : 0;
    }
    if (l == 0) status[item] = v;
}

// k_gather_rows — n rows of `len` bytes (a multiple of 16) from a strided source into a packed array: dk.ek -> the ek rows
// Encaps takes (the PCT leg of a call without ek)
__global__ void __launch_bounds__(256) k_gather_rows(size_t n, const uint8_t* __restrict__ src, size_t src_stride, uint8_t* __restrict__ dst,
                                                     unsigned len) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x, per = len / 16;
    if (g >= n * per) return;
    const size_t item = g / per, q = g - item * per;
    reinterpret_cast<uint4*>(dst + item * len)[q] = reinterpret_cast<const uint4*>(src + item * src_stride)[q];
}

}   // namespace mlkem
