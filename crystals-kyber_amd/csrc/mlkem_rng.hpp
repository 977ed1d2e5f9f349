// mlkem_rng.hpp — device-side seed derivation: the randomised KeyGen / Encaps of device-resident batches.
//
// FIPS 203's KeyGen() and Encaps(ek) draw d, z (64 bytes) and m (32 bytes) per item.  Here they are derived on the device from a
// 32-byte root that lives in the context's device memory and a 64-bit position the host counts:
//   block(root, dom, pos) = SHAKE256(root[32] || dom[1] || LE64(pos))      41-byte message, rate 136, suffix 0x1F: ONE permutation
//   KeyGen item:  d || z = first 64 bytes of block(root, 0x01, pos)
//   Encaps item:  m      = first 32 bytes of block(root, 0x02, pos)
// The block is built in registers from the root pointer, the domain byte and the call's base position: the root is never replicated
// per item in memory, and d, z, m never exist in host memory or on the bus.  This is a SHAKE256 expansion of the root, not an
// SP 800-90A DRBG.
// Two forms, following the project's split (mlkem_kernels.hpp / mlkem_wkeccak.hpp):
//   k_rng_derive     lane-sliced, one item per SIMD lane on KeccakState / keccak_f1600 (throughput)
//   k_rng_derive_w   one sponge per wavefront on wk_permute (the chain of a small call: 2.6 against ~10 us per permutation)
// Both write the d and z rows (or the m rows) in the layouts keygen_run / encaps_run read, into a region the context owns, and the
// d || z rows of the caller's seed_out when it asks for them.  The run functions below slice a call by the region's size, run the
// existing seeded pipeline on every slice and zero the region (and the dk staging of the seed-only KeyGen) in stream order.
#pragma once
#include "mlkem_keyset.hpp"
#ifdef MLKEM_EMU
#include <string.h>
#endif

namespace mlkem {

constexpr uint32_t RNG_DOM_KEYGEN = 0x01, RNG_DOM_ENCAPS = 0x02;

// the three state words after the root: byte 32 = dom, bytes 33..40 = LE64(pos), byte 41 = the SHAKE suffix 0x1F
__device__ __forceinline__ uint32_t rng_word8(uint32_t dom, uint64_t pos) { return dom | ((uint32_t)pos << 8); }
__device__ __forceinline__ uint32_t rng_word9(uint64_t pos) { return (uint32_t)(pos >> 24); }
__device__ __forceinline__ uint32_t rng_word10(uint64_t pos) { return (uint32_t)(pos >> 56) | 0x1F00u; }

// ------------------------------------------------------------------------------------------------
// k_rng_derive — one item per lane.  KEYGEN: out0 = d rows, out1 = z rows (n x 32 each), seed_out = d || z rows (n x 64) or null;
// otherwise out0 = m rows.  Item i uses position pos0 + i (mod 2^64).
// ------------------------------------------------------------------------------------------------
template <bool KEYGEN>
__global__ void __launch_bounds__(WAVE, MLKEM_KECCAK_MINWAVES) k_rng_derive(size_t n, const uint8_t* __restrict__ root, uint32_t dom, uint64_t pos0,
                                                                            uint8_t* __restrict__ out0, uint8_t* __restrict__ out1,
                                                                            uint8_t* __restrict__ seed_out) {
    const size_t item = (size_t)blockIdx.x * WAVE + lane_id();
    const uint64_t pos = pos0 + item;
    KeccakState s;
    uint32_t rr[8], w[8];
    load32(root, 0, 0, rr);   // the same 32 bytes for every lane: scalar loads
    keccak_zero(s);
    MLKEM_SET_WORDS8(s, 0, rr)
    keccak_word<8>(s) = rng_word8(dom, pos);
    keccak_word<9>(s) = rng_word9(pos);
    keccak_word<10>(s) = rng_word10(pos);
    keccak_xor_byte<135>(s, 0x80);
    keccak_f1600(s);
    if (item < n) {
        MLKEM_STATE_WORDS8(s, 0, w)
        store32(out0, 32, item, w);
        if (KEYGEN && seed_out) store32(seed_out, 64, item, w);
        if (KEYGEN) {
            MLKEM_STATE_WORDS8(s, 8, w)
            store32(out1, 32, item, w);
            if (seed_out) store32(seed_out + 32, 64, item, w);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_rng_derive_w — one item per wave (blockIdx.x = item), arguments as k_rng_derive.  Keccak lanes 0..3 = root, 4 and 5 = dom,
// pos and the suffix, 16 = the pad's last byte; the output is lanes 0..3 (d or m) and 4..7 (z).
// ------------------------------------------------------------------------------------------------
template <bool KEYGEN>
__global__ void __launch_bounds__(WAVE) k_rng_derive_w(size_t n, const uint8_t* __restrict__ root, uint32_t dom, uint64_t pos0,
                                                       uint8_t* __restrict__ out0, uint8_t* __restrict__ out1, uint8_t* __restrict__ seed_out) {
    const size_t item = blockIdx.x;
    if (item >= n) return;
    __shared__ uint2 rc_table[WK_RC_ENTRIES];
    const int i = wk_index();
    WkLane c;
    wk_lane_init(c, rc_table);
    const uint64_t pos = pos0 + item;
    WkState a;
    a.lo = 0; a.hi = 0;
    if (i >= 0 && i < 4) {   // primaries and copies alike: the state is well-formed as loaded
        const uint2 v = reinterpret_cast<const uint2*>(root)[i];
        a.lo = v.x; a.hi = v.y;
    } else if (i == 4) {
        a.lo = rng_word8(dom, pos); a.hi = rng_word9(pos);
    } else if (i == 5) {
        a.lo = rng_word10(pos);
    } else if (i == 16) {
        a.hi = 0x80000000u;
    }
    wk_permute(a, c);
    uint2 o;
    o.x = a.lo; o.y = a.hi;
    if (!wk_primary() || i >= (KEYGEN ? 8 : 4)) return;
    if (i < 4) reinterpret_cast<uint2*>(out0 + item * 32)[i] = o;
    else reinterpret_cast<uint2*>(out1 + item * 32)[i - 4] = o;
    if (KEYGEN && seed_out) reinterpret_cast<uint2*>(seed_out + item * 64)[i] = o;
}

// Calls (slices) of at most this many items derive with one sponge per wavefront: where the forms cross on one MI355X.  us per
// launch, wave-wide against lane-sliced: 6.9 / 12.7 at 64 items, 10.4 / 14.8 at 2048, 14.2 / 14.6 at 4096, 17.3 / 14.5 at 6144,
// 32.6 / 14.6 at 16384 (tools/rng_latency.py --sweep, profiles/rng_latency.txt; LABNOTES "Device-side seed derivation").
// Env MLKEM_RNG_WIDE_ITEMS (0: always lane-sliced).
constexpr size_t RNG_WIDE_ITEMS = 4096;

inline void rng_derive_launch(stream_t st, bool keygen, size_t n, const uint8_t* root, uint64_t pos, uint8_t* out0, uint8_t* out1,
                              uint8_t* seed_out, size_t wide_max) {
    const uint32_t dom = keygen ? RNG_DOM_KEYGEN : RNG_DOM_ENCAPS;
    if (n <= wide_max) {
        if (keygen) launch("k_rng_derive", k_rng_derive_w<true>, n, WAVE, st, n, root, dom, (uint64_t)pos, out0, out1, seed_out);
        else launch("k_rng_derive", k_rng_derive_w<false>, n, WAVE, st, n, root, dom, (uint64_t)pos, out0, out1, seed_out);
    } else {
        if (keygen) launch("k_rng_derive", k_rng_derive<true>, ceil_div(n, WAVE), WAVE, st, n, root, dom, (uint64_t)pos, out0, out1, seed_out);
        else launch("k_rng_derive", k_rng_derive<false>, ceil_div(n, WAVE), WAVE, st, n, root, dom, (uint64_t)pos, out0, out1, seed_out);
    }
}

// zero `bytes` at p after everything queued on the stream so far; false when the runtime refuses
inline bool rng_zero(stream_t st, void* p, size_t bytes) {
#ifdef MLKEM_EMU
    (void)st;
    memset(p, 0, bytes);
    return true;
#else
    return hipMemsetAsync(p, 0, bytes, st) == hipSuccess;
#endif
}

// The generator of one call: the root in device memory, the call's first position, the context's derived-seed region of
// slice_items x 64 bytes (slice_items = min(n, chunk items): d rows then z rows, or m rows) and the form switch.
struct RngCall {
    const uint8_t* root = nullptr;
    uint64_t pos = 0;
    uint8_t* seeds = nullptr;
    size_t slice_items = 0;
    size_t wide_max = RNG_WIDE_ITEMS;
};

// ---- ML-KEM.KeyGen(): items pos .. pos + n - 1 of the KeyGen domain -> ek, dk (n x dk_len, or null) and seed_out (n x 64, or null).
// dk == null: the expanded dk of every slice goes to `dk_stage` (slice_items x dk_len: the staging region of the seed-format
// Decaps), zeroed before the call returns control of it.  Returns nonzero when a zeroing could not be queued.
inline int keygen_random_run(stream_t st, const ParamSet& p, size_t n, const RngCall& g, uint8_t* ek, uint8_t* dk, uint8_t* seed_out,
                             uint8_t* dk_stage, const Workspace& ws) {
    if (n == 0) return 0;
    uint8_t *d = g.seeds, *z = d + g.slice_items * 32;
    for (size_t s0 = 0; s0 < n; s0 += g.slice_items) {
        const size_t sn = min_sz(g.slice_items, n - s0);
        rng_derive_launch(st, true, sn, g.root, g.pos + s0, d, z, seed_out ? seed_out + s0 * 64 : nullptr, g.wide_max);
        keygen_dispatch(st, p.set, sn, d, z, ek + s0 * p.ek_len, dk ? dk + s0 * p.dk_len : dk_stage, ws);
    }
    bool ok = rng_zero(st, g.seeds, g.slice_items * 64);
    if (!dk) ok = rng_zero(st, dk_stage, g.slice_items * (size_t)p.dk_len) && ok;
    return ok ? 0 : 1;
}

// ---- ML-KEM.Encaps(ek): items pos .. pos + n - 1 of the Encaps domain; mod_status as encaps_run takes it
inline int encaps_random_run(stream_t st, const ParamSet& p, size_t n, const RngCall& g, const uint8_t* ek, uint8_t* c, uint8_t* K,
                             int32_t* mod_status, const Workspace& ws) {
    if (n == 0) return 0;
    for (size_t s0 = 0; s0 < n; s0 += g.slice_items) {
        const size_t sn = min_sz(g.slice_items, n - s0);
        rng_derive_launch(st, false, sn, g.root, g.pos + s0, g.seeds, nullptr, nullptr, g.wide_max);
        encaps_dispatch(st, p.set, sn, ek + s0 * p.ek_len, g.seeds, c + s0 * p.c_len, K + s0 * 32, mod_status ? mod_status + s0 : nullptr, ws);
    }
    return rng_zero(st, g.seeds, g.slice_items * 32) ? 0 : 1;
}

// ---- the same to the keys of a prepared set (encaps_keyset_run): an out-of-range index still consumes its position
inline int encaps_keyset_random_run(stream_t st, const ParamSet& p, const KeysetView& ks, size_t n, const RngCall& g, const uint32_t* idx,
                                    uint8_t* c, uint8_t* K, int32_t* status, const Workspace& ws, const KeysetLimits& lim) {
    if (n == 0) return 0;
    for (size_t s0 = 0; s0 < n; s0 += g.slice_items) {
        const size_t sn = min_sz(g.slice_items, n - s0);
        rng_derive_launch(st, false, sn, g.root, g.pos + s0, g.seeds, nullptr, nullptr, g.wide_max);
        encaps_keyset_dispatch(st, p, ks, sn, idx ? idx + s0 : nullptr, g.seeds, c + s0 * p.c_len, K + s0 * 32, status ? status + s0 : nullptr, ws, lim);
    }
    return rng_zero(st, g.seeds, g.slice_items * 32) ? 0 : 1;
}

}   // namespace mlkem
