// mlkem_xwing.hpp — the X-Wing hybrid KEM (ML-KEM-768 + X25519 + a SHA3-256 combiner) over device-resident batches.
//
//   Label = 5c 2e 2f 2f 5e 5c
//   expand(sk[32]):  e = SHAKE256(sk, 96);  d = e[0:32], z = e[32:64], sk_X = e[64:96]
//                    (pk_M, dk_M) = ML-KEM-768.KeyGen_internal(d, z);  pk_X = X25519(sk_X, 9)
//   KeyGen(sk)            -> pk = pk_M || pk_X                                            (1216 bytes)
//   Encaps(pk, eseed[64]) -> (ct_M, ss_M) = ML-KEM-768.Encaps_internal(pk_M, eseed[0:32]); ek_X = eseed[32:64]
//                            ct_X = X25519(ek_X, 9); ss_X = X25519(ek_X, pk_X); ct = ct_M || ct_X   (1120 bytes)
//   Decaps(sk, ct)        -> expand(sk); ss_M = ML-KEM-768.Decaps_internal(dk_M, ct_M); ss_X = X25519(sk_X, ct_X)
//   ss = SHA3-256(ss_M || ss_X || ct_X || pk_X || Label)                                  (134-byte message: one permutation)
// ML-KEM here is always FIPS 203 (the caller passes a Workspace copy with fips set); there is no all-zero check on ss_X.
// The Keccak parts are one permutation each, one item per lane (k_xwing_expand, k_xwing_combine); the ML-KEM legs are the existing
// ML-KEM-768 dispatch functions, unchanged, on contiguous rows; k_xwing_rows moves the ML-KEM part of the wire rows to and from those.
// The X25519 kernels read and write the 32-byte tails of the wire rows in place (row strides 1216 / 1120 / 64).
// The run functions slice a call by the staging region a context owns and zero what they used of it before they return.
#pragma once
#include "mlkem_rng.hpp"
#include "mlkem_x25519.hpp"

namespace mlkem {

constexpr uint32_t RNG_DOM_XWING_SK = 0x03, RNG_DOM_XWING_ESEED = 0x04;   // generator domains (mlkem_rng.hpp): sk = block[:32], eseed = block[:64]
constexpr size_t XWING_PKM = 1184, XWING_CTM = 1088, XWING_PK = XWING_PKM + 32, XWING_CT = XWING_CTM + 32;
constexpr int XWING_SET = 768;

// ------------------------------------------------------------------------------------------------
// k_xwing_expand — e = SHAKE256(sk, 96): seed rows (d || z, 64 bytes: what decaps_seed_dispatch reads) and / or d rows and z rows
// (what keygen_dispatch reads), and the sk_X rows.  Null outputs are skipped.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE, MLKEM_KECCAK_MINWAVES) k_xwing_expand(size_t n, const uint8_t* __restrict__ sk, uint8_t* __restrict__ seed,
                                                                              uint8_t* __restrict__ d, uint8_t* __restrict__ z,
                                                                              uint8_t* __restrict__ skx) {
    const size_t item = (size_t)blockIdx.x * WAVE + lane_id();
    const size_t it = item < n ? item : n - 1;
    KeccakState s;
    uint32_t w[8];
    load32(sk, 32, it, w);
    keccak_zero(s);
    MLKEM_SET_WORDS8(s, 0, w)
    keccak_xor_byte<32>(s, 0x1F);
    keccak_xor_byte<135>(s, 0x80);
    keccak_f1600(s);
    if (item < n) {
        MLKEM_STATE_WORDS8(s, 0, w)
        if (seed) store32(seed, 64, item, w);
        if (d) store32(d, 32, item, w);
        MLKEM_STATE_WORDS8(s, 8, w)
        if (seed) store32(seed + 32, 64, item, w);
        if (z) store32(z, 32, item, w);
        MLKEM_STATE_WORDS8(s, 16, w)
        store32(skx, 32, item, w);
    }
}

// ------------------------------------------------------------------------------------------------
// k_xwing_combine — ss = SHA3-256(ss_M || ss_X || ct_X || pk_X || Label): the 134-byte message, the suffix 0x06 (byte 134) and the
// pad's last byte (135) are built in registers.  ct_X and pk_X are read from wire rows (or staged rows) with their strides.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE, MLKEM_KECCAK_MINWAVES) k_xwing_combine(size_t n, const uint8_t* __restrict__ ssm, const uint8_t* __restrict__ ssx,
                                                                               const uint8_t* __restrict__ ct_x, size_t ct_x_stride,
                                                                               const uint8_t* __restrict__ pk_x, size_t pk_x_stride,
                                                                               uint8_t* __restrict__ ss) {
    const size_t item = (size_t)blockIdx.x * WAVE + lane_id();
    const size_t it = item < n ? item : n - 1;
    KeccakState s;
    uint32_t w[8];
    keccak_zero(s);
    load32(ssm, 32, it, w);
    MLKEM_SET_WORDS8(s, 0, w)
    load32(ssx, 32, it, w);
    MLKEM_SET_WORDS8(s, 8, w)
    load32(ct_x, ct_x_stride, it, w);
    MLKEM_SET_WORDS8(s, 16, w)
    load32(pk_x, pk_x_stride, it, w);
    MLKEM_SET_WORDS8(s, 24, w)
    keccak_word<32>(s) = 0x2F2F2E5Cu;   // Label[0:4]
    keccak_word<33>(s) = 0x80065C5Eu;   // Label[4:6], 0x06, 0x80
    keccak_f1600(s);
    if (item < n) {
        MLKEM_STATE_WORDS8(s, 0, w)
        store32(ss, 32, item, w);
    }
}

// n rows of 16 * row16 bytes from one row stride to another (both multiples of 16, bases 16-byte aligned): one uint4 per thread
__global__ void __launch_bounds__(256) k_xwing_rows(size_t n, unsigned row16, const uint8_t* __restrict__ src, size_t src_stride,
                                                    uint8_t* __restrict__ dst, size_t dst_stride) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t row = idx / row16, col = idx - row * row16;
    if (row >= n) return;
    *reinterpret_cast<uint4*>(dst + row * dst_stride + col * 16) = *reinterpret_cast<const uint4*>(src + row * src_stride + col * 16);
}

inline void xwing_rows_launch(stream_t st, size_t n, size_t row_bytes, const uint8_t* src, size_t src_stride, uint8_t* dst, size_t dst_stride) {
    const unsigned row16 = (unsigned)(row_bytes / 16);
    launch("k_xwing_rows", k_xwing_rows, ceil_div(n * row16, 256), 256, st, n, row16, src, src_stride, dst, dst_stride);
}

// out[i] = X25519(scalar[i], u[i]), u == null: the base point
inline void x25519_launch(stream_t st, size_t n, const uint8_t* scalar, size_t scalar_stride, const uint8_t* u, size_t u_stride, uint8_t* out,
                          size_t out_stride, int32_t* status) {
    const size_t nblk = ceil_div(n, WAVE);
    if (u) launch("k_x25519", k_x25519<false>, nblk, WAVE, st, n, nblk, scalar, scalar_stride, u, u_stride, out, out_stride, (const uint8_t*)nullptr, (size_t)0, (uint8_t*)nullptr, (size_t)0, status);
    else launch("k_x25519", k_x25519<true>, nblk, WAVE, st, n, nblk, scalar, scalar_stride, (const uint8_t*)nullptr, (size_t)0, out, out_stride, (const uint8_t*)nullptr, (size_t)0, (uint8_t*)nullptr, (size_t)0, status);
}
// base[i] = X25519(scalar[i], 9) and out[i] = X25519(scalar[i], u[i]) in ONE launch of twice the blocks
inline void x25519_pair_launch(stream_t st, size_t n, const uint8_t* scalar, size_t scalar_stride, uint8_t* base, size_t base_stride,
                               const uint8_t* u, size_t u_stride, uint8_t* out, size_t out_stride) {
    const size_t nblk = ceil_div(n, WAVE);
    launch("k_x25519", k_x25519<true>, 2 * nblk, WAVE, st, n, nblk, scalar, scalar_stride, (const uint8_t*)nullptr, (size_t)0, base, base_stride, u, u_stride, out, out_stride, (int32_t*)nullptr);
}

// The staging region of the X-Wing calls, for `items` items: rows the ML-KEM dispatch functions and the combiner take.
//   seed (d || z) 64 | d 32 | z 32 | sk_X or ek_X 32 | m 32 | ss_M 32 | ss_X 32 | pk_X 32 | pk_M 1184 | ct_M 1088
constexpr size_t XWING_STAGE_ITEM_BYTES = 64 + 7 * 32 + XWING_PKM + XWING_CTM;
// Items per slice at most: the region of a context is min(chunk_items, this) items (671 MB at most).  At 2^20 items slices of 2^14 /
// 2^15 / 2^16 / 2^17 / 2^18 items take 58.1 / 32.5 / 29.3 / 23.8 / 18.3 ms (KeyGen) and 62.5 / 53.8 / 40.7 / 30.2 / 29.3 ms (Encaps): the
// ML-KEM kernels of a short slice leave the chip half empty (profiles/xwing.txt; env MLKEM_XWING_SLICE_ITEMS lowers it).
constexpr size_t XWING_SLICE_MAX = (size_t)1 << 18;
struct XwingStage {
    uint8_t* base = nullptr;
    size_t items = 0;          // slice size of this call: min(n, the region's capacity)
    uint8_t* dk_stage = nullptr;   // the seed-format staging region (seed_stage_bytes(ML-KEM-768) x items at least): KeyGen's dk, Decaps' d, z, ek, dk
    uint8_t* seed() const { return base; }
    uint8_t* d() const { return base + items * 64; }
    uint8_t* z() const { return base + items * 96; }
    uint8_t* skx() const { return base + items * 128; }
    uint8_t* m() const { return base + items * 160; }
    uint8_t* ssm() const { return base + items * 192; }
    uint8_t* ssx() const { return base + items * 224; }
    uint8_t* pkx() const { return base + items * 256; }
    uint8_t* pkm() const { return base + items * 288; }
    uint8_t* ctm() const { return base + items * (288 + XWING_PKM); }
    size_t used() const { return items * XWING_STAGE_ITEM_BYTES; }
};

// blocks of the generator in the two X-Wing domains: sk rows (out0), or m rows (out0) and ek_X rows (out1) of an eseed
inline void xwing_derive_launch(stream_t st, bool eseed, size_t n, const uint8_t* root, uint64_t pos, uint8_t* out0, uint8_t* out1, size_t wide_max) {
    const uint32_t dom = eseed ? RNG_DOM_XWING_ESEED : RNG_DOM_XWING_SK;
    uint8_t* none = nullptr;
    if (n <= wide_max) {
        if (eseed) launch("k_rng_derive", k_rng_derive_w<true>, n, WAVE, st, n, root, dom, pos, out0, out1, none);
        else launch("k_rng_derive", k_rng_derive_w<false>, n, WAVE, st, n, root, dom, pos, out0, none, none);
    } else {
        if (eseed) launch("k_rng_derive", k_rng_derive<true>, ceil_div(n, WAVE), WAVE, st, n, root, dom, pos, out0, out1, none);
        else launch("k_rng_derive", k_rng_derive<false>, ceil_div(n, WAVE), WAVE, st, n, root, dom, pos, out0, none, none);
    }
}

// ---- X-Wing.KeyGen: sk (n x 32) -> pk (n x 1216).  The expanded dk_M of a slice goes to g.dk_stage and is zeroed, as in
// keygen_random_run with dk == nullptr.  Returns nonzero when a zeroing could not be queued.
inline int xwing_keygen_run(stream_t st, size_t n, const XwingStage& g, const uint8_t* sk, uint8_t* pk, const Workspace& ws) {
    if (n == 0) return 0;
    for (size_t s0 = 0; s0 < n; s0 += g.items) {
        const size_t sn = min_sz(g.items, n - s0);
        uint8_t* pks = pk + s0 * XWING_PK;
        launch("k_xwing_expand", k_xwing_expand, ceil_div(sn, WAVE), WAVE, st, sn, sk + s0 * 32, (uint8_t*)nullptr, g.d(), g.z(), g.skx());
        keygen_dispatch(st, XWING_SET, sn, g.d(), g.z(), g.pkm(), g.dk_stage, ws);
        xwing_rows_launch(st, sn, XWING_PKM, g.pkm(), XWING_PKM, pks, XWING_PK);
        x25519_launch(st, sn, g.skx(), 32, nullptr, 0, pks + XWING_PKM, XWING_PK, nullptr);
    }
    bool ok = rng_zero(st, g.base, g.used());
    ok = rng_zero(st, g.dk_stage, g.items * (size_t)2400) && ok;
    return ok ? 0 : 1;
}

// ---- X-Wing.Encaps: pk (n x 1216) and eseed (n x 64), or, with eseed == nullptr, the generator `rng` (positions rng->pos ..,
// domain 0x04) -> ct (n x 1120), ss (n x 32); status (or null) as encaps_run's mod_status in FIPS 203 mode
inline int xwing_encaps_run(stream_t st, size_t n, const XwingStage& g, const uint8_t* pk, const uint8_t* eseed, const RngCall* rng, uint8_t* ct,
                            uint8_t* ss, int32_t* status, const Workspace& ws) {
    if (n == 0) return 0;
    for (size_t s0 = 0; s0 < n; s0 += g.items) {
        const size_t sn = min_sz(g.items, n - s0);
        const uint8_t* pks = pk + s0 * XWING_PK;
        uint8_t* cts = ct + s0 * XWING_CT;
        const uint8_t* ekx;
        size_t ekx_stride;
        if (eseed) {
            xwing_rows_launch(st, sn, 32, eseed + s0 * 64, 64, g.m(), 32);
            ekx = eseed + s0 * 64 + 32;
            ekx_stride = 64;
        } else {
            xwing_derive_launch(st, true, sn, rng->root, rng->pos + s0, g.m(), g.skx(), rng->wide_max);
            ekx = g.skx();
            ekx_stride = 32;
        }
        xwing_rows_launch(st, sn, XWING_PKM, pks, XWING_PK, g.pkm(), XWING_PKM);
        encaps_dispatch(st, XWING_SET, sn, g.pkm(), g.m(), g.ctm(), g.ssm(), status ? status + s0 : nullptr, ws);
        xwing_rows_launch(st, sn, XWING_CTM, g.ctm(), XWING_CTM, cts, XWING_CT);
        x25519_pair_launch(st, sn, ekx, ekx_stride, cts + XWING_CTM, XWING_CT, pks + XWING_PKM, XWING_PK, g.ssx(), 32);
        launch("k_xwing_combine", k_xwing_combine, ceil_div(sn, WAVE), WAVE, st, sn, (const uint8_t*)g.ssm(), (const uint8_t*)g.ssx(),
               (const uint8_t*)(cts + XWING_CTM), XWING_CT, pks + XWING_PKM, XWING_PK, ss + s0 * 32);
    }
    return rng_zero(st, g.base, g.used()) ? 0 : 1;
}

// ---- X-Wing.Decaps: sk (n x 32), ct (n x 1120) -> ss (n x 32).  pk (n x 1216, or null): pk_X is read from its last 32 bytes
// instead of being recomputed from sk_X (a wrong pk gives a wrong ss silently).  g.dk_stage is used by calls above ML-KEM-768's
// small_max only; smaller ones decapsulate in one launch with the expanded key in LDS only.
inline int xwing_decaps_run(stream_t st, size_t n, const XwingStage& g, const uint8_t* sk, const uint8_t* ct, const uint8_t* pk, uint8_t* ss,
                            const Workspace& ws) {
    if (n == 0) return 0;
    ParamSet p;
    (void)param_set(XWING_SET, p);
    const bool big = n > ws.small_max(p.k);
    for (size_t s0 = 0; s0 < n; s0 += g.items) {
        const size_t sn = min_sz(g.items, n - s0);
        const uint8_t* cts = ct + s0 * XWING_CT;
        launch("k_xwing_expand", k_xwing_expand, ceil_div(sn, WAVE), WAVE, st, sn, sk + s0 * 32, g.seed(), (uint8_t*)nullptr, (uint8_t*)nullptr, g.skx());
        xwing_rows_launch(st, sn, XWING_CTM, cts, XWING_CT, g.ctm(), XWING_CTM);
        decaps_seed_dispatch(st, XWING_SET, sn, g.seed(), g.ctm(), g.ssm(), big ? g.dk_stage : nullptr, big ? g.items : 0, ws);
        const uint8_t* pkx;
        size_t pkx_stride;
        if (pk) {
            x25519_launch(st, sn, g.skx(), 32, cts + XWING_CTM, XWING_CT, g.ssx(), 32, nullptr);
            pkx = pk + s0 * XWING_PK + XWING_PKM;
            pkx_stride = XWING_PK;
        } else {
            x25519_pair_launch(st, sn, g.skx(), 32, g.pkx(), 32, cts + XWING_CTM, XWING_CT, g.ssx(), 32);
            pkx = g.pkx();
            pkx_stride = 32;
        }
        launch("k_xwing_combine", k_xwing_combine, ceil_div(sn, WAVE), WAVE, st, sn, (const uint8_t*)g.ssm(), (const uint8_t*)g.ssx(),
               cts + XWING_CTM, XWING_CT, pkx, pkx_stride, ss + s0 * 32);
    }
    bool ok = rng_zero(st, g.base, g.used());
    if (big) ok = rng_zero(st, g.dk_stage, g.items * seed_stage_bytes(p)) && ok;
    return ok ? 0 : 1;
}

}   // namespace mlkem
