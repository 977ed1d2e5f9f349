// mlkem_sha3r.hpp — SHA-3 / SHAKE over a device-resident batch of messages of UNEQUAL length (mlkem_sha3_ragged_dev).
//
// Message i = head row i (a fixed-length, 8-byte aligned prefix: typically the K rows an Encaps / Decaps call has just written)
// followed by body[body_off[i] .. + body_len[i]), which may start at ANY byte address.  Every message has its own length, so
// everything the equal-length kernels keep wave-uniform (block count, position of the suffix byte, last block) is per item here.
// Two forms, following the project's split (mlkem_kernels.hpp / mlkem_wkeccak.hpp):
//   k_sha3_ragged<RATE>   lane-sliced, one sponge per SIMD lane on KeccakState / keccak_f1600 (throughput)
//   k_sha3_ragged_w       one sponge per wavefront on wk_permute (the dependency chain of a call of few messages)
//
// How message bytes reach the state, in both forms: the body is read with naturally aligned 8-byte loads of the qwords that hold
// it and two neighbouring qwords are funnel-shifted by the body's own byte offset (8 * (address & 7) bits) into the 8 message
// bytes a Keccak lane absorbs; bytes past the message's end are masked to zero.  A qword is loaded only if it holds at least one
// byte of the item's own body (or head), so an item is never read before the aligned qword of its first byte or past the one of
// its last: a body may begin at the first and end at the last byte of an allocation.  A zero-length body and an out-of-bounds
// item issue no body load at all.  Neither form puts message bytes in LDS (the wave-wide form's only LDS is the round-constant
// table, which it clears before it exits).
// Control flow and addresses depend on lengths and offsets only, never on message bytes: the head may be a secret.
//
// Load balance: a wave of the lane-sliced form runs as long as its longest message (the other lanes idle through the extra
// permutations); there is no sorting or binning pass.  Callers with very skewed lengths should group messages of similar length.
#pragma once
#include "mlkem_wkeccak.hpp"

// the CPU tier records every message load (item, address, width) through this hook (tests/emu/emu_sha3r.cpp)
#ifndef MLKEM_EMU_LOAD_PROBE
#define MLKEM_EMU_LOAD_PROBE(item, p, bytes)
#endif

namespace mlkem {

constexpr int SHA3R_ERR_ARG = -101;   // MLKEM_ERR_ARG as a per-item status
// Calls of at most this many messages run one sponge per wavefront: the call has a limit of its own, because the forms cross well
// above the 2048 of the stand-alone sponge calls (ws.wide_max).  us per call, wave-wide / lane-sliced, SHA3-256: a 32-byte head +
// a body uniform in [0, 256]: 14.2 / 40.3 at 2048 items, 20.7 / 38.8 at 4096, 33.0 / 38.7 at 8192, 55.1 / 38.5 at 16384; messages of
// 1184 bytes: 41.7 / 105.0 at 2048, 70.8 / 100.2 at 4096, 127.6 / 100.0 at 8192 (tools/sha3_ragged_bench.py section (c),
// profiles/sha3_ragged.txt).  4096 is the largest measured size at which the wave-wide form wins for both shapes.
// Env MLKEM_SHA3_WIDE_ITEMS (0: always lane-sliced).
constexpr size_t SHA3R_WIDE_ITEMS = 4096;

// alg: 0..3 = SHA3-224 / 256 / 384 / 512, 4 = SHAKE128, 5 = SHAKE256 (include/mlkem_batch.h).  digest = 0: any output length.
inline bool sha3r_alg(int alg, unsigned& rate, unsigned& digest, uint32_t& suffix) {
    switch (alg) {
    case 0: rate = 144; digest = 28; suffix = 0x06; return true;
    case 1: rate = 136; digest = 32; suffix = 0x06; return true;
    case 2: rate = 104; digest = 48; suffix = 0x06; return true;
    case 3: rate = 72; digest = 64; suffix = 0x06; return true;
    case 4: rate = 168; digest = 0; suffix = 0x1F; return true;
    case 5: rate = 136; digest = 0; suffix = 0x1F; return true;
    default: return false;
    }
}

struct Sha3rArgs {
    size_t n;
    const uint8_t* head; unsigned head_len; size_t head_stride;            // head_len % 8 == 0, base and stride 8-byte aligned
    const uint8_t* body; size_t body_bytes;
    const uint64_t* body_off; const uint32_t* body_len;
    uint8_t* out; unsigned outlen; size_t out_stride;                      // out 16-byte aligned, out_stride % 4 == 0
    int32_t* status;                                                       // or null
    uint32_t suffix;                                                       // 0x06 (SHA-3) / 0x1F (SHAKE)
};

// the argument rules of mlkem_sha3_ragged_dev (include/mlkem_batch.h), shared by the C-ABI and the CPU tier; fills rate and a.suffix
inline bool sha3r_check_args(int alg, Sha3rArgs& a, unsigned& rate) {
    unsigned digest = 0;
    if (!sha3r_alg(alg, rate, digest, a.suffix)) return false;
    if (digest ? a.outlen != digest : (a.outlen < 1 || a.outlen > 65536)) return false;
    if (a.n == 0) return true;
    if (!a.head) a.head_len = 0;
    if (!a.out || !a.body_off || !a.body_len || (!a.body && a.body_bytes)) return false;
    if (a.head_len % 8 || a.head_len >= (1u << 31)) return false;
    if (a.head_len && ((reinterpret_cast<uintptr_t>(a.head) & 7u) || a.head_stride % 8 || a.head_stride < a.head_len)) return false;
    if ((reinterpret_cast<uintptr_t>(a.body_off) & 7u) || (reinterpret_cast<uintptr_t>(a.body_len) & 3u)) return false;
    if ((reinterpret_cast<uintptr_t>(a.out) & 15u) || a.out_stride % 4 || a.out_stride < a.outlen) return false;
    if (a.status && (reinterpret_cast<uintptr_t>(a.status) & 3u)) return false;
    return true;
}

// one message as its kernel sees it
struct Sha3rItem {
    const uint8_t* head;    // the item's head row
    const uint8_t* bodyq;   // the aligned qword that holds the body's first byte
    unsigned shift;         // 8 * (address of the body's first byte & 7): bits the body sits above that qword's start
    unsigned len, total;    // body bytes, head + body bytes
    bool bad;               // body out of bounds (or the message 2^31 bytes or longer): nothing of it is read
};
__device__ __forceinline__ Sha3rItem sha3r_item(const Sha3rArgs& a, size_t item) {
    Sha3rItem it;
    const uint64_t off = a.body_off[item];
    const uint32_t len = a.body_len[item];
    // off + len > body_bytes without forming the sum (it may not wrap at 2^64)
    it.bad = off > (uint64_t)a.body_bytes || (uint64_t)len > (uint64_t)a.body_bytes - off || (uint64_t)a.head_len + len >= (1ull << 31);
    const uint8_t* first = a.body + (it.bad ? 0 : off);
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(first) & 7u);
    it.bodyq = first - mis;      // (derived from `body` by arithmetic, so the loads stay global loads)
    it.shift = 8u * mis;
    it.len = it.bad ? 0u : len;
    it.total = it.bad ? 0u : a.head_len + len;
    it.head = a.head + item * a.head_stride;   // never dereferenced when head_len = 0
    return it;
}

// the one way message bytes are read: a naturally aligned 8-byte load
__device__ __forceinline__ uint64_t sha3r_ld8(size_t item, const uint8_t* p) {
    (void)item;
    MLKEM_EMU_LOAD_PROBE(item, p, 8);
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    return (uint64_t)v.x | ((uint64_t)v.y << 32);
}
// 8 message bytes out of two neighbouring aligned qwords: those `shift` bits (a multiple of 8, < 64) above the start of `lo`
__device__ __forceinline__ uint64_t sha3r_funnel(uint64_t lo, uint64_t hi, unsigned shift) {
    return shift ? (lo >> shift) | (hi << (64u - shift)) : lo;
}
// keep the bytes of the qword at message position p that lie before the message's end `total` (none when p >= total)
__device__ __forceinline__ uint64_t sha3r_keep(uint64_t v, unsigned total, unsigned p) {
    const unsigned nbytes = p >= total ? 0u : total - p;
    return nbytes >= 8u ? v : (nbytes == 0u ? 0ull : v & ((1ull << (8u * nbytes)) - 1ull));
}
// does the aligned qword 8 bytes after the one holding body position j (j % 8 == 0) hold a byte of the body?
__device__ __forceinline__ bool sha3r_next_has_body(const Sha3rItem& it, unsigned j) { return j + 8u < it.len + (it.shift >> 3); }

// zero the `outlen` bytes of an output row (4-byte aligned): lane `l` of `nl` cooperating lanes
__device__ __forceinline__ void sha3r_zero_row(uint8_t* o, unsigned outlen, unsigned l, unsigned nl) {
    for (unsigned w = l; 4u * w + 4u <= outlen; w += nl) *reinterpret_cast<uint32_t*>(o + 4u * w) = 0u;
    if (l == 0)
        for (unsigned b = outlen & ~3u; b < outlen; b++) o[b] = 0;
}

// xor `v` into state dword `w` (per lane, w < RATE / 4): selects, not a dynamic index (which would put the state in scratch)
template <int RATE>
__device__ __forceinline__ void sha3r_xor_word(KeccakState& s, unsigned w, uint32_t v) {
#define MLKEM_XW(W) if constexpr (W < RATE / 4) keccak_word<W>(s) ^= (w == W) ? v : 0u;
    MLKEM_XW(0) MLKEM_XW(1) MLKEM_XW(2) MLKEM_XW(3) MLKEM_XW(4) MLKEM_XW(5) MLKEM_XW(6) MLKEM_XW(7)
    MLKEM_XW(8) MLKEM_XW(9) MLKEM_XW(10) MLKEM_XW(11) MLKEM_XW(12) MLKEM_XW(13) MLKEM_XW(14) MLKEM_XW(15)
    MLKEM_XW(16) MLKEM_XW(17) MLKEM_XW(18) MLKEM_XW(19) MLKEM_XW(20) MLKEM_XW(21) MLKEM_XW(22) MLKEM_XW(23)
    MLKEM_XW(24) MLKEM_XW(25) MLKEM_XW(26) MLKEM_XW(27) MLKEM_XW(28) MLKEM_XW(29) MLKEM_XW(30) MLKEM_XW(31)
    MLKEM_XW(32) MLKEM_XW(33) MLKEM_XW(34) MLKEM_XW(35) MLKEM_XW(36) MLKEM_XW(37) MLKEM_XW(38) MLKEM_XW(39)
    MLKEM_XW(40) MLKEM_XW(41)
#undef MLKEM_XW
}

// ------------------------------------------------------------------------------------------------
// k_sha3_ragged — one message per lane.  Iteration t of the wave: the lanes whose message has a rate block t absorb it (the
// suffix byte at the lane's own total % RATE and 0x80 at RATE - 1 in the lane's own last block), every lane permutes, and the
// lanes that are squeezing store their next output block at once -- so the permutations the wave still runs for longer
// messages cannot touch an output that is complete.  The wave ends when its last lane has stored its last block.
// A lane streams its body with ONE load per absorbed qword: the upper qword of a funnel shift is the lower one of the next
// (`carry`), across block boundaries too; the head / body boundary is wave-uniform (head_len), so the carry starts there.
// Compiled for 4 waves per SIMD (128 VGPRs) like k_hash_batch: the per-lane message description lives next to the 50-register state.
// ------------------------------------------------------------------------------------------------
constexpr int SHA3R_GROUP = 8;   // qword loads a lane has in flight
template <int RATE>
__global__ void __launch_bounds__(WAVE, 4) k_sha3_ragged(Sha3rArgs a) {
    constexpr int NQ = RATE / 8;
    const size_t item = (size_t)blockIdx.x * WAVE + (size_t)lane_id();
    const bool live = item < a.n;
    Sha3rItem it;
    it.head = nullptr; it.bodyq = nullptr; it.shift = 0; it.len = 0; it.total = 0; it.bad = false;
    if (live) it = sha3r_item(a, item);
    const bool run = live && !it.bad;
    uint8_t* orow = a.out + (live ? item : 0) * a.out_stride;
    if (live && a.status) a.status[item] = it.bad ? SHA3R_ERR_ARG : 0;
    if (live && it.bad) sha3r_zero_row(orow, a.outlen, 0, 1);
    const unsigned nabs = run ? it.total / (unsigned)RATE + 1u : 0u;        // rate blocks this lane absorbs
    const unsigned nsq = (a.outlen + (unsigned)RATE - 1u) / (unsigned)RATE;  // ... and squeezes
    const unsigned nperm = run ? nabs + nsq - 1u : 0u;
    KeccakState s;
    keccak_zero(s);
    uint64_t carry = 0;
#pragma unroll 1
    for (unsigned t = 0; __ballot(t < nperm) != 0; t++) {
        if (t < nabs) {
            const unsigned base = t * (unsigned)RATE;
            // SHA3R_GROUP qwords at a time: first every load of the group (each under its own predicate, nothing waits in between),
            // then the funnel shifts and XORs -- one memory round trip per group, and at most 2 * SHA3R_GROUP staging registers
            // next to the 50-register state
#pragma unroll
            for (int w0 = 0; w0 < NQ; w0 += SHA3R_GROUP) {
                uint64_t raw[SHA3R_GROUP];
                if (base + 8u * (unsigned)w0 <= a.head_len && a.head_len < base + 8u * (unsigned)(w0 + SHA3R_GROUP < NQ ? w0 + SHA3R_GROUP : NQ) && it.len)
                    carry = sha3r_ld8(item, it.bodyq);            // the body starts in this group (wave-uniform position)
#pragma unroll
                for (int k = 0; k < SHA3R_GROUP; k++) {
                    const unsigned p = base + 8u * (unsigned)(w0 + k);   // message position of this qword: wave-uniform
                    raw[k] = 0;
                    // ONE load per qword, its address selected (wave-uniformly) between head and body: with a load on either side
                    // of a branch every head load waited for all loads before it
                    const bool in_head = p < a.head_len;
                    const uint8_t* src = in_head ? it.head + p : it.bodyq + (p - a.head_len) + 8u;
                    if (w0 + k < NQ && p < it.total && (in_head || sha3r_next_has_body(it, p - a.head_len))) raw[k] = sha3r_ld8(item, src);
                }
#pragma unroll
                for (int k = 0; k < SHA3R_GROUP; k++) {
                    if (w0 + k >= NQ) break;
                    const unsigned p = base + 8u * (unsigned)(w0 + k);
                    uint64_t v = raw[k];
                    if (p >= a.head_len) {                        // body: the upper qword of this funnel shift is the lower one of the next
                        v = sha3r_funnel(carry, raw[k], it.shift);
                        carry = raw[k];
                    }
                    v = sha3r_keep(v, it.total, p);
                    s.lo[w0 + k] ^= (uint32_t)v;
                    s.hi[w0 + k] ^= (uint32_t)(v >> 32);
                }
                pin_state<NQ>(s);
                sched_fence();
            }
            const bool last = t + 1u == nabs;
            const unsigned pos = it.total - base;             // the lane's own total % RATE in its last block
            sha3r_xor_word<RATE>(s, pos >> 2, last ? a.suffix << (8u * (pos & 3u)) : 0u);
            keccak_xor_byte<RATE - 1>(s, last ? 0x80u : 0u);
        }
        keccak_f1600(s);
        if (t + 1u >= nabs && t < nperm) {                    // squeezing: output block t + 1 - nabs
            const unsigned done = (t + 1u - nabs) * (unsigned)RATE;
            const unsigned take = a.outlen - done < (unsigned)RATE ? a.outlen - done : (unsigned)RATE;
            uint8_t* o = orow + done;
#ifndef MLKEM_EMU
            asm volatile("" : "+v"(o));   // the row's dword addresses are offsets of this one: otherwise RATE / 4 pointers are hoisted out of the loop
#endif
#define MLKEM_SQ(W)                                                                                          \
            if constexpr (W < RATE / 4) {                                                                    \
                if (4u * W + 4u <= take) *reinterpret_cast<uint32_t*>(o + 4 * W) = keccak_word<W>(s);        \
                else if (4u * W < take) {                                                                    \
                    const uint32_t v = keccak_word<W>(s);                                                    \
                    for (unsigned b = 0; 4u * W + b < take; b++) o[4 * W + b] = (uint8_t)(v >> (8 * b));     \
                }                                                                                            \
            }
            MLKEM_SQ(0) MLKEM_SQ(1) MLKEM_SQ(2) MLKEM_SQ(3) MLKEM_SQ(4) MLKEM_SQ(5) MLKEM_SQ(6) MLKEM_SQ(7)
            MLKEM_SQ(8) MLKEM_SQ(9) MLKEM_SQ(10) MLKEM_SQ(11) MLKEM_SQ(12) MLKEM_SQ(13) MLKEM_SQ(14) MLKEM_SQ(15)
            MLKEM_SQ(16) MLKEM_SQ(17) MLKEM_SQ(18) MLKEM_SQ(19) MLKEM_SQ(20) MLKEM_SQ(21) MLKEM_SQ(22) MLKEM_SQ(23)
            MLKEM_SQ(24) MLKEM_SQ(25) MLKEM_SQ(26) MLKEM_SQ(27) MLKEM_SQ(28) MLKEM_SQ(29) MLKEM_SQ(30) MLKEM_SQ(31)
            MLKEM_SQ(32) MLKEM_SQ(33) MLKEM_SQ(34) MLKEM_SQ(35) MLKEM_SQ(36) MLKEM_SQ(37) MLKEM_SQ(38) MLKEM_SQ(39)
            MLKEM_SQ(40) MLKEM_SQ(41)
#undef MLKEM_SQ
        }
    }
}

// ------------------------------------------------------------------------------------------------
// wk_absorb_bytes — wk_absorb's byte-granular sibling: one message of any length from an unaligned base.  Keccak lane i of rate
// block b takes message bytes [b * rate + 8 i, + 8): one aligned load when they lie in the head or the body is 8-byte aligned,
// two neighbouring ones funnel-shifted otherwise.  Like wk_absorb, the next block's loads are issued before the permutation they
// hide behind (after the XOR, outside any branch on the block number; the last iteration re-reads its own block).
// `rate` is a run-time value (a multiple of 8); the state is left after the last permutation.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wk_absorb_bytes(WkState& a, const WkLane& c, const Sha3rItem& it, size_t item, unsigned head_len,
                                                unsigned rate, uint32_t suffix) {
    const int i = wk_index();
    const unsigned nq = rate / 8u, mine = 8u * (unsigned)(i < 0 ? 0 : i);
    const bool carries = i >= 0 && (unsigned)i < nq;
    a.lo = 0; a.hi = 0;
    const unsigned nblocks = it.total / rate + 1u;
    // the loads of one block (the raw aligned qwords: nothing here waits for them) ...
    struct Raw { uint64_t lo, hi; };
    auto fetch = [&](unsigned blk) {
        const unsigned p = blk * rate + mine;
        const bool in_head = p < head_len, want = carries && p < it.total;
        const unsigned j = in_head ? 0u : p - head_len;
        const uint8_t* src = in_head ? it.head + p : it.bodyq + j;     // one load with a selected address, as in k_sha3_ragged
        Raw r;
        r.lo = 0; r.hi = 0;
        if (want) r.lo = sha3r_ld8(item, src);
        if (want && !in_head && it.shift && sha3r_next_has_body(it, j)) r.hi = sha3r_ld8(item, src + 8);
        return r;
    };
    // ... and the 8 message bytes they make, computed where they are absorbed: after the permutation the loads hid behind
    auto bytes_of = [&](unsigned blk, const Raw& r) {
        const unsigned p = blk * rate + mine;
        const uint64_t v = p < head_len ? r.lo : sha3r_funnel(r.lo, r.hi, it.shift);
        return sha3r_keep(v, it.total, p);
    };
    Raw r = fetch(0);
#pragma unroll 1
    for (unsigned blk = 0; blk < nblocks; blk++) {
        const uint64_t v = bytes_of(blk, r);
        a.lo ^= (uint32_t)v; a.hi ^= (uint32_t)(v >> 32);
        sched_fence();
        const bool last = blk + 1u == nblocks;
        r = fetch(last ? blk : blk + 1u);
        if (last) {                 // pad10*1: suffix byte at message position `total`, 0x80 at the block's last byte
            const unsigned pos = it.total - blk * rate;        // < rate
            if (carries && mine == (pos & ~7u)) {
                const uint32_t sv = suffix << (8u * (pos & 3u));
                if (pos & 4u) a.hi ^= sv; else a.lo ^= sv;
            }
            if (i == (int)nq - 1) a.hi ^= 0x80000000u;
        }
        wk_permute(a, c);
    }
}

// ------------------------------------------------------------------------------------------------
// k_sha3_ragged_w — one message per wave (blockIdx.x = item), arguments as k_sha3_ragged, any of the five rates at run time.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) k_sha3_ragged_w(Sha3rArgs a, unsigned rate) {
    const size_t item = blockIdx.x;
    if (item >= a.n) return;
    __shared__ uint2 rc_table[WK_RC_ENTRIES];
    const int i = wk_index();
    const bool prim = wk_primary();
    const Sha3rItem it = sha3r_item(a, item);
    uint8_t* orow = a.out + item * a.out_stride;
    if (lane_id() == 0 && a.status) a.status[item] = it.bad ? SHA3R_ERR_ARG : 0;
    if (it.bad) {
        sha3r_zero_row(orow, a.outlen, (unsigned)lane_id(), WAVE);
        return;
    }
    WkLane c;
    wk_lane_init(c, rc_table);
    WkState st;
    wk_absorb_bytes(st, c, it, item, a.head_len, rate, a.suffix);
    const unsigned mine = 8u * (unsigned)(i < 0 ? 0 : i);
    for (unsigned done = 0; done < a.outlen; done += rate) {
        if (done) wk_permute(st, c);
        const unsigned take = a.outlen - done < rate ? a.outlen - done : rate;
        if (prim && mine < take) {
            uint8_t* o = orow + done + mine;
            const unsigned left = take - mine;
            if (left >= 4u) *reinterpret_cast<uint32_t*>(o) = st.lo;
            else for (unsigned b = 0; b < left; b++) o[b] = (uint8_t)(st.lo >> (8u * b));
            if (left >= 8u) *reinterpret_cast<uint32_t*>(o + 4) = st.hi;
            else for (unsigned b = 4; b < left; b++) o[b] = (uint8_t)(st.hi >> (8u * (b - 4u)));
        }
    }
    // the wave's only LDS is the round-constant table, which never holds message bytes; it is cleared all the same, so that "this
    // kernel leaves its LDS zero" is a property the CPU tier can read back
    wave_lds_fence();
    if (lane_id() < WK_RC_ENTRIES) {
        uint2 z;
        z.x = 0; z.y = 0;
        rc_table[lane_id()] = z;
    }
#ifdef MLKEM_EMU_LDS_PROBE
    wave_lds_fence();
    if (lane_id() == 0) MLKEM_EMU_LDS_PROBE(rc_table, sizeof rc_table);
#endif
}

}   // namespace mlkem
