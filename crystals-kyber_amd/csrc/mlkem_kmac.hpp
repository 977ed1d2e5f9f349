// mlkem_kmac.hpp — SP 800-185 cSHAKE128 / 256, KMAC128 / 256 and KMACXOF128 / 256 over a device-resident batch of messages of
// UNEQUAL length (mlkem_cshake_dev, mlkem_kmac_dev), keyed by device rows used in place (the K an Encaps / Decaps call has written).
//
//   cSHAKE(X_i, L, N, S) = Keccak[c](bytepad(encode_string(N) || encode_string(S), rate) || X_i || 00, L)     (SHAKE when N = S = "")
//   KMAC(K_i, X_i, L, S) = cSHAKE(bytepad(encode_string(K_i), rate) || X_i || right_encode(L), L, "KMAC", S)   (XOF: right_encode(0))
//   X_i = lead (0..8 call-uniform bytes, e.g. the counter 00 00 00 01 of SP 800-56C) || head row i || body_i, head and body exactly
//   as in mlkem_sha3r.hpp.
//
// What a per-item kernel absorbs, as ONE byte stream whose positions are wave-uniform except its end:
//   [0, KB)              with a per-item key (key_stride > 0) the key block, KB = rate: a 4- or 5-byte header (01 rate, then
//                        01 xx for key_len < 32 or 02 hh ll), the key, zeros.  key_len <= 128, so it is one block at both rates.
//                        KB = 0 without a per-item key.
//   [KB, KB + PL)        lead || head, PL = lead_len + head_len: the head's aligned qwords funnel-shifted by lead_len bytes
//   [KB + PL, total)     the body: its aligned qwords funnel-shifted by (address - PL) & 7, the lane's own shift
//   [total, + tail_len)  right_encode(L) || 04 (KMAC), 04 (cSHAKE) or 1F (SHAKE): at most 5 bytes at the LANE'S OWN position, which
//                        may straddle a rate block boundary: every absorbed qword takes its share of one 64-bit constant shifted by
//                        the lane's distance to `total` (kmac_tail_at).  nabs = (total + tail_len - 1) / rate + 1 blocks, 0x80 at
//                        rate - 1 of the last.
// Everything in front of that stream is call-uniform and is absorbed ONCE per call by k_kmac_prefix (one wavefront on wk_permute):
// bytepad(encode_string(N) || encode_string(S), rate), built on the host and passed by value, and for a SHARED key (key_stride = 0:
// any length 0..512, any address) bytepad(encode_string(K), rate), whose bytes the kernel reads from device memory.  It leaves the
// 200-byte Keccak state (the "midstate") in a region owned by the context and the per-item kernels start from it instead of zero:
// a KMAC with a per-item key over a short message is 2 permutations per item instead of 3.
//
// The midstate region is allocated WITH THE CONTEXT (mlkem_ctx_create; 256 bytes), never lazily: every call is a pure function of
// its inputs and may be captured into a graph from the first one on.  With a shared key the midstate is key-equivalent, so the call
// zeroes the region in stream order after its last kernel (as rng_zero does for derived seeds).  Like the context's scratch, the
// region serves one call at a time: calls of one context are made on one stream (or ordered by the caller).
//
// The rules of mlkem_sha3r.hpp hold: every message or key load is a naturally aligned 8-byte load (sha3r_ld8) holding at least one
// byte of the item's own key, head or body (of the shared key in k_kmac_prefix); no message or key byte goes to LDS; control flow and
// addresses depend on lengths and offsets only; a squeezing lane stores each output block at once.
#pragma once
#include "mlkem_sha3r.hpp"
#include <string.h>

namespace mlkem {

constexpr size_t KMAC_ITEM_NONE = ~(size_t)0;   // `item` of the shared key's loads in the CPU tier's load probe
constexpr unsigned KMAC_MID_BYTES = 256;        // the context's midstate region (200 used)
constexpr unsigned KMAC_PREFIX_WORDS = 63;      // bytepad(encode_string(N) || encode_string(S)): at most 3 blocks of 168 bytes

// ---- SP 800-185 encodings (host) -------------------------------------------------------------------------------------------
// left_encode / right_encode of x < 2^32 into o (at most 5 bytes); returns the length
inline unsigned kmac_left_encode(uint64_t x, uint8_t* o) {
    unsigned nb = 1;
    while (nb < 8 && (x >> (8 * nb))) nb++;
    o[0] = (uint8_t)nb;
    for (unsigned b = 0; b < nb; b++) o[1 + b] = (uint8_t)(x >> (8 * (nb - 1 - b)));
    return nb + 1;
}
inline unsigned kmac_right_encode(uint64_t x, uint8_t* o) {
    unsigned nb = 1;
    while (nb < 8 && (x >> (8 * nb))) nb++;
    for (unsigned b = 0; b < nb; b++) o[b] = (uint8_t)(x >> (8 * (nb - 1 - b)));
    o[nb] = (uint8_t)nb;
    return nb + 1;
}
inline uint64_t kmac_le64(const uint8_t* b, unsigned nbytes) {
    uint64_t v = 0;
    for (unsigned i = 0; i < nbytes && i < 8; i++) v |= (uint64_t)b[i] << (8 * i);
    return v;
}

// one call as the C-ABI takes it (include/mlkem_batch.h); `s` carries n, head, body, out and status
struct KmacCall {
    int bits;                                           // 128 | 256
    bool kmac, xof;                                     // KMAC (N = "KMAC", key block, right_encode) / its XOF variant; else cSHAKE
    const uint8_t* fname; unsigned fname_len;           // N (cSHAKE only), host bytes, <= 32
    const uint8_t* custom; unsigned custom_len;         // S, host bytes, <= 256
    const uint8_t* lead; unsigned lead_len;             // host bytes, <= 8
    const uint8_t* key; unsigned key_len; size_t key_stride;   // KMAC: device key rows (stride > 0) or one shared key (stride 0)
    Sha3rArgs s;
};

// The argument rules of mlkem_cshake[_dev] / mlkem_kmac[_dev], shared by the C-ABI and the CPU tier.  dev = false: the arrays are
// host arrays that will be staged, so the rules about device addresses (alignment of head, key, offsets, out) do not apply.
inline bool kmac_check_args(KmacCall& c, bool dev, unsigned& rate) {
    Sha3rArgs& a = c.s;
    if (c.bits != 128 && c.bits != 256) return false;
    rate = c.bits == 128 ? 168u : 136u;
    if (a.outlen < 1 || a.outlen > 65536) return false;
    if (c.fname_len > 32 || c.custom_len > 256 || c.lead_len > 8) return false;
    if ((c.fname_len && !c.fname) || (c.custom_len && !c.custom) || (c.lead_len && !c.lead)) return false;
    if (c.kmac) {
        if (c.key_stride) {
            if (c.key_len % 8 || c.key_len < 8 || c.key_len > 128 || c.key_stride < c.key_len) return false;
            if (dev && c.key_stride % 8) return false;
        } else if (c.key_len > 512) {
            return false;
        }
    }
    if (a.n == 0) return true;
    if (c.kmac && c.key_len && !c.key) return false;
    if (c.kmac && c.key_stride && dev && (reinterpret_cast<uintptr_t>(c.key) & 7u)) return false;
    if (!a.head) a.head_len = 0;
    if (!a.out || !a.body_off || !a.body_len || (!a.body && a.body_bytes)) return false;
    if (a.head_len % 8 || a.head_len >= (1u << 31) || (a.head_len && a.head_stride < a.head_len) || a.out_stride < a.outlen) return false;
    if (!dev) return true;
    if (a.head_len && ((reinterpret_cast<uintptr_t>(a.head) & 7u) || a.head_stride % 8)) return false;
    if ((reinterpret_cast<uintptr_t>(a.body_off) & 7u) || (reinterpret_cast<uintptr_t>(a.body_len) & 3u)) return false;
    if ((reinterpret_cast<uintptr_t>(a.out) & 15u) || a.out_stride % 4) return false;
    if (a.status && (reinterpret_cast<uintptr_t>(a.status) & 3u)) return false;
    return true;
}

// the call-uniform prefix blocks built on the host: bytepad(encode_string(N) || encode_string(S), rate) as little-endian qwords
struct KmacPrefix {
    uint64_t w[KMAC_PREFIX_WORDS];
    unsigned nblocks;
};
inline void kmac_build_prefix(KmacPrefix& p, unsigned rate, const uint8_t* N, unsigned nlen, const uint8_t* S, unsigned slen) {
    uint8_t buf[8 * KMAC_PREFIX_WORDS];
    memset(buf, 0, sizeof buf);
    unsigned pos = kmac_left_encode(rate, buf);
    pos += kmac_left_encode(8ull * nlen, buf + pos);
    if (nlen) memcpy(buf + pos, N, nlen);
    pos += nlen;
    pos += kmac_left_encode(8ull * slen, buf + pos);
    if (slen) memcpy(buf + pos, S, slen);
    pos += slen;                                        // <= 2 + 35 + 259 = 296: three blocks of 136, two of 168
    p.nblocks = (pos + rate - 1) / rate;
    for (unsigned i = 0; i < KMAC_PREFIX_WORDS; i++) p.w[i] = kmac_le64(buf + 8 * i, 8);
}
// the header of a key block: left_encode(rate) || left_encode(8 * key_len), 4 bytes for key_len < 32 and 5 up to 512 (-> hdr_len)
inline uint64_t kmac_key_header(unsigned rate, unsigned key_len, unsigned& hdr_len) {
    uint8_t b[16];
    unsigned pos = kmac_left_encode(rate, b);
    pos += kmac_left_encode(8ull * key_len, b + pos);
    hdr_len = pos;
    return kmac_le64(b, pos);
}

// what the per-item kernels take
struct KmacArgs {
    Sha3rArgs s;                          // n, head, body, out, status as in k_sha3_ragged (s.suffix unused: the tail carries it)
    const uint8_t* key;                   // per-item key rows (key_stride > 0), 8-byte aligned
    unsigned key_len; size_t key_stride;  // key_stride = 0: no key block in the per-item stream
    uint64_t khdr; unsigned khdr_len;     // the key block's header bytes (low khdr_len bytes), 4 or 5
    uint64_t lead; unsigned lead_len;     // the lead bytes (low lead_len bytes)
    uint64_t tail; unsigned tail_len;     // right_encode(L) || 04, 04 or 1F (low tail_len bytes), 1..5
    const uint64_t* mid;                  // the midstate k_kmac_prefix left (25 qwords), or null: start from zero (plain SHAKE)
};

// the share of the tail constant in the qword at stream position p of a message that ends at `total`
__device__ __forceinline__ uint64_t kmac_tail_at(uint64_t tail, unsigned total, unsigned p) {
    const int d = (int)(total - p);       // bytes from this qword's first byte to the tail's first (either sign)
    if (d >= 8 || d <= -8) return 0;
    return d >= 0 ? tail << (8u * (unsigned)d) : tail >> (8u * (unsigned)(-d));
}

// one item as both kernels see it: sha3r_item plus the positions that depend on the lead and the key block
struct KmacItem {
    Sha3rItem it;          // it.bodyq moved back 8 bytes when the body's shift is smaller than the call's (boff)
    unsigned total;        // key block + lead + head + body
    unsigned es;           // bits the body's stream sits above the start of its first stream qword: 8 * ((address - PL) & 7)
    unsigned boff;         // 0, or (unsigned)-8: the stream's first body qword begins 8 bytes before it.bodyq's (nothing is loaded there)
};
__device__ __forceinline__ KmacItem kmac_item(const KmacArgs& a, size_t item, unsigned kb) {
    KmacItem k;
    k.it = sha3r_item(a.s, item);
    const unsigned pl = a.lead_len + a.s.head_len, m8 = 8u * (pl & 7u);
    k.it.bad = k.it.bad || (uint64_t)pl + k.it.len >= (1ull << 31);
    if (k.it.bad) k.it.len = 0;
    k.total = k.it.bad ? 0u : kb + pl + k.it.len;
    k.es = (k.it.shift - m8) & 63u;
    k.boff = k.it.shift >= m8 ? 0u : ~7u;
    k.it.bodyq += (int)k.boff;
    return k;
}
// does the aligned qword at byte j (a multiple of 8, relative to the stream's first body qword) hold a byte of the body?
__device__ __forceinline__ bool kmac_has_body(const KmacItem& k, unsigned j) { return k.it.len && sha3r_next_has_body(k.it, j + k.boff - 8u); }

// store `take` bytes (<= RATE) of the state at o (4-byte aligned): the squeeze of the lane-sliced form
template <int RATE>
__device__ __forceinline__ void kmac_store_block(KeccakState& s, uint8_t* o, unsigned take) {
#ifndef MLKEM_EMU
    asm volatile("" : "+v"(o));   // the row's dword addresses are offsets of this one (as in k_sha3_ragged)
#endif
#define MLKEM_SQ(W)                                                                                          \
    if constexpr (W < RATE / 4) {                                                                            \
        if (4u * W + 4u <= take) *reinterpret_cast<uint32_t*>(o + 4 * W) = keccak_word<W>(s);                \
        else if (4u * W < take) {                                                                            \
            const uint32_t v = keccak_word<W>(s);                                                            \
            for (unsigned b = 0; 4u * W + b < take; b++) o[4 * W + b] = (uint8_t)(v >> (8 * b));             \
        }                                                                                                    \
    }
    MLKEM_SQ(0) MLKEM_SQ(1) MLKEM_SQ(2) MLKEM_SQ(3) MLKEM_SQ(4) MLKEM_SQ(5) MLKEM_SQ(6) MLKEM_SQ(7)
    MLKEM_SQ(8) MLKEM_SQ(9) MLKEM_SQ(10) MLKEM_SQ(11) MLKEM_SQ(12) MLKEM_SQ(13) MLKEM_SQ(14) MLKEM_SQ(15)
    MLKEM_SQ(16) MLKEM_SQ(17) MLKEM_SQ(18) MLKEM_SQ(19) MLKEM_SQ(20) MLKEM_SQ(21) MLKEM_SQ(22) MLKEM_SQ(23)
    MLKEM_SQ(24) MLKEM_SQ(25) MLKEM_SQ(26) MLKEM_SQ(27) MLKEM_SQ(28) MLKEM_SQ(29) MLKEM_SQ(30) MLKEM_SQ(31)
    MLKEM_SQ(32) MLKEM_SQ(33) MLKEM_SQ(34) MLKEM_SQ(35) MLKEM_SQ(36) MLKEM_SQ(37) MLKEM_SQ(38) MLKEM_SQ(39)
    MLKEM_SQ(40) MLKEM_SQ(41)
#undef MLKEM_SQ
}

// ------------------------------------------------------------------------------------------------
// k_kmac_prefix — one wavefront: absorbs the call-uniform prefix and leaves the Keccak state in `mid` (25 qwords).
// `pre`: the host-built blocks of bytepad(encode_string(N) || encode_string(S), rate).  has_key: then the blocks of
// bytepad(encode_string(K), rate) for the shared key at `key` (any address, key_len 0..512): header khdr, the key read by aligned
// 8-byte loads of the qwords that hold it, zeros up to the block's end.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) k_kmac_prefix(KmacPrefix pre, unsigned rate, const uint8_t* key, unsigned key_len, int has_key,
                                                      uint64_t khdr, unsigned khdr_len, uint64_t* mid) {
    __shared__ uint2 rc_table[WK_RC_ENTRIES];
    const int i = wk_index();
    const unsigned nq = rate / 8u, li = (unsigned)(i < 0 ? 0 : i);
    const bool carries = i >= 0 && li < nq;
    WkLane c;
    wk_lane_init(c, rc_table);
    WkState st;
    st.lo = 0; st.hi = 0;
#pragma unroll 1
    for (unsigned blk = 0; blk < pre.nblocks; blk++) {
        const unsigned w = blk * nq + li;
        const uint64_t v = carries && w < KMAC_PREFIX_WORDS ? pre.w[w] : 0ull;
        st.lo ^= (uint32_t)v; st.hi ^= (uint32_t)(v >> 32);
        wk_permute(st, c);
    }
    if (has_key) {
        const unsigned nkb = (khdr_len + key_len + rate - 1u) / rate;
        const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(key) & 7u);
        const uint8_t* keyq = key - mis;                     // the aligned qword that holds the key's first byte
#pragma unroll 1
        for (unsigned blk = 0; blk < nkb; blk++) {
            // stream bytes [p, p + 8) = key bytes [p - khdr_len, + 8): raw bytes [r, r + 8) above keyq, r = mis + p - khdr_len
            const unsigned p = blk * rate + 8u * li;
            const int r = (int)(mis + p) - (int)khdr_len;    // >= -5
            const int q0 = r >= 0 ? (r & ~7) : -8;           // the aligned qword holding raw byte r (r < 0: the one before keyq)
            const unsigned sh = 8u * (unsigned)(r - q0);
            const int end = (int)(mis + key_len);            // raw bytes [mis, end) are the key
            uint64_t lo = 0, hi = 0;
            const bool want = carries && p < khdr_len + key_len;
            if (want && q0 >= 0 && q0 < end) lo = sha3r_ld8(KMAC_ITEM_NONE, keyq + q0);
            if (want && sh && q0 + 8 < end) hi = sha3r_ld8(KMAC_ITEM_NONE, keyq + q0 + 8);
            uint64_t v = sha3r_funnel(lo, hi, sh);
            // keep the bytes that are key bytes: stream byte p + b is key byte p + b - khdr_len
            const int first = (int)khdr_len - (int)p;        // bytes below this are header (only in the stream's first qword)
            if (first > 0) v &= ~0ull << (8u * (unsigned)first);
            v = sha3r_keep(v, khdr_len + key_len, p);
            if (p == 0) v |= khdr;
            if (!carries) v = 0;
            st.lo ^= (uint32_t)v; st.hi ^= (uint32_t)(v >> 32);
            wk_permute(st, c);
        }
    }
    if (wk_primary()) {
        uint2 o;
        o.x = st.lo; o.y = st.hi;
        reinterpret_cast<uint2*>(mid)[i] = o;
    }
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

// ------------------------------------------------------------------------------------------------
// k_kmac_ragged — one message per lane, the loop of k_sha3_ragged over the stream described above.  Iteration t: the lanes whose
// stream has a rate block t absorb it, every lane permutes, the squeezing lanes store their next output block at once.
// With a per-item key, block 0 is the key block of every running lane (wave-uniform): header and key through a funnel shift by the
// header's length, one load per key qword.  In the blocks after it one load per absorbed qword: the head's (the upper qword of
// the lead funnel; the lower one is the previous load, re-read once per group of KMAC_GROUP) or the body's (`carry`, as in
// k_sha3_ragged).  The one qword that holds the head's last and the body's first bytes (lead_len % 8 != 0) takes both shares.
// Compiled for 4 waves per SIMD (128 VGPRs); no LDS.
// ------------------------------------------------------------------------------------------------
constexpr int KMAC_GROUP = 4;   // qword loads a lane has in flight: half of SHA3R_GROUP, the lead funnel and the tail cost the registers of the other half
template <int RATE>
__global__ void __launch_bounds__(WAVE, 4) k_kmac_ragged(KmacArgs a) {
    constexpr int NQ = RATE / 8;
    const size_t item = (size_t)blockIdx.x * WAVE + (size_t)lane_id();
    const bool live = item < a.s.n;
    const unsigned kb = a.key_stride ? (unsigned)RATE : 0u;           // the key block
    const unsigned pl = a.lead_len + a.s.head_len;                    // lead || head
    const unsigned m = pl & 7u, xb0 = pl - m;                         // X position of the first qword holding a body byte
    const unsigned nph = (pl + 7u) / 8u, hq = a.s.head_len / 8u;      // X qwords holding lead / head bytes; head qwords
    const unsigned hs = 8u * ((8u - a.lead_len) & 7u);                // the lead funnel (lead_len 1..8)
    KmacItem k;
    k.it.head = nullptr; k.it.bodyq = nullptr; k.it.shift = 0; k.it.len = 0; k.it.total = 0; k.it.bad = false;
    k.total = 0; k.es = 0; k.boff = 0;
    if (live) k = kmac_item(a, item, kb);
    const bool run = live && !k.it.bad;
    uint8_t* orow = a.s.out + (live ? item : 0) * a.s.out_stride;
    if (live && a.s.status) a.s.status[item] = k.it.bad ? SHA3R_ERR_ARG : 0;
    if (live && k.it.bad) sha3r_zero_row(orow, a.s.outlen, 0, 1);
    const unsigned nabs = run ? (k.total + a.tail_len - 1u) / (unsigned)RATE + 1u : 0u;
    const unsigned nsq = (a.s.outlen + (unsigned)RATE - 1u) / (unsigned)RATE;
    const unsigned nperm = run ? nabs + nsq - 1u : 0u;
    KeccakState s;
    if (a.mid) {
#pragma unroll
        for (int w = 0; w < 25; w++) {
            const uint64_t v = a.mid[w];                              // wave-uniform
            s.lo[w] = (uint32_t)v; s.hi[w] = (uint32_t)(v >> 32);
        }
    } else {
        keccak_zero(s);
    }
    uint64_t carry = 0;
#pragma unroll 1
    for (unsigned t = 0; __ballot(t < nperm) != 0; t++) {
        if (t < nabs && kb && t == 0) {
            // the key block: stream qword q = funnel(K[q - 1], K[q]) with the header in front of K[0]
            const unsigned nkq = a.key_len / 8u, ks = 8u * (8u - a.khdr_len);
            const uint8_t* krow = a.key + item * a.key_stride;
            uint64_t prev = a.khdr << ks;
#pragma unroll
            for (int w0 = 0; w0 < 24; w0 += KMAC_GROUP) {           // key_len <= 128: qwords 0..16
                uint64_t raw[KMAC_GROUP];
#pragma unroll
                for (int q = 0; q < KMAC_GROUP; q++) {
                    raw[q] = 0;
                    if (w0 + q < NQ && (unsigned)(w0 + q) < nkq) raw[q] = sha3r_ld8(item, krow + 8 * (w0 + q));
                }
#pragma unroll
                for (int q = 0; q < KMAC_GROUP; q++) {
                    if (w0 + q >= NQ) break;
                    const uint64_t v = (unsigned)(w0 + q) <= nkq ? sha3r_funnel(prev, raw[q], ks) : 0ull;
                    prev = raw[q];
                    s.lo[w0 + q] ^= (uint32_t)v;
                    s.hi[w0 + q] ^= (uint32_t)(v >> 32);
                }
                pin_state<NQ>(s);
                sched_fence();
            }
        } else if (t < nabs) {
            const unsigned base = t * (unsigned)RATE;                 // stream position; X position = base - kb
#pragma unroll
            for (int w0 = 0; w0 < NQ; w0 += KMAC_GROUP) {
                uint64_t raw[KMAC_GROUP];
                const unsigned x0 = base - kb + 8u * (unsigned)w0;                          // wave-uniform
                const unsigned x1 = base - kb + 8u * (unsigned)(w0 + KMAC_GROUP < NQ ? w0 + KMAC_GROUP : NQ);
                if (x0 <= xb0 && xb0 < x1 && k.it.len && k.boff == 0u) carry = sha3r_ld8(item, k.it.bodyq);   // the body starts in this group
                uint64_t hprev = 0;                                   // lower qword of the lead funnel at the group's first qword
                if (a.lead_len && x0 < 8u * nph) {
                    if (x0 == 0u) hprev = a.lead << hs;
                    else if (x0 / 8u - 1u < hq) hprev = sha3r_ld8(item, k.it.head + (x0 - 8u));
                }
#pragma unroll
                for (int q = 0; q < KMAC_GROUP; q++) {
                    const unsigned x = x0 + 8u * (unsigned)q, p = x + kb;
                    raw[q] = 0;
                    const bool in_head = x / 8u < hq;
                    const uint8_t* src = in_head ? k.it.head + x : k.it.bodyq + (x - xb0) + 8u;
                    if (w0 + q < NQ && p < k.total && (in_head || (x >= xb0 && kmac_has_body(k, x - xb0 + 8u)))) raw[q] = sha3r_ld8(item, src);
                }
#pragma unroll
                for (int q = 0; q < KMAC_GROUP; q++) {
                    if (w0 + q >= NQ) break;
                    const unsigned x = x0 + 8u * (unsigned)q, p = x + kb;
                    const bool in_head = x / 8u < hq;
                    uint64_t v = 0;
                    if (x < 8u * nph) {                               // lead / head share
                        const uint64_t h = in_head ? raw[q] : 0ull;
                        v = a.lead_len ? sha3r_funnel(hprev, h, hs) : h;
                        hprev = h;
                    }
                    if (x >= xb0) {                                   // body share
                        uint64_t bv = sha3r_funnel(carry, raw[q], k.es);
                        carry = raw[q];
                        if (x == xb0 && m) bv &= ~0ull << (8u * m);   // bytes in front of the body's first
                        v ^= bv;
                    }
                    v = sha3r_keep(v, k.total, p) ^ kmac_tail_at(a.tail, k.total, p);
                    s.lo[w0 + q] ^= (uint32_t)v;
                    s.hi[w0 + q] ^= (uint32_t)(v >> 32);
                }
                pin_state<NQ>(s);
                sched_fence();
            }
            keccak_xor_byte<RATE - 1>(s, t + 1u == nabs ? 0x80u : 0u);
        }
        keccak_f1600(s);
        if (t + 1u >= nabs && t < nperm) {                            // squeezing: output block t + 1 - nabs
            const unsigned done = (t + 1u - nabs) * (unsigned)RATE;
            const unsigned take = a.s.outlen - done < (unsigned)RATE ? a.s.outlen - done : (unsigned)RATE;
            kmac_store_block<RATE>(s, orow + done, take);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_kmac_ragged_w — one message per wave (blockIdx.x = item) on wk_permute, either rate at run time.  Keccak lane i of block b takes
// the stream's bytes [b * rate + 8 i, + 8): at most three aligned loads (the head's last qword and two of the body where they
// meet), issued one block ahead of the permutation they hide behind, as in wk_absorb_bytes.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) k_kmac_ragged_w(KmacArgs a, unsigned rate) {
    const size_t item = blockIdx.x;
    if (item >= a.s.n) return;
    __shared__ uint2 rc_table[WK_RC_ENTRIES];
    const int i = wk_index();
    const bool prim = wk_primary();
    const unsigned kb = a.key_stride ? rate : 0u;
    const KmacItem k = kmac_item(a, item, kb);
    uint8_t* orow = a.s.out + item * a.s.out_stride;
    if (lane_id() == 0 && a.s.status) a.s.status[item] = k.it.bad ? SHA3R_ERR_ARG : 0;
    if (k.it.bad) {
        sha3r_zero_row(orow, a.s.outlen, (unsigned)lane_id(), WAVE);
        return;
    }
    WkLane c;
    wk_lane_init(c, rc_table);
    const unsigned nq = rate / 8u, mine = 8u * (unsigned)(i < 0 ? 0 : i);
    const bool carries = i >= 0 && (unsigned)i < nq;
    const unsigned pl = a.lead_len + a.s.head_len, m = pl & 7u, xb0 = pl - m;
    const unsigned nph = (pl + 7u) / 8u, hq = a.s.head_len / 8u, hs = 8u * ((8u - a.lead_len) & 7u);
    const unsigned nkq = a.key_len / 8u, ks = 8u * (8u - a.khdr_len);
    const uint8_t* krow = a.key + item * a.key_stride;
    const uint8_t* bq = k.it.bodyq;
    WkState st;
    st.lo = 0; st.hi = 0;
    if (a.mid && i >= 0) {                                            // copies load what their primaries load
        const uint64_t v = a.mid[i];
        st.lo = (uint32_t)v; st.hi = (uint32_t)(v >> 32);
    }
    const unsigned nblocks = (k.total + a.tail_len - 1u) / rate + 1u;
    struct Raw { uint64_t a, b, c; };     // key: K[q - 1], K[q] ; lead / head: lower and upper qword (a, b) ; body: lower and upper (b, c)
    auto fetch = [&](unsigned blk) {
        const unsigned p = blk * rate + mine;
        Raw r;
        r.a = 0; r.b = 0; r.c = 0;
        if (!carries || p >= k.total) return r;
        if (p < kb) {
            const unsigned q = mine / 8u;
            if (q == 0u) r.a = a.khdr << ks;
            else if (q - 1u < nkq) r.a = sha3r_ld8(item, krow + 8u * (q - 1u));
            if (q < nkq) r.b = sha3r_ld8(item, krow + 8u * q);
            return r;
        }
        const unsigned x = p - kb;
        const bool ph = x < 8u * nph, bd = x >= xb0;
        if (ph && !a.lead_len) {
            r.a = sha3r_ld8(item, k.it.head + x);
        } else if (ph) {
            if (x == 0u) r.a = a.lead << hs;
            else if (x / 8u - 1u < hq) r.a = sha3r_ld8(item, k.it.head + (x - 8u));
            if (!bd && x / 8u < hq) r.b = sha3r_ld8(item, k.it.head + x);
        }
        if (bd) {
            const unsigned j = x - xb0;
            if (kmac_has_body(k, j)) r.b = sha3r_ld8(item, bq + j);
            if (k.es && kmac_has_body(k, j + 8u)) r.c = sha3r_ld8(item, bq + j + 8u);
        }
        return r;
    };
    auto bytes_of = [&](unsigned blk, const Raw& r) {
        const unsigned p = blk * rate + mine;
        if (!carries) return (uint64_t)0;
        uint64_t v = 0;
        if (p < kb) {
            v = mine / 8u <= nkq ? sha3r_funnel(r.a, r.b, ks) : 0ull;
        } else {
            const unsigned x = p - kb;
            const bool ph = x < 8u * nph, bd = x >= xb0;
            if (ph) v = a.lead_len ? sha3r_funnel(r.a, bd ? 0ull : r.b, hs) : r.a;
            if (bd) {
                uint64_t bv = sha3r_funnel(r.b, r.c, k.es);
                if (x == xb0 && m) bv &= ~0ull << (8u * m);
                v ^= bv;
            }
        }
        return sha3r_keep(v, k.total, p) ^ kmac_tail_at(a.tail, k.total, p);
    };
    Raw r = fetch(0);
#pragma unroll 1
    for (unsigned blk = 0; blk < nblocks; blk++) {
        const uint64_t v = bytes_of(blk, r);
        st.lo ^= (uint32_t)v; st.hi ^= (uint32_t)(v >> 32);
        sched_fence();
        const bool last = blk + 1u == nblocks;
        r = fetch(last ? blk : blk + 1u);
        if (last && i == (int)nq - 1) st.hi ^= 0x80000000u;
        wk_permute(st, c);
    }
    for (unsigned done = 0; done < a.s.outlen; done += rate) {
        if (done) wk_permute(st, c);
        const unsigned take = a.s.outlen - done < rate ? a.s.outlen - done : rate;
        if (prim && mine < take) {
            uint8_t* o = orow + done + mine;
            const unsigned left = take - mine;
            if (left >= 4u) *reinterpret_cast<uint32_t*>(o) = st.lo;
            else for (unsigned b = 0; b < left; b++) o[b] = (uint8_t)(st.lo >> (8u * b));
            if (left >= 8u) *reinterpret_cast<uint32_t*>(o + 4) = st.hi;
            else for (unsigned b = 4; b < left; b++) o[b] = (uint8_t)(st.hi >> (8u * (b - 4u)));
        }
    }
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
