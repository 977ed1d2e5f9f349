// mlkem_keyset.hpp — prepared key sets (mlkem_keyset_create / mlkem_encaps_keyset_dev / mlkem_decaps_keyset_dev).
//
// A key set holds, per key, the bytes of ek or dk, h = H(ek) and A-hat^T (k x k polynomials, uint16, the layout the sampler writes
// with transpose = 1).  The FIPS 203 §7.2 / §7.3 input checks run once, at import; later calls name each item's key by index and
// run none of the key's work again: per ML-KEM-768 item 8 of Encaps' 44 Keccak-f remain (G + 7 PRF rows) and 15 of Decaps' 51
// (G + J + 7 PRF rows; in the batch form J runs for rejected ciphertexts only: 8 for an accepted one).
//
// Import (keyset_import_run): the check kernel of mlkem_check_keys_dev on the set's own copy of the keys, k_hash_batch<0> for the
// H table, the sampler (n_xof = keys of a chunk, transpose = 1) writing straight into the set's A-hat^T table; the status words
// are ORed into one word on the device so that the caller synchronises once.  Seed imports run KeyGen into the set's dk table
// first (keyset_seed_run).
// Calls:
//   small calls (KeysetLimits)     k_encaps_keyset_small / k_decaps_keyset_small: one launch, one workgroup per item (as the
//                                  kernels of mlkem_small.hpp, minus H(ek), the hash check and the k^2 SampleNTT jobs)
//   larger                         the batch pipeline with indexed kernels: k_hash_g_keyset, the PRF rows of the sampler,
//                                  k_encrypt2_keyset; k_decrypt4_keyset, k_hash_decaps_keyset (G alone), the compare in CMP_DEFER
//                                  mode and k_hash_j_rejected (J(z || c) of the rejected items, z read from the set by index); then
//                                  k_keyset_fix writes the status words and zeroes the outputs of items whose index is out of range
// Every gathering kernel bounds-checks its index (keyset_key): an index >= n_keys reads key 0, never outside the set.
#pragma once
#include "mlkem_pipeline.hpp"

namespace mlkem {

constexpr int32_t KS_ERR_ARG = -101;   // MLKEM_ERR_ARG (include/mlkem_batch.h): per-item status of an index >= n_keys

// The device tables of a key set (all rows of one parameter set).  keys + ek_off is the ek of key 0 (ek_off = 384 k inside dk rows).
struct KeysetView {
    const uint8_t* keys = nullptr;   // n_keys rows of key_stride bytes: ek (ek import) or dk (dk / seed import)
    size_t key_stride = 0;
    size_t ek_off = 0;
    const uint8_t* h = nullptr;      // n_keys x 32: H(ek)
    const uint16_t* At = nullptr;    // n_keys x k^2 x 256: A-hat^T
    size_t n_keys = 0;
    bool has_dk = false;
};

// Calls of at most enc_max_k[k - 2] (Encaps) / dec_max_k[k - 2] (Decaps) items run one workgroup per item; of those, calls of at
// most enc_lat_k / dec_lat_k items use eight waves per item, larger ones four.  The values are where the forms cross in the sweep of
// tools/keyset_sweep.py on one MI355X (sizes 1 .. 4096; LABNOTES "Prepared key sets"): Decaps keeps the small kernels about twice
// as far as Encaps because its batch path ran J lane-sliced for every item when they were swept (7-9 chained permutations at
// 8.8 us; it now defers J to the rejected items, and the Decaps limits have not been swept again).  Env MLKEM_KEYSET_SMALL_ITEMS /
// MLKEM_KEYSET_LATENCY_ITEMS set all of them.
struct KeysetLimits {
    size_t enc_max_k[3] = {1536, 1024, 768}, dec_max_k[3] = {3072, 2048, 3072};
    size_t enc_lat_k[3] = {256, 512, 256}, dec_lat_k[3] = {384, 256, 256};
    size_t enc_max(int k) const { return enc_max_k[k - 2]; }
    size_t dec_max(int k) const { return dec_max_k[k - 2]; }
    size_t enc_lat(int k) const { return enc_lat_k[k - 2]; }
    size_t dec_lat(int k) const { return dec_lat_k[k - 2]; }
    void set_all(size_t max_items, size_t lat_items) {
        for (int i = 0; i < 3; i++) {
            if (max_items != (size_t)-1) enc_max_k[i] = dec_max_k[i] = max_items;
            if (lat_items != (size_t)-1) enc_lat_k[i] = dec_lat_k[i] = lat_items;
        }
    }
};

// keyset_key (the item's key, bounds-checked) lives in mlkem_kernels.hpp: k_hash_j_rejected resolves z rows with it

// ------------------------------------------------------------------------------------------------
// Batch path
// ------------------------------------------------------------------------------------------------
// (K, r) = G(m || h[key]) per item (ml_kem.c:1113-1124), k_hash_g_shared with the item's own row of the H table
__global__ void __launch_bounds__(WAVE, MLKEM_KECCAK_MINWAVES) k_hash_g_keyset(size_t n, const uint32_t* __restrict__ idx, size_t n_keys,
                                                                               const uint8_t* __restrict__ m, const uint8_t* __restrict__ hs,
                                                                               uint8_t* __restrict__ Kout, uint8_t* __restrict__ r_ws) {
    const size_t item = (size_t)blockIdx.x * WAVE + lane_id();
    const size_t it = item < n ? item : n - 1;
    uint32_t mm[8], hh[8], w[8];
    load32(m, 32, it, mm);
    load32(hs, 32, keyset_key(idx, n_keys, it), hh);
    KeccakState s;
    lane_G64(s, mm, hh);
    if (item < n) {
        MLKEM_STATE_WORDS8(s, 0, w)
        store32(Kout, 32, item, w);
        MLKEM_STATE_WORDS8(s, 8, w)
        store32(r_ws, 32, item, w);
    }
}

// Decaps_internal's G (ml_kem.c:1187-1196) with the key's h: (K', r') = G(m' || h[key]).  J(z || c) is deferred to the rejected items
// (k_hash_j_rejected reads z from the set by index): no z row is gathered into scratch any more.  zero_ws: the item's 32-byte row of
// the scratch region that earlier versions gathered z into (ws.rho); it is still written to zero, so that "no key material is left in
// the context scratch after a key-set Decaps" stays a property the CPU tier reads back from that region.
__global__ void __launch_bounds__(WAVE, MLKEM_KECCAK_MINWAVES) k_hash_decaps_keyset(size_t n, const uint32_t* __restrict__ idx, size_t n_keys,
                                                                                    const uint8_t* __restrict__ hs, uint8_t* __restrict__ zero_ws,
                                                                                    const uint8_t* __restrict__ m_ws, uint8_t* __restrict__ Kp_ws,
                                                                                    uint8_t* __restrict__ r_ws) {
    const size_t item = (size_t)blockIdx.x * WAVE + lane_id();
    const size_t it = item < n ? item : n - 1;
    uint32_t mm[8], hh[8], w[8];
    load32(m_ws, 32, it, mm);
    load32(hs, 32, keyset_key(idx, n_keys, it), hh);
    KeccakState s;
    lane_G64(s, mm, hh);
    if (item < n) {
        MLKEM_STATE_WORDS8(s, 0, w)
        store32(Kp_ws, 32, item, w);
        MLKEM_STATE_WORDS8(s, 8, w)
        store32(r_ws, 32, item, w);
#pragma unroll
        for (int q = 0; q < 8; q++) w[q] = 0u;
        store32(zero_ws, 32, item, w);
    }
}

// K-PKE.Encrypt two items per wave (encrypt2_body) with ek and A-hat^T of each half-wave's key: the two items of a wave may have
// different keys, so the key rows are per-lane pointers (stride 0 inside the body), 64-bit offsets into the set
template <int K, int ETA1, int DU, int DV, int CMP>
__global__ void __launch_bounds__(WAVE * KPKE2_WAVES, kpke2_minwaves(K))
k_encrypt2_keyset(size_t n, const uint32_t* __restrict__ idx, size_t n_keys, const uint8_t* __restrict__ ek, size_t ek_stride,
                  const uint16_t* __restrict__ At, const uint8_t* __restrict__ msg, const uint8_t* __restrict__ prf, uint8_t* __restrict__ c_out,
                  const uint8_t* __restrict__ c_in, const uint8_t* __restrict__ Kp, uint8_t* __restrict__ Kout, uint32_t* __restrict__ rej,
                  uint32_t rej_base) {
    __shared__ K2Lds<K + 1> lds_all[KPKE2_WAVES];
    const int wv = wave_id();
    const size_t item0 = 2 * ((size_t)blockIdx.x * KPKE2_WAVES + wv);
    if (item0 >= n) return;
    const size_t h = (size_t)(lane_id() >> 5), item = item0 + h < n ? item0 + h : item0;   // the body's item of this half
    const size_t key = keyset_key(idx, n_keys, item);
    encrypt2_body<K, ETA1, DU, DV, CMP>(lds_all[wv].xch, item0, n, ek + key * ek_stride, 0, msg, At + key * (size_t)(K * K * 256), prf,
                                        c_out, c_in, Kp, (const uint8_t*)nullptr, Kout, (int32_t*)nullptr, 0, rej, rej_base);
}

// K-PKE.Decrypt four items per wave (decrypt4_body) with dk_pke of each item's key
template <int K, int DU, int DV>
__global__ void __launch_bounds__(64 * KPKE4_WAVES, kpke4_minwaves(K)) k_decrypt4_keyset(size_t n, const uint32_t* __restrict__ idx, size_t n_keys,
                                                                                       const uint8_t* __restrict__ dk, size_t dk_stride,
                                                                                       const uint8_t* __restrict__ c, uint8_t* __restrict__ m_out) {
    const size_t quad = (size_t)blockIdx.x * KPKE4_WAVES + wave_id();
    if (4 * quad >= n) return;
    const size_t item_raw = 4 * quad + (size_t)rntt_lane().p, item = item_raw < n ? item_raw : n - 1;   // the body's item of this lane
    decrypt4_body<K, DU, DV>(quad, n, dk + keyset_key(idx, n_keys, item) * dk_stride, 0, c, m_out);
}

// status[i] = 0, or MLKEM_ERR_ARG with c_i (when c is given) and K_i zeroed where idx[i] >= n_keys
__global__ void __launch_bounds__(256) k_keyset_fix(size_t n, const uint32_t* __restrict__ idx, size_t n_keys, uint8_t* __restrict__ c,
                                                    unsigned c_len, uint8_t* __restrict__ Kout, int32_t* __restrict__ status) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const bool bad = idx && (size_t)idx[i] >= n_keys;
        if (status) status[i] = bad ? KS_ERR_ARG : 0;
        if (!bad) continue;
        uint32_t* k = reinterpret_cast<uint32_t*>(Kout + i * 32);
        for (int w = 0; w < 8; w++) k[w] = 0;
        if (c) {
            uint32_t* cw = reinterpret_cast<uint32_t*>(c + i * c_len);
            for (unsigned w = 0; w < c_len / 4; w++) cw[w] = 0;
        }
    }
}

// *out |= status[0 .. n): the import's refusal test in one word (*out zeroed before, in stream order)
__global__ void __launch_bounds__(256) k_keyset_status_or(size_t n, const int32_t* __restrict__ status, uint32_t* __restrict__ out) {
    uint32_t v = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) v |= (uint32_t)status[i];
    if (v) atomicOr(out, v);
}

// ------------------------------------------------------------------------------------------------
// Small calls: one workgroup per item (mlkem_small.hpp's hand-over scheme).  The job counter starts at k^2, so small_jobs hands
// out the 2k + 1 PRF rows alone; A-hat^T is read by encrypt1_body straight from the set (it requests the whole matrix up front).
// ------------------------------------------------------------------------------------------------
template <int K, int ETA1>
struct __attribute__((aligned(16))) KeysetHand {
    uint8_t prf[(2 * K + 1) * (ETA1 == 3 ? 192 : 128)];
    uint8_t r[32], m[32], Kp[32], Kbar[32];
};

// an item whose index is out of range: c (when given) and K zeroed, status MLKEM_ERR_ARG -- by wave 0 of its workgroup
__device__ __forceinline__ void keyset_small_reject(size_t item, uint8_t* c, unsigned c_len, uint8_t* Kout, int32_t* status) {
    const unsigned l = (unsigned)lane_id();
    if (l < 8) reinterpret_cast<uint32_t*>(Kout + item * 32)[l] = 0;
    if (c)
        for (unsigned w = l; w < c_len / 4; w += WAVE) reinterpret_cast<uint32_t*>(c + item * c_len)[w] = 0;
    if (l == 0 && status) status[item] = KS_ERR_ARG;
}

// ML-KEM.Encaps_internal (ml_kem.c:1093-1130) to the item's key: wave 0: (K, r) = G(m || h), r_ready | every wave: the 2k + 1 PRF
// rows | wave 0: K-PKE.Encrypt, then it zeroes r, the PRF rows and the NTT exchange
template <int K, int ETA1, int DU, int DV, int NW>
__global__ void __launch_bounds__(WAVE * NW)
k_encaps_keyset_small(size_t n, const uint32_t* __restrict__ idx, size_t n_keys, const uint8_t* __restrict__ ek, size_t ek_stride,
                      const uint8_t* __restrict__ hs, const uint16_t* __restrict__ At, const uint8_t* __restrict__ m, uint8_t* __restrict__ c,
                      uint8_t* __restrict__ Kout, int32_t* __restrict__ status, int prf_rate) {
    __shared__ K2Lds<K + 1> xl;
    __shared__ KeysetHand<K, ETA1> hand;
    __shared__ uint2 rc_tables[NW][WK_RC_ENTRIES];
    __shared__ SmallSync sy;
    constexpr unsigned CLEN = 32 * (DU * K + DV);
    const int wv = wave_id();
    const size_t item = blockIdx.x;
    if (item >= n) return;
    const size_t key = idx ? (size_t)idx[item] : 0;
    if (key >= n_keys) {   // workgroup-uniform
        if (wv == 0) keyset_small_reject(item, c, CLEN, Kout, status);
        return;
    }
    const uint8_t* my_ek = ek + key * ek_stride;
    WkLane cst;
    wk_lane_init(cst, rc_tables[wave_id()]);
    if (threadIdx.x == 0) { sy.next_job = K * K; sy.jobs_done = 0; sy.r_ready = 0; sy.kbar_ready = 0; }
    block_barrier();
    if (wv == 0) {                                   // (K, r) = G(m || h)
        const int i = wk_index();
        uint2 v;
        v.x = 0; v.y = 0;
        if (i >= 0 && i < 4) v = reinterpret_cast<const uint2*>(m + item * 32)[i];
        else if (i >= 4 && i < 8) v = reinterpret_cast<const uint2*>(hs + key * 32)[i - 4];
        WkState a;
        a.lo = v.x; a.hi = v.y;
        if (i == 8) { a.lo = 0x06u; a.hi = 0x80000000u; }
        wk_permute(a, cst);
        uint2 o;
        o.x = a.lo; o.y = a.hi;
        if (wk_primary() && i < 4) reinterpret_cast<uint2*>(Kout + item * 32)[i] = o;
        else if (wk_primary() && i < 8) reinterpret_cast<uint2*>(hand.r)[i - 4] = o;
        flag_signal(&sy.r_ready);
    }
    small_jobs<K, ETA1>(sy, cst, nullptr, /*transpose=*/true, nullptr, hand.r, hand.prf, 2 * K + 1, (unsigned)prf_rate, nullptr);
    if (wv != 0) return;
    flag_wait(&sy.jobs_done, (uint32_t)(2 * K + 1));
    encrypt1_body<K, ETA1, DU, DV, false>(xl.xch, my_ek, m + item * 32, At + key * (size_t)(K * K * 256), hand.prf, c + item * CLEN, nullptr,
                                          nullptr, nullptr, nullptr, nullptr);
    if (lane_id() == 0 && status) status[item] = 0;
    wave_lds_fence();
    wave_zero_lds(hand);
    wave_zero_lds(xl);
#ifdef MLKEM_EMU_LDS_PROBE
    if (lane_id() == 0) { MLKEM_EMU_LDS_PROBE(&hand, sizeof hand); MLKEM_EMU_LDS_PROBE(&xl, sizeof xl); }
#endif
}

// Decaps_internal (ml_kem.c:1136-1225) under the item's key: wave 0: m' = K-PKE.Decrypt, (K', r') = G(m' || h), r_ready | wave 1:
// Kbar = J(z || c), kbar_ready | every wave: the 2k + 1 PRF rows | wave 0: c' = Encrypt, K = c == c' ? K' : Kbar, then it zeroes
// m', K', Kbar, r', the PRF rows and the NTT exchange
template <int K, int ETA1, int DU, int DV, int JRATE, int NW>
__global__ void __launch_bounds__(WAVE * NW)
k_decaps_keyset_small(size_t n, const uint32_t* __restrict__ idx, size_t n_keys, const uint8_t* __restrict__ dk, size_t dk_stride,
                      const uint8_t* __restrict__ hs, const uint16_t* __restrict__ At, const uint8_t* __restrict__ c, uint8_t* __restrict__ Kout,
                      int32_t* __restrict__ status, int prf_rate) {
    static_assert(NW >= 2, "roles of waves 0 and 1");
    __shared__ K2Lds<K + 1> xl;
    __shared__ KeysetHand<K, ETA1> hand;
    __shared__ uint2 rc_tables[NW][WK_RC_ENTRIES];
    __shared__ SmallSync sy;
    constexpr unsigned DK = 768 * K + 96, CLEN = 32 * (DU * K + DV);
    const int wv = wave_id();
    const size_t item = blockIdx.x;
    if (item >= n) return;
    const size_t key = idx ? (size_t)idx[item] : 0;
    if (key >= n_keys) {   // workgroup-uniform
        if (wv == 0) keyset_small_reject(item, nullptr, CLEN, Kout, status);
        return;
    }
    const uint8_t* my_dk = dk + key * dk_stride;
    const uint8_t* my_c = c + item * CLEN;
    WkLane cst;
    wk_lane_init(cst, rc_tables[wave_id()]);
    const int i = wk_index();
    const bool prim = wk_primary();
    if (threadIdx.x == 0) { sy.next_job = K * K; sy.jobs_done = 0; sy.r_ready = 0; sy.kbar_ready = 0; }
    block_barrier();
    if (wv == 0) {                                   // m' = K-PKE.Decrypt(dk_pke, c) ; (K', r') = G(m' || h)
        decrypt4_body<K, DU, DV>(0, 1, my_dk, (size_t)DK, my_c, hand.m);
        wave_global_fence();
        uint2 v;
        v.x = 0; v.y = 0;
        if (i >= 0 && i < 4) v = reinterpret_cast<const uint2*>(hand.m)[i];
        else if (i >= 4 && i < 8) v = reinterpret_cast<const uint2*>(hs + key * 32)[i - 4];
        WkState a;
        a.lo = v.x; a.hi = v.y;
        if (i == 8) { a.lo = 0x06u; a.hi = 0x80000000u; }
        wk_permute(a, cst);
        uint2 o;
        o.x = a.lo; o.y = a.hi;
        if (prim && i < 4) reinterpret_cast<uint2*>(hand.Kp)[i] = o;
        else if (prim && i < 8) reinterpret_cast<uint2*>(hand.r)[i - 4] = o;
        flag_signal(&sy.r_ready);
    } else if (wv == 1) {                            // Kbar = J(z || c): only the final select waits for it
        WkState a;
        wk_absorb<JRATE, 0x1F>(a, cst, my_dk + 768 * K + 64, 32, my_c, 32 + CLEN);
        uint2 o;
        o.x = a.lo; o.y = a.hi;
        if (prim && i < 4) reinterpret_cast<uint2*>(hand.Kbar)[i] = o;
        flag_signal(&sy.kbar_ready);
    }
    small_jobs<K, ETA1>(sy, cst, nullptr, /*transpose=*/true, nullptr, hand.r, hand.prf, 2 * K + 1, (unsigned)prf_rate, nullptr);
    if (wv != 0) return;
    flag_wait(&sy.jobs_done, (uint32_t)(2 * K + 1));
    encrypt1_body<K, ETA1, DU, DV, true>(xl.xch, my_dk + 384 * K, hand.m, At + key * (size_t)(K * K * 256), hand.prf, nullptr, my_c, hand.Kp,
                                         hand.Kbar, Kout + item * 32, nullptr, &sy.kbar_ready);
    if (lane_id() == 0 && status) status[item] = 0;
    // the fence: every lane's reads of K' and Kbar for the select are done before any lane overwrites them
    wave_lds_fence();
    wave_zero_lds(hand);
    wave_zero_lds(xl);
#ifdef MLKEM_EMU_LDS_PROBE
    if (lane_id() == 0) { MLKEM_EMU_LDS_PROBE(&hand, sizeof hand); MLKEM_EMU_LDS_PROBE(&xl, sizeof xl); }
#endif
}

// ------------------------------------------------------------------------------------------------
// Sequencing
// ------------------------------------------------------------------------------------------------
inline size_t keyset_table_bytes_per_key(const ParamSet& p, bool has_dk) {
    return (has_dk ? (size_t)p.dk_len : (size_t)p.ek_len) + 32 + (size_t)(p.k * p.k) * 512;
}

// Import of n_keys keys already copied into ks.keys: status[i] = the check bits of mlkem_check_keys_dev (ek or dk alone; nullptr
// for a seed import, whose keys are consistent by construction), ORed into *status_or (zeroed here); then the H and A-hat^T
// tables.  hs / At: the set's tables, written here; status_or: two words.
template <int K>
inline void keyset_import_run(stream_t st, const ParamSet& p, const KeysetView& ks, uint8_t* hs, uint16_t* At, int32_t* status,
                              uint32_t* status_or, const Workspace& ws) {
    const size_t n = ks.n_keys;
    zero_u32x2(st, status_or);
    if (status) {
        const uint8_t* ek = ks.has_dk ? nullptr : ks.keys;
        const uint8_t* dk = ks.has_dk ? ks.keys : nullptr;
        check_keys_dispatch(st, p.set, n, ek, dk, nullptr, nullptr, status, nullptr, min_sz(n, ws.cap), ws);
        launch("k_keyset_status_or", k_keyset_status_or, min_sz(ceil_div(n, 256), 1024), 256u, st, n, (const int32_t*)status, status_or);
    }
    hash_launch(st, 0, n, ks.keys + ks.ek_off, p.ek_len, ks.key_stride, hs);
    for (size_t c0 = 0; c0 < n; c0 += ws.cap) {   // A-hat^T[a][b] = SampleNTT(rho || a || b) straight into the set's table
        const size_t cn = min_sz(ws.cap, n - c0);
        Workspace w = ws;
        w.A = At + c0 * (size_t)(K * K * 256);
        launch_sample_split(st, p, cn, 0, ks.keys + c0 * ks.key_stride + ks.ek_off + 384 * K, ks.key_stride, /*transpose=*/1, nullptr, 0, 0, w);
    }
}

// seed import: d || z (n x 64) -> KeyGen_internal into the set's dk table; tmp: n x (64 + ek_len) bytes the caller zeroes afterwards
inline void keyset_seed_run(stream_t st, const ParamSet& p, size_t n, const uint8_t* seed, uint8_t* dk, uint8_t* tmp, const Workspace& ws) {
    uint8_t *d = tmp, *z = d + n * 32, *ek = z + n * 32;
    launch("k_seed_split", k_seed_split, ceil_div(4 * n, 256), 256, st, n, reinterpret_cast<const uint4*>(seed), reinterpret_cast<uint4*>(d),
           reinterpret_cast<uint4*>(z));
    keygen_dispatch(st, p.set, n, d, z, ek, dk, ws);
}

template <int K, int ETA1, int DU, int DV>
inline void encaps_keyset_run(stream_t st, const ParamSet& p, const KeysetView& ks, size_t n, const uint32_t* idx, const uint8_t* m, uint8_t* c,
                              uint8_t* Kout, int32_t* status, const Workspace& ws, const KeysetLimits& lim) {
    if (n == 0) return;
    const uint8_t* ek = ks.keys + ks.ek_off;
    if (n <= lim.enc_max(K)) {   // one launch, one workgroup per item
        const int rate = ws.fips ? 136 : 168;
        if (n <= lim.enc_lat(K))
            launch("k_encaps_keyset_small", k_encaps_keyset_small<K, ETA1, DU, DV, SMALL_WAVES>, n, WAVE * SMALL_WAVES, st, n, idx, ks.n_keys, ek,
                   ks.key_stride, ks.h, ks.At, m, c, Kout, status, rate);
        else
            launch("k_encaps_keyset_small", k_encaps_keyset_small<K, ETA1, DU, DV, SMALL_WAVES_DENSE>, n, WAVE * SMALL_WAVES_DENSE, st, n, idx,
                   ks.n_keys, ek, ks.key_stride, ks.h, ks.At, m, c, Kout, status, rate);
        return;
    }
    for (size_t h0 = 0; h0 < n; h0 += ws.hcap) {
        const size_t hn = min_sz(ws.hcap, n - h0);
        const uint32_t* idh = idx ? idx + h0 : nullptr;
        launch("k_hash_g_keyset", k_hash_g_keyset, ceil_div(hn, WAVE), WAVE, st, hn, idh, ks.n_keys, m + h0 * 32, ks.h, Kout + h0 * 32, ws.r);
        for (size_t c0 = 0; c0 < hn; c0 += ws.cap) {
            const size_t cn = min_sz(ws.cap, hn - c0), i0 = h0 + c0;
            launch_sample_split(st, p, 0, cn, nullptr, 0, 1, ws.r + c0 * 32, 2 * K + 1, K, ws);   // PRF rows per item
            launch("k_encrypt_keyset", k_encrypt2_keyset<K, ETA1, DU, DV, CMP_NONE>, ceil_div(ceil_div(cn, 2), KPKE2_WAVES), WAVE * KPKE2_WAVES, st, cn,
                   idx ? idx + i0 : nullptr, ks.n_keys, ek, ks.key_stride, ks.At, m + i0 * 32, (const uint8_t*)ws.prf, c + i0 * p.c_len,
                   (const uint8_t*)nullptr, (const uint8_t*)nullptr, (uint8_t*)nullptr, (uint32_t*)nullptr, 0u);
        }
    }
    if (idx || status)
        launch("k_keyset_fix", k_keyset_fix, min_sz(ceil_div(n, 256), 1024), 256u, st, n, idx, ks.n_keys, c, p.c_len, Kout, status);
}

template <int K, int ETA1, int DU, int DV>
inline void decaps_keyset_run(stream_t st, const ParamSet& p, const KeysetView& ks, size_t n, const uint32_t* idx, const uint8_t* c,
                              uint8_t* Kout, int32_t* status, const Workspace& ws, const KeysetLimits& lim) {
    constexpr int CLEN = 32 * (DU * K + DV);
    if (n == 0) return;
    if (n <= lim.dec_max(K)) {   // one launch, one workgroup per item
        const int rate = ws.fips ? 136 : 168;
#define MLKEM_DKS(JR, NW) launch("k_decaps_keyset_small", k_decaps_keyset_small<K, ETA1, DU, DV, JR, NW>, n, WAVE * NW, st, n, idx, ks.n_keys, \
                                 ks.keys, ks.key_stride, ks.h, ks.At, c, Kout, status, rate)
        if (!ws.fips && n <= lim.dec_lat(K)) MLKEM_DKS(168, SMALL_WAVES);
        else if (!ws.fips) MLKEM_DKS(168, SMALL_WAVES_DENSE);
        else if (n <= lim.dec_lat(K)) MLKEM_DKS(136, SMALL_WAVES);
        else MLKEM_DKS(136, SMALL_WAVES_DENSE);
#undef MLKEM_DKS
        return;
    }
    for (size_t h0 = 0; h0 < n; h0 += ws.hcap) {
        const size_t hn = min_sz(ws.hcap, n - h0);
        const uint32_t* idh = idx ? idx + h0 : nullptr;
        const uint8_t* ch = c + h0 * p.c_len;
        launch("k_decrypt_keyset", k_decrypt4_keyset<K, DU, DV>, ceil_div(ceil_div(hn, 4), KPKE4_WAVES), 64 * KPKE4_WAVES, st, hn, idh, ks.n_keys,
               ks.keys, ks.key_stride, ch, ws.m);
        reject_list_reset(st, ws);
        launch("k_hash_decaps_keyset", k_hash_decaps_keyset, ceil_div(hn, WAVE), WAVE, st, hn, idh, ks.n_keys, ks.h, ws.rho, (const uint8_t*)ws.m,
               ws.Kp, ws.r);
        for (size_t c0 = 0; c0 < hn; c0 += ws.cap) {
            const size_t cn = min_sz(ws.cap, hn - c0), i0 = h0 + c0;
            launch_sample_split(st, p, 0, cn, nullptr, 0, 1, ws.r + c0 * 32, 2 * K + 1, K, ws);
            launch("k_encrypt_cmp_keyset", k_encrypt2_keyset<K, ETA1, DU, DV, CMP_DEFER>, ceil_div(ceil_div(cn, 2), KPKE2_WAVES), WAVE * KPKE2_WAVES,
                   st, cn, idx ? idx + i0 : nullptr, ks.n_keys, ks.keys + 384 * K, ks.key_stride, ks.At, (const uint8_t*)(ws.m + c0 * 32),
                   (const uint8_t*)ws.prf, (uint8_t*)nullptr, c + i0 * p.c_len, (const uint8_t*)(ws.Kp + c0 * 32), Kout + i0 * 32, reject_list(ws),
                   (uint32_t)c0);
        }
        // J(z || c) of the rejected items, z from the set by index -- before k_keyset_fix, which zeroes the K rows of bad indices
        j_rejected_launch<CLEN>(st, ws, hn, ks.keys + 768 * K + 64, ks.key_stride, idh, ks.n_keys, ch, Kout + h0 * 32);
    }
    if (idx || status)
        launch("k_keyset_fix", k_keyset_fix, min_sz(ceil_div(n, 256), 1024), 256u, st, n, idx, ks.n_keys, (uint8_t*)nullptr, p.c_len, Kout, status);
}

inline int keyset_import_dispatch(stream_t st, const ParamSet& p, const KeysetView& ks, uint8_t* hs, uint16_t* At, int32_t* status,
                                  uint32_t* status_or, const Workspace& ws) {
    switch (p.set) {
    case 512: keyset_import_run<2>(st, p, ks, hs, At, status, status_or, ws); break;
    case 768: keyset_import_run<3>(st, p, ks, hs, At, status, status_or, ws); break;
    default: keyset_import_run<4>(st, p, ks, hs, At, status, status_or, ws); break;
    }
    return 0;
}
inline int encaps_keyset_dispatch(stream_t st, const ParamSet& p, const KeysetView& ks, size_t n, const uint32_t* idx, const uint8_t* m,
                                  uint8_t* c, uint8_t* K, int32_t* status, const Workspace& ws, const KeysetLimits& lim) {
    switch (p.set) {
    case 512: encaps_keyset_run<2, 3, 10, 4>(st, p, ks, n, idx, m, c, K, status, ws, lim); break;
    case 768: encaps_keyset_run<3, 2, 10, 4>(st, p, ks, n, idx, m, c, K, status, ws, lim); break;
    default: encaps_keyset_run<4, 2, 11, 5>(st, p, ks, n, idx, m, c, K, status, ws, lim); break;
    }
    return 0;
}
inline int decaps_keyset_dispatch(stream_t st, const ParamSet& p, const KeysetView& ks, size_t n, const uint32_t* idx, const uint8_t* c,
                                  uint8_t* K, int32_t* status, const Workspace& ws, const KeysetLimits& lim) {
    switch (p.set) {
    case 512: decaps_keyset_run<2, 3, 10, 4>(st, p, ks, n, idx, c, K, status, ws, lim); break;
    case 768: decaps_keyset_run<3, 2, 10, 4>(st, p, ks, n, idx, c, K, status, ws, lim); break;
    default: decaps_keyset_run<4, 2, 11, 5>(st, p, ks, n, idx, c, K, status, ws, lim); break;
    }
    return 0;
}

}   // namespace mlkem
