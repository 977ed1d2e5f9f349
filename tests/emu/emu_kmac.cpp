// tests/emu/emu_kmac.cpp — TEST INFRASTRUCTURE ONLY: the three kernels of mlkem_kmac.hpp (k_kmac_prefix; k_kmac_ragged: one sponge per
// lane; k_kmac_ragged_w: one sponge per wavefront) compiled for the host wave emulator (hip_emu.hpp) and sequenced by the product's own
// kmac_launch, the per-item form forced by the caller.  Every message or key load the kernels issue is recorded through the
// MLKEM_EMU_LOAD_PROBE hook of mlkem_sha3r.hpp and checked after the launch against the memory rule of the call: a naturally aligned
// 8-byte load holding at least one byte of the item's own key, head or body (of the shared key for the prefix kernel's loads).  The
// LDS the wave-wide kernels report through MLKEM_EMU_LDS_PROBE (their round-constant tables) is read back by emu_kmac_lds_nonzero,
// and the midstate region (owned by this file, as a context owns it in the product) by emu_kmac_mid_nonzero.
#include "hip_emu.hpp"

#include <stddef.h>

#include <mutex>
#include <vector>

struct LoadRec { size_t item; const void* p; unsigned bytes; };
static std::vector<LoadRec> g_loads;
static std::mutex g_mu;
static void probe_load(size_t item, const void* p, unsigned bytes) {
    std::lock_guard<std::mutex> lock(g_mu);
    g_loads.push_back({item, p, bytes});
}
#define MLKEM_EMU_LOAD_PROBE(item, p, bytes) probe_load((item), (p), (bytes))

struct LdsRegion { const void* p; size_t bytes; };
static LdsRegion g_regions[16];
static int g_nregions = 0;
static void probe_region(const void* p, size_t bytes) {
    std::lock_guard<std::mutex> lock(g_mu);
    for (int i = 0; i < g_nregions; i++)
        if (g_regions[i].p == p) return;
    if (g_nregions < 16) g_regions[g_nregions++] = {p, bytes};
}
#define MLKEM_EMU_LDS_PROBE(p, bytes) probe_region((p), (bytes))

#include "../../crystals-kyber_amd/csrc/mlkem_pipeline.hpp"

using namespace mlkem;

static size_t g_last_loads = 0;
alignas(16) static uint64_t g_mid[KMAC_MID_BYTES / 8];

static bool overlaps(uintptr_t p, size_t bytes, uintptr_t q, size_t len) { return len && p < q + len && q < p + bytes; }

// one call: argument check, launch, load audit.  0, -101 for an argument error (nothing ran), -3 when a load breaks the memory rule
static int run(int form, KmacCall& c) {
    unsigned rate = 0;
    if (!kmac_check_args(c, true, rate)) return -101;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        g_loads.clear();
    }
    g_last_loads = 0;
    const Sha3rArgs& a = c.s;
    if (a.n == 0) return 0;
    if (kmac_launch(nullptr, rate, c, g_mid, form ? (size_t)-1 : 0)) return -101;
    std::lock_guard<std::mutex> lock(g_mu);
    g_last_loads = g_loads.size();
    const bool per_item = c.kmac && c.key_stride, shared = c.kmac && !c.key_stride;
    for (const LoadRec& r : g_loads) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(r.p);
        if (r.bytes != 8 || p % 8) return -3;
        if (r.item == KMAC_ITEM_NONE) {          // the prefix kernel: the shared key only
            if (!shared || !overlaps(p, 8, reinterpret_cast<uintptr_t>(c.key), c.key_len)) return -3;
            continue;
        }
        if (r.item >= a.n) return -3;
        const uint64_t off = a.body_off[r.item];
        const uint32_t len = a.body_len[r.item];
        if (off > a.body_bytes || len > a.body_bytes - off) return -3;   // an out-of-bounds item loads nothing
        const bool in_key = per_item && overlaps(p, 8, reinterpret_cast<uintptr_t>(c.key) + r.item * c.key_stride, c.key_len);
        const bool in_head = overlaps(p, 8, reinterpret_cast<uintptr_t>(a.head) + r.item * a.head_stride, a.head_len);
        const bool in_body = overlaps(p, 8, reinterpret_cast<uintptr_t>(a.body) + (uintptr_t)off, len);
        if (!in_key && !in_head && !in_body) return -3;
    }
    return 0;
}

extern "C" {
// form 0: lane-sliced, 1: one sponge per wavefront
int emu_cshake(int form, int bits, size_t n, const uint8_t* fname, unsigned fname_len, const uint8_t* custom, unsigned custom_len,
               const uint8_t* lead, unsigned lead_len, const uint8_t* head, unsigned head_len, size_t head_stride, const uint8_t* body,
               size_t body_bytes, const uint64_t* body_off, const uint32_t* body_len, uint8_t* out, unsigned outlen, size_t out_stride,
               int32_t* status) {
    KmacCall c{bits, false, false, fname, fname_len, custom, custom_len, lead, lead_len, nullptr, 0, 0,
               Sha3rArgs{n, head, head_len, head_stride, body, body_bytes, body_off, body_len, out, outlen, out_stride, status, 0}};
    return run(form, c);
}
// alg: MLKEM_KMAC128 .. MLKEM_KMACXOF256 (0..3)
int emu_kmac(int form, int alg, size_t n, const uint8_t* key, unsigned key_len, size_t key_stride, const uint8_t* custom, unsigned custom_len,
             const uint8_t* lead, unsigned lead_len, const uint8_t* head, unsigned head_len, size_t head_stride, const uint8_t* body,
             size_t body_bytes, const uint64_t* body_off, const uint32_t* body_len, uint8_t* out, unsigned outlen, size_t out_stride,
             int32_t* status) {
    if (alg < 0 || alg > 3) return -101;
    KmacCall c{(alg & 1) ? 256 : 128, true, alg >= 2, nullptr, 0, custom, custom_len, lead, lead_len, key, key_len, key_stride,
               Sha3rArgs{n, head, head_len, head_stride, body, body_bytes, body_off, body_len, out, outlen, out_stride, status, 0}};
    return run(form, c);
}
size_t emu_kmac_loads(void) { return g_last_loads; }
int emu_kmac_lds_regions(void) {
    std::lock_guard<std::mutex> lock(g_mu);
    return g_nregions;
}
long emu_kmac_lds_nonzero(void) {
    std::lock_guard<std::mutex> lock(g_mu);
    long nz = 0;
    for (int i = 0; i < g_nregions; i++)
        for (size_t b = 0; b < g_regions[i].bytes; b++) nz += static_cast<const uint8_t*>(g_regions[i].p)[b] != 0;
    return nz;
}
// nonzero bytes of the midstate region (zero after a shared-key call; the public prefix state of the last call otherwise)
long emu_kmac_mid_nonzero(void) {
    long nz = 0;
    for (size_t b = 0; b < sizeof g_mid; b++) nz += reinterpret_cast<const uint8_t*>(g_mid)[b] != 0;
    return nz;
}
}
