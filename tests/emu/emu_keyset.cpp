// tests/emu/emu_keyset.cpp — TEST INFRASTRUCTURE ONLY: prepared key sets (mlkem_keyset.hpp: the import, the one-workgroup-per-item
// kernels k_encaps_keyset_small / k_decaps_keyset_small and the indexed batch path) compiled for the host wave emulator
// (hip_emu.hpp), with lowered cap / hcap / small limits so that every path and chunk loop runs on a few items.  The set lives in
// host memory laid out as mlkem_keyset_create lays it out.  It also records the secret-bearing LDS regions of the small kernels, so
// that a test can read them after the launch (under the emulator __shared__ objects are statics that outlive it).
#include "hip_emu.hpp"

#include <stddef.h>

#include <mutex>

struct LdsRegion { const void* p; size_t bytes; };
static LdsRegion g_regions[16];
static int g_nregions = 0;
static std::mutex g_regions_mu;
static void probe_region(const void* p, size_t bytes) {
    std::lock_guard<std::mutex> lock(g_regions_mu);
    for (int i = 0; i < g_nregions; i++)
        if (g_regions[i].p == p) return;
    if (g_nregions < 16) g_regions[g_nregions++] = {p, bytes};
}
#define MLKEM_EMU_LDS_PROBE(p, bytes) probe_region((p), (bytes))

#include "../../crystals-kyber_amd/csrc/mlkem_keyset.hpp"

#include <stdlib.h>
#include <string.h>

using namespace mlkem;

static size_t g_cap = 0, g_hcap = 0, g_small = 0, g_small_lat = 0;
static int g_fips = 0;

static void* xalloc(size_t bytes) { return aligned_alloc(64, (bytes + 127) / 64 * 64); }

struct EmuWs {
    Workspace ws;
    explicit EmuWs(size_t n) {
        ws.cap = g_cap ? g_cap : (n ? n : 1);
        ws.hcap = g_hcap ? g_hcap : ws.cap;
        if (ws.hcap < ws.cap) ws.hcap = ws.cap;
        ws.fips = g_fips;
        ws.wide_max = 0;
        ws.small_max_k[0] = ws.small_max_k[1] = ws.small_max_k[2] = 0;   // KeyGen of a seed import: the batch kernels
        ws.small_wide_max = 0;
        ws.A = (uint16_t*)xalloc(ws.cap * 16 * 512);
        ws.prf = (uint8_t*)xalloc(ws.cap * 9 * 192);
        ws.leftover = (uint32_t*)xalloc((ws.cap * 16 + 2) * 4);
        ws.resume = (uint32_t*)xalloc((size_t)64 * RESUME_WORDS * 4 + 16);
        ws.resume_cap = 64;
        ws.r = (uint8_t*)xalloc(ws.hcap * 32);
        ws.rho = (uint8_t*)xalloc(ws.hcap * 32);
        ws.m = (uint8_t*)xalloc(ws.hcap * 32);
        ws.Kp = (uint8_t*)xalloc(ws.hcap * 32);
        ws.Kbar = (uint8_t*)xalloc(ws.hcap * 32);
    }
    ~EmuWs() {
        free(ws.A); free(ws.prf); free(ws.leftover); free(ws.resume);
        free(ws.r); free(ws.rho); free(ws.m); free(ws.Kp); free(ws.Kbar);
    }
};

static ParamSet g_p;
static KeysetView g_ks;
static uint8_t* g_mem = nullptr;

extern "C" {
// cap / hcap: chunk and h-chunk capacity (0: the call's n); small: key-set calls of at most this many items run the small kernels,
// of which calls of at most small_lat use eight waves per item (four above)
void emu_ks_config(size_t cap, size_t hcap, size_t small_max, size_t small_lat) { g_cap = cap; g_hcap = hcap; g_small = small_max; g_small_lat = small_lat; }
void emu_ks_conformance(int fips) { g_fips = fips != 0; }
void emu_ks_destroy(void) {
    free(g_mem);
    g_mem = nullptr;
    g_ks = KeysetView();
}
// mlkem_keyset_create's sequence on host memory: 0, -6 (refused: some key_status word nonzero), -1 bad arguments
int emu_ks_create(int set, size_t n, const uint8_t* ek, const uint8_t* dk, const uint8_t* seed, int32_t* key_status) {
    emu_ks_destroy();
    ParamSet p;
    if (!param_set(set, p) || n == 0 || (ek ? 1 : 0) + (dk ? 1 : 0) + (seed ? 1 : 0) != 1) return -1;
    EmuWs w(n);
    const bool has_dk = ek == nullptr;
    const size_t key_len = has_dk ? p.dk_len : p.ek_len;
    g_mem = (uint8_t*)xalloc(n * (key_len + 32 + (size_t)(p.k * p.k) * 512));
    uint8_t* keys = g_mem;
    uint8_t* hs = keys + n * key_len;
    uint16_t* At = reinterpret_cast<uint16_t*>(hs + n * 32);
    uint32_t status_or[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    if (seed) {
        uint8_t* tmp = (uint8_t*)xalloc(n * (64 + p.ek_len));
        keyset_seed_run(nullptr, p, n, seed, keys, tmp, w.ws);
        free(tmp);
        memset(key_status, 0, n * 4);
    } else {
        memcpy(keys, ek ? ek : dk, n * key_len);
    }
    g_p = p;
    g_ks.keys = keys;
    g_ks.key_stride = key_len;
    g_ks.ek_off = has_dk ? 384u * p.k : 0;
    g_ks.h = hs;
    g_ks.At = At;
    g_ks.n_keys = n;
    g_ks.has_dk = has_dk;
    keyset_import_dispatch(nullptr, p, g_ks, hs, At, seed ? nullptr : key_status, status_or, w.ws);
    if (status_or[0]) {
        emu_ks_destroy();
        return -6;
    }
    return 0;
}
static KeysetLimits limits() {
    KeysetLimits lim;
    lim.set_all(g_small, g_small_lat);
    return lim;
}
int emu_ks_encaps(size_t n, const uint32_t* idx, const uint8_t* m, uint8_t* c, uint8_t* K, int32_t* status) {
    if (!g_mem) return -1;
    EmuWs w(n);
    return encaps_keyset_dispatch(nullptr, g_p, g_ks, n, idx, m, c, K, status, w.ws, limits());
}
// -2: the batch path left a gathered z row in the context scratch (ws.rho) instead of zeroing it after use
int emu_ks_decaps(size_t n, const uint32_t* idx, const uint8_t* c, uint8_t* K, int32_t* status) {
    if (!g_mem || !g_ks.has_dk) return -1;
    EmuWs w(n);
    memset(w.ws.rho, 0xA5, w.ws.hcap * 32);
    int rc = decaps_keyset_dispatch(nullptr, g_p, g_ks, n, idx, c, K, status, w.ws, limits());
    if (rc == 0 && n > g_small)
        for (size_t b = 0; b < (n < w.ws.hcap ? n : w.ws.hcap) * 32; b++)
            if (w.ws.rho[b]) return -2;
    return rc;
}
// the H and A-hat^T tables of the set (for the tests' own check of what import stored)
size_t emu_ks_tables(uint8_t* h_out, uint16_t* a_out) {
    if (!g_mem) return 0;
    memcpy(h_out, g_ks.h, g_ks.n_keys * 32);
    memcpy(a_out, g_ks.At, g_ks.n_keys * (size_t)(g_p.k * g_p.k) * 512);
    return g_ks.n_keys;
}
// secret-bearing LDS regions of the small kernels: how many were recorded, and how many nonzero bytes they hold now
int emu_ks_lds_regions(void) {
    std::lock_guard<std::mutex> lock(g_regions_mu);
    return g_nregions;
}
size_t emu_ks_lds_nonzero(void) {
    std::lock_guard<std::mutex> lock(g_regions_mu);
    size_t nz = 0;
    for (int i = 0; i < g_nregions; i++)
        for (size_t b = 0; b < g_regions[i].bytes; b++) nz += static_cast<const uint8_t*>(g_regions[i].p)[b] != 0;
    return nz;
}
void emu_ks_lds_reset(void) {
    std::lock_guard<std::mutex> lock(g_regions_mu);
    g_nregions = 0;
}
}
