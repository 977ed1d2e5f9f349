// tests/emu/emu_check.cpp — TEST INFRASTRUCTURE ONLY: batched key validation (check_keys_run: the structural check kernel
// k_check_keys with the in-kernel wave-wide hash or the lane-sliced pre-pass, and the seed / PCT legs through the staging region)
// compiled for the host wave emulator (hip_emu.hpp), with lowered cap / wide / small limits so that every path runs on a few
// items.  It also records the LDS block of k_check_keys' sponge wave, so that a test can read what it holds after the launch (under
// the emulator __shared__ objects are statics that outlive it).
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

#include "../../crystals-kyber_amd/csrc/mlkem_pipeline.hpp"

#include <stdlib.h>
#include <string.h>

using namespace mlkem;

static size_t g_cap = 0, g_wide = 4096, g_small = 0;
static int g_fips = 0;
static size_t g_last_chunk = 0;

static void* xalloc(size_t bytes) { return aligned_alloc(64, (bytes + 127) / 64 * 64); }

extern "C" {
// cap: chunk capacity of the context (0: the call's n); wide: ws.wide_kem (in-kernel hash up to this many items); small: small_max
void emu_check_config(size_t cap, size_t wide, size_t small_max) { g_cap = cap; g_wide = wide; g_small = small_max; }
void emu_check_conformance(int fips) { g_fips = fips != 0; }
// status = mlkem_check_keys_dev on a context of the configured limits; the staging region is sized as a context's
// (max(cap, 2) items of ML-KEM-1024's 4800 bytes) and must read back as zero after the call (returns -2 otherwise)
int emu_check_keys(int set, size_t n, const uint8_t* ek, const uint8_t* dk, const uint8_t* seed, const uint8_t* m, int32_t* status) {
    ParamSet p, p4;
    if (!param_set(set, p)) return -1;
    (void)param_set(1024, p4);
    Workspace ws;
    ws.cap = g_cap ? g_cap : (n ? n : 1);
    ws.hcap = ws.cap;
    ws.fips = g_fips;
    ws.wide_max = 0;
    ws.wide_max_k[0] = ws.wide_max_k[1] = ws.wide_max_k[2] = g_wide;
    ws.small_max_k[0] = ws.small_max_k[1] = ws.small_max_k[2] = g_small;
    ws.small_lat_max = g_small;
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
    const size_t stage_bytes = (ws.cap < 2 ? 2 : ws.cap) * seed_stage_bytes(p4);
    uint8_t* stage = (uint8_t*)xalloc(stage_bytes);
    memset(stage, 0, stage_bytes);
    const size_t chunk = check_chunk_items(p, n, ek != nullptr, seed != nullptr, m != nullptr, stage_bytes, ws);
    g_last_chunk = chunk;
    int rc = check_keys_dispatch(nullptr, set, n, ek, dk, seed, m, status, stage, chunk, ws);
    const size_t used = chunk * check_stage_bytes(p, ek != nullptr, seed != nullptr, m != nullptr);
    if (used > stage_bytes) rc = -3;
    memset(stage, 0, used);   // as the C-ABI does after the call
    for (size_t b = 0; b < stage_bytes && rc == 0; b++)
        if (stage[b]) rc = -2;
    free(stage);
    free(ws.A); free(ws.prf); free(ws.leftover); free(ws.resume);
    free(ws.r); free(ws.rho); free(ws.m); free(ws.Kp); free(ws.Kbar);
    return rc;
}
size_t emu_check_last_chunk(void) { return g_last_chunk; }
// LDS block(s) of k_check_keys' sponge wave, as recorded by its probe: count, and a copy of the first one's bytes
int emu_check_lds_regions(void) {
    std::lock_guard<std::mutex> lock(g_regions_mu);
    return g_nregions;
}
size_t emu_check_lds_copy(uint8_t* out, size_t max) {
    std::lock_guard<std::mutex> lock(g_regions_mu);
    if (g_nregions == 0) return 0;
    const size_t b = g_regions[0].bytes < max ? g_regions[0].bytes : max;
    memcpy(out, g_regions[0].p, b);
    return b;
}
void emu_check_lds_reset(void) {
    std::lock_guard<std::mutex> lock(g_regions_mu);
    g_nregions = 0;
}
}
