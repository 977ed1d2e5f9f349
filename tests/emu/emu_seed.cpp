// tests/emu/emu_seed.cpp — TEST INFRASTRUCTURE ONLY: decapsulation from 64-byte seeds (decaps_seed_run: the one-workgroup-per-item
// kernel k_decaps_seed_small and the batch composition) compiled for the host wave emulator (hip_emu.hpp), with the knobs of
// emu_lib.cpp.  It also records where the fused kernel's secret-bearing LDS regions live, so that a test can read them after the
// launch (under the emulator __shared__ objects are statics that outlive it).
#include "hip_emu.hpp"

#include <stddef.h>

#include <mutex>

struct LdsRegion { const void* p; size_t bytes; };
static LdsRegion g_regions[16];
static int g_nregions = 0;
static std::mutex g_regions_mu;
// called by lane 0 of the zeroing wave of every workgroup; the workgroups of a launch run one after another, but the lock keeps
// the record sound whoever calls
static void probe_region(const void* p, size_t bytes) {
    std::lock_guard<std::mutex> lock(g_regions_mu);
    for (int i = 0; i < g_nregions; i++)
        if (g_regions[i].p == p) return;
    if (g_nregions < 16) g_regions[g_nregions++] = {p, bytes};
}
#define MLKEM_EMU_LDS_PROBE(p, bytes) probe_region((p), (bytes))

#include "../../crystals-kyber_amd/csrc/mlkem_pipeline.hpp"

#include <stdlib.h>

using namespace mlkem;

static size_t g_cap = 0, g_hcap = 0;
static int g_fips = 0;
static size_t g_small = 0, g_small_lat = 256, g_small_wide = 0;

static void* xalloc(size_t bytes) { return aligned_alloc(64, (bytes + 127) / 64 * 64); }

extern "C" {
void emu_seed_config(size_t cap, size_t hcap) { g_cap = cap; g_hcap = hcap; }
void emu_seed_conformance(int fips) { g_fips = fips != 0; }
void emu_seed_small(size_t small_max, size_t small_lat_max, size_t small_wide_max) {
    g_small = small_max; g_small_lat = small_lat_max; g_small_wide = small_wide_max;
}
// K = Decaps_internal(KeyGen_internal(d, z).dk, c) for n items; the staging region holds min(n, cap) items as a context's does
int emu_decaps_seed(int set, size_t n, const uint8_t* seed, const uint8_t* c, uint8_t* K) {
    ParamSet p;
    if (!param_set(set, p)) return -1;
    Workspace ws;
    ws.cap = g_cap ? g_cap : (n ? n : 1);
    ws.hcap = g_hcap ? g_hcap : (n ? n : 1);
    if (ws.hcap < ws.cap) ws.hcap = ws.cap;
    ws.fips = g_fips;
    ws.wide_max = ws.wide_max_k[0] = ws.wide_max_k[1] = ws.wide_max_k[2] = 0;   // lane-sliced hash kernels (fast under emulation)
    ws.small_max_k[0] = ws.small_max_k[1] = ws.small_max_k[2] = g_small;
    ws.small_lat_max = g_small_lat;
    ws.small_wide_max = g_small_wide;
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
    const size_t stage_items = min_sz(ws.cap, n ? n : 1);
    uint8_t* stage = (uint8_t*)xalloc(stage_items * seed_stage_bytes(p));
    const int rc = decaps_seed_dispatch(nullptr, set, n, seed, c, K, stage, stage_items, ws);
    free(stage);
    free(ws.A); free(ws.prf); free(ws.leftover); free(ws.resume);
    free(ws.r); free(ws.rho); free(ws.m); free(ws.Kp); free(ws.Kbar);
    return rc;
}
// secret-bearing LDS regions the fused kernel has zeroed, as recorded by its probe: count, and the number of nonzero bytes in them
int emu_seed_lds_regions(void) {
    std::lock_guard<std::mutex> lock(g_regions_mu);
    return g_nregions;
}
long emu_seed_lds_nonzero(void) {
    std::lock_guard<std::mutex> lock(g_regions_mu);
    long nz = 0;
    for (int i = 0; i < g_nregions; i++)
        for (size_t b = 0; b < g_regions[i].bytes; b++) nz += static_cast<const uint8_t*>(g_regions[i].p)[b] != 0;
    return nz;
}
void emu_seed_lds_reset(void) {
    std::lock_guard<std::mutex> lock(g_regions_mu);
    g_nregions = 0;
}
}
