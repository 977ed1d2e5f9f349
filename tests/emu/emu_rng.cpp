// tests/emu/emu_rng.cpp — TEST INFRASTRUCTURE ONLY: device-side seed derivation (mlkem_rng.hpp: both derivation forms and the sliced
// random KeyGen / Encaps sequencing) compiled for the host wave emulator (hip_emu.hpp), with lowered cap / hcap / small / form
// limits so that every slice loop runs more than once with a short last slice.  The root, the derived-seed region and the dk staging
// region live in host memory laid out as a context lays them out; both regions are filled with a pattern before a call and must read
// zero after it.
#include "hip_emu.hpp"

#include <stddef.h>

#include "../../crystals-kyber_amd/csrc/mlkem_rng.hpp"

#include <stdlib.h>
#include <string.h>

using namespace mlkem;

static size_t g_cap = 0, g_hcap = 0, g_small = 0, g_small_lat = 256, g_rng_wide = 0;
static int g_fips = 0;

static void* xalloc(size_t bytes) { return aligned_alloc(64, (bytes + 127) / 64 * 64); }

struct EmuWs {
    Workspace ws;
    explicit EmuWs(size_t n) {
        ws.cap = g_cap ? g_cap : (n ? n : 1);
        ws.hcap = g_hcap ? g_hcap : ws.cap;
        if (ws.hcap < ws.cap) ws.hcap = ws.cap;
        ws.fips = g_fips;
        ws.wide_max = ws.wide_max_k[0] = ws.wide_max_k[1] = ws.wide_max_k[2] = 0;   // lane-sliced hash kernels (fast under emulation)
        ws.small_max_k[0] = ws.small_max_k[1] = ws.small_max_k[2] = g_small;
        ws.small_lat_max = g_small_lat;
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

// a context's generator state for one call: the root copied to its own "device" buffer, the region sized for a chunk
struct EmuRng {
    RngCall g;
    uint8_t* root;
    size_t region_bytes;
    EmuRng(const uint8_t* root32, uint64_t pos, size_t n, size_t cap) {
        root = (uint8_t*)xalloc(32);
        memcpy(root, root32, 32);
        region_bytes = cap * 64;
        g.root = root;
        g.pos = pos;
        g.seeds = (uint8_t*)xalloc(region_bytes);
        memset(g.seeds, 0xA5, region_bytes);
        g.slice_items = n < cap ? n : cap;
        g.wide_max = g_rng_wide;
    }
    // the part of the region a call of this size may have touched reads zero
    bool clean(size_t bytes_per_item) const {
        for (size_t b = 0; b < g.slice_items * bytes_per_item; b++)
            if (g.seeds[b]) return false;
        return true;
    }
    ~EmuRng() { free(g.seeds); free(root); }
};

extern "C" {
// cap / hcap: chunk and h-chunk capacity (0: the call's n); small / small_lat: as emu_lib.cpp; rng_wide: slices of at most this many
// items derive with one sponge per wavefront
void emu_rng_config(size_t cap, size_t hcap, size_t small_max, size_t small_lat, size_t rng_wide) {
    g_cap = cap; g_hcap = hcap; g_small = small_max; g_small_lat = small_lat; g_rng_wide = rng_wide;
}
void emu_rng_conformance(int fips) { g_fips = fips != 0; }

// the bare derivation: form 0 = lane-sliced, 1 = one sponge per wavefront; keygen: out0 / out1 = d / z rows and seed_out (or NULL),
// otherwise out0 = m rows
void emu_rng_derive(int form, int keygen, size_t n, const uint8_t* root, uint64_t pos, uint8_t* out0, uint8_t* out1, uint8_t* seed_out) {
    rng_derive_launch(nullptr, keygen != 0, n, root, pos, out0, out1, seed_out, form ? (size_t)-1 : 0);
}

// mlkem_keygen_random_dev's sequence: 0, -1 bad arguments, -2 the derived-seed region or the dk staging region did not read zero after
int emu_rng_keygen(int set, size_t n, const uint8_t* root, uint64_t pos, uint8_t* ek, uint8_t* dk, uint8_t* seed_out) {
    ParamSet p;
    if (!param_set(set, p) || n == 0 || (!dk && !seed_out)) return -1;
    EmuWs w(n);
    EmuRng r(root, pos, n, w.ws.cap);
    const size_t stage_bytes = r.g.slice_items * (size_t)p.dk_len;
    uint8_t* stage = (uint8_t*)xalloc(stage_bytes);
    memset(stage, 0xA5, stage_bytes);
    int rc = keygen_random_run(nullptr, p, n, r.g, ek, dk, seed_out, stage, w.ws);
    if (rc == 0 && !r.clean(64)) rc = -2;
    if (rc == 0 && !dk)
        for (size_t b = 0; b < stage_bytes; b++)
            if (stage[b]) { rc = -2; break; }
    free(stage);
    return rc;
}

// mlkem_encaps_random_dev's sequence (status as mlkem_encaps_status_dev: all zero in the reference's mode); -2 as above
int emu_rng_encaps(int set, size_t n, const uint8_t* root, uint64_t pos, const uint8_t* ek, uint8_t* c, uint8_t* K, int32_t* status) {
    ParamSet p;
    if (!param_set(set, p) || n == 0) return -1;
    EmuWs w(n);
    EmuRng r(root, pos, n, w.ws.cap);
    if (status && !g_fips) {
        memset(status, 0, n * sizeof(int32_t));
        status = nullptr;
    }
    int rc = encaps_random_run(nullptr, p, n, r.g, ek, c, K, status, w.ws);
    if (rc == 0 && !r.clean(32)) rc = -2;
    return rc;
}
}
