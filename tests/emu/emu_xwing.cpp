// tests/emu/emu_xwing.cpp — TEST INFRASTRUCTURE ONLY: batched X25519 (mlkem_x25519.hpp) and the X-Wing layer (mlkem_xwing.hpp: the
// expand / combine / row kernels and the sliced KeyGen / Encaps / Decaps sequencing over the product's ML-KEM-768 dispatch functions)
// compiled for the host wave emulator (hip_emu.hpp).  The staging regions live in host memory laid out as a context lays them out;
// they are filled with a pattern before a call and must read zero after it (-2 otherwise).  Two field helpers, which no GPU entry
// point reaches on their own: decode -> canonical encode, and decode, multiply, encode.
#include "hip_emu.hpp"

#include <stddef.h>

#include "../../crystals-kyber_amd/csrc/mlkem_xwing.hpp"

#include <stdlib.h>
#include <string.h>

using namespace mlkem;

static size_t g_cap = 0, g_small = 0, g_rng_wide = 0;

// the field helpers' kernel: out = canonical encoding of the 255 low bits of a, or of a * b
__global__ void __launch_bounds__(WAVE) k_fe_test(size_t n, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint8_t* __restrict__ out) {
    const size_t item = (size_t)blockIdx.x * WAVE + lane_id();
    if (item >= n) return;
    uint32_t wa[8], wb[8], r[8];
    Fe fa, fb, h;
    load32(a, 32, item, wa);
    fe_decode(fa, wa);
    if (b) {
        load32(b, 32, item, wb);
        fe_decode(fb, wb);
        fe_mul(h, fa, fb);
    } else {
        h = fa;
    }
    fe_encode(r, h);
    store32(out, 32, item, r);
}

static void* xalloc(size_t bytes) { return aligned_alloc(64, (bytes + 127) / 64 * 64); }

struct EmuWs {
    Workspace ws;
    explicit EmuWs(size_t n) {
        ws.cap = g_cap ? g_cap : (n ? n : 1);
        ws.hcap = ws.cap;
        ws.fips = 1;   // X-Wing fixes FIPS 203
        ws.wide_max = ws.wide_max_k[0] = ws.wide_max_k[1] = ws.wide_max_k[2] = 0;   // lane-sliced hash kernels (fast under emulation)
        ws.small_max_k[0] = ws.small_max_k[1] = ws.small_max_k[2] = g_small;
        ws.small_lat_max = 256;
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

// the two regions of a context for one call: slice size min(n, cap)
struct EmuStage {
    XwingStage g;
    size_t big_bytes;
    EmuStage(size_t n, size_t cap) {
        ParamSet p;
        (void)param_set(768, p);
        g.items = n < cap ? n : cap;
        g.base = (uint8_t*)xalloc(g.used());
        memset(g.base, 0xA5, g.used());
        big_bytes = g.items * seed_stage_bytes(p);
        g.dk_stage = (uint8_t*)xalloc(big_bytes);
        memset(g.dk_stage, 0xA5, big_bytes);
    }
    // both regions read zero; `big_used`: whether the call staged through dk_stage at all (an untouched region keeps its pattern)
    bool clean(size_t big_used) const {
        for (size_t b = 0; b < g.used(); b++)
            if (g.base[b]) return false;
        for (size_t b = 0; b < big_used; b++)
            if (g.dk_stage[b]) return false;
        return true;
    }
    ~EmuStage() { free(g.base); free(g.dk_stage); }
};

extern "C" {
// cap: slice and chunk capacity (0: the call's n); small_max: as emu_lib.cpp; rng_wide: slices of at most this many items derive with
// one sponge per wavefront
void emu_xwing_config(size_t cap, size_t small_max, size_t rng_wide) { g_cap = cap; g_small = small_max; g_rng_wide = rng_wide; }

// out = canonical encoding of the 255 low bits of a (b == NULL), or of a * b
void emu_fe(size_t n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
    launch("k_fe_test", k_fe_test, ceil_div(n, WAVE), WAVE, nullptr, n, a, b, out);
}

// mlkem_x25519_dev's launch: u == NULL is the base point
void emu_x25519(size_t n, const uint8_t* scalar, const uint8_t* u, uint8_t* out, int32_t* status) {
    x25519_launch(nullptr, n, scalar, 32, u, 32, out, 32, status);
}
// the two multiplications of an Encaps item in one launch
void emu_x25519_pair(size_t n, const uint8_t* scalar, uint8_t* base, const uint8_t* u, uint8_t* out) {
    x25519_pair_launch(nullptr, n, scalar, 32, base, 32, u, 32, out, 32);
}

// the run functions: 0, -1 bad arguments, -2 a staging region did not read zero after the call
int emu_xwing_keygen(size_t n, const uint8_t* sk, uint8_t* pk) {
    if (n == 0) return -1;
    EmuWs w(n);
    EmuStage s(n, w.ws.cap);
    int rc = xwing_keygen_run(nullptr, n, s.g, sk, pk, w.ws);
    if (rc == 0 && !s.clean(s.g.items * 2400)) rc = -2;
    return rc;
}
// eseed == NULL: derived from the generator (root, pos) in domain 0x04
int emu_xwing_encaps(size_t n, const uint8_t* pk, const uint8_t* eseed, const uint8_t* root, uint64_t pos, uint8_t* ct, uint8_t* ss,
                     int32_t* status) {
    if (n == 0 || (!eseed && !root)) return -1;
    EmuWs w(n);
    EmuStage s(n, w.ws.cap);
    RngCall r;
    r.root = root;
    r.pos = pos;
    r.wide_max = g_rng_wide;
    int rc = xwing_encaps_run(nullptr, n, s.g, pk, eseed, eseed ? nullptr : &r, ct, ss, status, w.ws);
    if (rc == 0 && !s.clean(0)) rc = -2;
    return rc;
}
int emu_xwing_decaps(size_t n, const uint8_t* sk, const uint8_t* ct, const uint8_t* pk, uint8_t* ss) {
    if (n == 0) return -1;
    EmuWs w(n);
    EmuStage s(n, w.ws.cap);
    int rc = xwing_decaps_run(nullptr, n, s.g, sk, ct, pk, ss, w.ws);
    if (rc == 0 && !s.clean(n > g_small ? s.big_bytes : 0)) rc = -2;
    return rc;
}
// sk rows of the generator's domain 0x03
void emu_xwing_derive_sk(size_t n, const uint8_t* root, uint64_t pos, uint8_t* sk) {
    xwing_derive_launch(nullptr, false, n, root, pos, sk, nullptr, g_rng_wide);
}
}
