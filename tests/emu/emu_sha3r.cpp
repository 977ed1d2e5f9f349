// tests/emu/emu_sha3r.cpp — TEST INFRASTRUCTURE ONLY: the two kernels of mlkem_sha3r.hpp (k_sha3_ragged: one sponge per lane;
// k_sha3_ragged_w: one sponge per wavefront) compiled for the host wave emulator (hip_emu.hpp), each form forced by the caller.
// Every message load the kernels issue is recorded through the header's MLKEM_EMU_LOAD_PROBE hook and checked after the launch
// against the memory rule of the call: naturally aligned, at most 16 bytes, and holding at least one byte of the item's own head
// or body.  The LDS a kernel reports through MLKEM_EMU_LDS_PROBE (k_sha3_ragged_w: its round-constant table, the only LDS of either form)
// is read back by emu_sha3r_lds_nonzero after the launch (under the emulator __shared__ objects are statics that outlive it).
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

// do [p, p + bytes) and [q, q + len) share a byte?
static bool overlaps(uintptr_t p, size_t bytes, uintptr_t q, size_t len) { return len && p < q + len && q < p + bytes; }

extern "C" {
// form 0: lane-sliced, 1: one sponge per wavefront.  Returns 0, -101 for an argument error (nothing ran), -3 when a recorded load
// breaks the memory rule.
int emu_sha3r(int form, int alg, size_t n, const uint8_t* head, unsigned head_len, size_t head_stride, const uint8_t* body,
              size_t body_bytes, const uint64_t* body_off, const uint32_t* body_len, uint8_t* out, unsigned outlen, size_t out_stride,
              int32_t* status) {
    Sha3rArgs a{n, head, head_len, head_stride, body, body_bytes, body_off, body_len, out, outlen, out_stride, status, 0};
    unsigned rate = 0;
    if (!sha3r_check_args(alg, a, rate)) return -101;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        g_loads.clear();
    }
    g_last_loads = 0;
    if (n == 0) return 0;
    if (sha3_ragged_launch(nullptr, rate, a, form ? (size_t)-1 : 0)) return -101;
    std::lock_guard<std::mutex> lock(g_mu);
    g_last_loads = g_loads.size();
    for (const LoadRec& r : g_loads) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(r.p);
        if (r.item >= n || r.bytes == 0 || r.bytes > 16 || (r.bytes & (r.bytes - 1)) || p % r.bytes) return -3;
        const uint64_t off = body_off[r.item];
        const uint32_t len = body_len[r.item];
        if (off > body_bytes || len > body_bytes - off) return -3;   // an out-of-bounds item loads nothing
        const bool in_head = overlaps(p, r.bytes, reinterpret_cast<uintptr_t>(a.head) + r.item * head_stride, a.head_len);
        const bool in_body = overlaps(p, r.bytes, reinterpret_cast<uintptr_t>(body) + (uintptr_t)off, len);
        if (!in_head && !in_body) return -3;
    }
    return 0;
}
// message loads the last call issued
size_t emu_sha3r_loads(void) { return g_last_loads; }
// LDS regions the kernels have reported (the wave-wide form's round-constant table; the lane-sliced form has no LDS at all), and the
// number of nonzero bytes in them
int emu_sha3r_lds_regions(void) {
    std::lock_guard<std::mutex> lock(g_mu);
    return g_nregions;
}
long emu_sha3r_lds_nonzero(void) {
    std::lock_guard<std::mutex> lock(g_mu);
    long nz = 0;
    for (int i = 0; i < g_nregions; i++)
        for (size_t b = 0; b < g_regions[i].bytes; b++) nz += static_cast<const uint8_t*>(g_regions[i].p)[b] != 0;
    return nz;
}
}
