/*
 * mlkem_batch.h — C-ABI of libmlkem_amd.so, the MI355X (gfx950) batched ML-KEM engine.
 *
 * This is the drop-in boundary for the hot path of rsjahnige/CRYSTALS-Kyber: every entry point is
 * `extern "C"`, takes plain pointers + sizes, and names the reference interface it replaces.  All byte
 * strings are PACKED uint8 (one byte per byte — not the reference's 4-byte `union byte`, SURVEY.md F1;
 * the ml_kem.h-compatible shim in mlkem_compat.h widens/narrows at its edge), polynomials are uint16[256]
 * with coefficients in [0, q), item i of a batch lives at base + i * item_size.
 *
 * Results are bit-identical to the reference's ml_kem.c on the same inputs, including its deviations
 * from FIPS 203: PRF and J are SHAKE128 (ml_kem.c:508, :546) and ByteDecode_12 performs no reduction, so
 * the Encaps modulus check never fires (ml_kem.c:170, :1273-1291).
 *
 * Two families:
 *   *_dev : pointers are DEVICE pointers (HBM resident), the work is enqueued on `stream` (a hipStream_t
 *           passed as void*; NULL = default stream) and the call returns without synchronising.
 *           Base pointers must be 16-byte aligned.
 *   plain : pointers are HOST pointers; the call stages through device memory, runs the *_dev path and
 *           synchronises before returning.
 * There is no CPU fallback: without a usable HIP device every call returns MLKEM_ERR_NO_DEVICE.
 *
 * Return value: 0 on success, negative MLKEM_ERR_* otherwise.  Per-item conditions (the reference's
 * ml_errno = -5 hash-check failure) are reported through the `status` array, never through a global.
 */
#ifndef MLKEM_BATCH_H
#define MLKEM_BATCH_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: only the entry points declared here (MLKEM_API) are exported. */
#ifndef MLKEM_API
#define MLKEM_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MLKEM_OK 0
#define MLKEM_ERR_PARAM_SET (-1)    /* unknown parameter set   (reference: ml_errno = -1, ml_kem.c:1389-1391) */
#define MLKEM_ERR_RNG (-2)          /* entropy source failed   (reference: ml_errno = -2, ml_kem.c:1243, :1297) */
#define MLKEM_ERR_LENGTH (-3)       /* ek/dk/c length mismatch (reference: ml_errno = -3, ml_kem.c:1269, :1323, :1331) */
#define MLKEM_ERR_MODULUS (-4)      /* never produced: the reference's check is a no-op (ml_kem.c:1273-1291) */
#define MLKEM_ERR_HASH (-5)         /* per-item status: H(dk.ek) != dk.h (reference: ml_errno = -5, ml_kem.c:1347) */
#define MLKEM_ERR_KEY (-6)          /* a key failed validation: no key set was created (key_status says which and why) */
#define MLKEM_ERR_NO_DEVICE (-100)  /* no HIP device / HIP runtime error */
#define MLKEM_ERR_ARG (-101)        /* NULL or misaligned pointer, bad argument */
#define MLKEM_ERR_ALLOC (-102)      /* device or host allocation failed */

/* Lengths of ek / dk / c for a parameter set in {512, 768, 1024} (ml_kem.h:52-59, ml_kem.c:1363-1395). */
MLKEM_API int mlkem_sizes(int param_set, unsigned* ek_len, unsigned* dk_len, unsigned* c_len);
/* (k, eta1, eta2, du, dv) as the reference's init() fills struct PARAMS (ml_kem.c:1363-1395). */
MLKEM_API int mlkem_params(int param_set, int out_k_eta1_eta2_du_dv[5]);
/* Number of visible HIP devices (0 when none / runtime unusable). */
MLKEM_API int mlkem_device_count(void);
/* Text for an MLKEM_ERR_* code. */
MLKEM_API const char* mlkem_strerror(int code);
/* Last HIP runtime error string seen by this thread's calls ("" if none). */
MLKEM_API const char* mlkem_last_hip_error(void);

/* ---- engine context: owns the scratch HBM of one device --------------------------------------------- */
typedef struct mlkem_ctx mlkem_ctx;
/* `chunk_items` = items per sampler/arithmetic chunk (0 = default 2^18, env MLKEM_CHUNK_ITEMS); scratch is
 * ~10 KiB x chunk_items, allocated once here so that no *_dev call allocates.  A context is bound to `device`: *_dev
 * calls launch on the caller's current HIP device and return MLKEM_ERR_ARG when that is not the context's device.
 * The context gets one side stream with its first encaps / decaps call of at most `chunk_items` items (env
 * MLKEM_SIDE_STREAM=0: never): such a call samples its matrix there while the hash kernels run on the caller's stream; fork and
 * join are events inside the call, so the caller's stream is ordered after all of the call's work exactly as without it
 * (stream capture sees a fork/join).  Contexts that only ever see larger calls create no stream.
 * A context's scratch serves ONE call at a time: queue the *_dev calls of a context on one stream (or order the streams
 * yourself); work that runs side by side on several streams needs a context per stream. */
MLKEM_API int mlkem_ctx_create(mlkem_ctx** out, int device, size_t chunk_items);
MLKEM_API void mlkem_ctx_destroy(mlkem_ctx* ctx);
MLKEM_API size_t mlkem_ctx_scratch_bytes(const mlkem_ctx* ctx);

/* Conformance of a context.  REFERENCE (default): bit-identical to ml_kem.c including its deviations
 * from FIPS 203 (PRF and J on SHAKE128: ml_kem.c:508, :546; modulus check that never fires: :1273-1291).
 * FIPS203: PRF = SHAKE256(s || b), J = SHAKE256(z || c) (FIPS 203 section 4.1) and mlkem_encaps_status_dev reports
 * MLKEM_ERR_MODULUS per item when ByteEncode_12(ByteDecode_12(ek)) != ek (FIPS 203 section 7.2). */
#define MLKEM_CONFORMANCE_REFERENCE 0
#define MLKEM_CONFORMANCE_FIPS203 1
MLKEM_API int mlkem_ctx_set_conformance(mlkem_ctx* ctx, int mode);

/* ---- per-kernel timing (measurement aid used by bench.py) ---------------------------------------------
 * Between begin and end, every kernel launched by this thread is bracketed by HIP events on its launch
 * stream.  mlkem_timing_end synchronises and returns per-kernel-label rows: labels[32*i..] (NUL-terminated),
 * total_ms[i], counts[i]; return value = number of rows (<= max) or a negative error (MLKEM_ERR_NO_DEVICE when an event
 * could not be created or recorded: incomplete rows are not reported). */
/* Measurement aid (tools/energy_probe.py): restrict the batch path of this context's *_dev KEM calls (more than 256 items) to some
 * of its kernel families -- mask bits: 1 = hash kernels, 2 = sampler, 4 = K-PKE.Encrypt, 8 = K-PKE.Decrypt; 15 = all (default).
 * The outputs of a call with stages missing are meaningless; only time and power of the remaining launches are of interest. */
MLKEM_API int mlkem_ctx_debug_stages(mlkem_ctx* ctx, unsigned mask);
MLKEM_API int mlkem_timing_begin(void);
MLKEM_API int mlkem_timing_end(char* labels, double* total_ms, int* counts, int max);

/* ---- batched KEM, device pointers ----------------------------------------------------------------- */
/* replaces KeyGen_internal(params, d, z)          ml_kem.c:1034-1084   (d, z : n x 32 ; ek : n x ek_len ; dk : n x dk_len) */
MLKEM_API int mlkem_keygen_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* d, const uint8_t* z, uint8_t* ek, uint8_t* dk,
                     void* stream);
/* replaces Encaps_internal(params, ek, m)         ml_kem.c:1093-1130   (m : n x 32 ; c : n x c_len ; K : n x 32) */
MLKEM_API int mlkem_encaps_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* ek, const uint8_t* m, uint8_t* c, uint8_t* K,
                     void* stream);
/* mlkem_encaps_dev + the encapsulation-key modulus check of KEM_Encaps (ml_kem.c:1273-1291).  REFERENCE conformance:
 * status[i] = 0 always, because the reference's check cannot fail (F3).  FIPS203 conformance: status[i] = 0, or
 * MLKEM_ERR_MODULUS when a 12-bit coefficient of ek_i is >= q (c_i / K_i are then still written but must be discarded). */
MLKEM_API int mlkem_encaps_status_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* ek, const uint8_t* m, uint8_t* c, uint8_t* K,
                            int32_t* status, void* stream);
/* replaces KEM_Decaps(params, dk, dk_len, c, c_len) ml_kem.c:1310-1359 incl. the dk hash check:
 *   status[i] = 0, or MLKEM_ERR_HASH when H(dk[384k : 768k+32]) != dk[768k+32 : 768k+64]
 *   K[i]      = Decaps_internal(dk_i, c_i) (ml_kem.c:1136-1225) — for status -5 the reference returns NULL;
 *               K[i] then holds the value Decaps_internal would have produced.
 * `status` may be NULL (check skipped = Decaps_internal semantics). */
MLKEM_API int mlkem_decaps_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* dk, const uint8_t* c, uint8_t* K, int32_t* status,
                     void* stream);
/* Decapsulation from the 64-byte SEED FORMAT of the decapsulation key (FIPS 203 §3.3: d || z stored in place of dk):
 *   K_i = Decaps_internal(KeyGen_internal(d_i, z_i).dk, c_i); seed : n x 64 (d || z), c : n x c_len, K : n x 32
 * bit-identical to mlkem_keygen_dev followed by mlkem_decaps_dev (status NULL) on a context of the same conformance mode;
 * no hash check and no status (the expanded dk is consistent by construction); implicit rejection as in Decaps.
 * Calls of at most small_max items (1536 / 768 / 512) are ONE launch, one workgroup per item: the expanded dk, sigma, m', K'
 * and K-bar live in LDS only, and the workgroup zeroes that LDS before it exits.  Larger calls expand the keys chunk by chunk
 * into a staging region the context allocates with its first such call (max(chunk_items, 2) x 4800 bytes: one chunk of ML-KEM-1024, at least two items because mlkem_check_keys_dev shares the region
 * and its legs need up to 8000 bytes for one item),
 * zeroes after every call and frees with the context. */
MLKEM_API int mlkem_decaps_seed_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* seed, const uint8_t* c, uint8_t* K, void* stream);

/* ---- key validation -------------------------------------------------------------------------------------------------
 * Per-item result bits of mlkem_check_keys[_dev]; 0 = every requested check passed.  A bit whose inputs are absent is 0. */
#define MLKEM_KEYCHECK_EK_MODULUS 1   /* ek: a ByteDecode_12 coefficient >= q                              (FIPS 203 §7.2) */
#define MLKEM_KEYCHECK_DK_MODULUS 2   /* the ek embedded in dk: a coefficient >= q                         (FIPS 203 §7.2 on dk.ek) */
#define MLKEM_KEYCHECK_DK_HASH 4      /* H(dk.ek) != dk.h                                                  (FIPS 203 §7.3) */
#define MLKEM_KEYCHECK_EK_MISMATCH 8  /* dk.ek != ek (both given) */
#define MLKEM_KEYCHECK_SEED 16        /* KeyGen_internal(d, z) != (ek, dk) on whichever of ek / dk is given */
#define MLKEM_KEYCHECK_PCT 32         /* Decaps_internal(dk, c) != K for (c, K) = Encaps_internal(ek', m_i) */
/* Batched key validation: ek n x ek_len or NULL, dk n x dk_len or NULL (at least one of them), seed n x 64 (d || z) or NULL, m n x 32
 * or NULL (needs dk), status n x int32 (required).  `seed` requests the seed leg; `m` the pair-wise consistency test, which
 * encapsulates to ek' = ek when given, dk.ek otherwise.  The modulus and hash checks are the FIPS 203 definitions in BOTH
 * conformance modes (H is SHA3-256 either way); mlkem_encaps_dev on a REFERENCE-mode context still accepts a key that fails the
 * modulus check.  The seed and PCT legs use the context's mode (PRF, J): they test consistency with this context's KeyGen / Encaps /
 * Decaps.  The structural check is one launch up to the wave-wide hash limit (the expensive legs are the existing KeyGen / Encaps /
 * Decaps kernels); the legs stage through the context's region of mlkem_decaps_seed_dev (allocated with the first call that needs it,
 * zeroed after every call). */
MLKEM_API int mlkem_check_keys_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* ek, const uint8_t* dk, const uint8_t* seed,
                                   const uint8_t* m, int32_t* status, void* stream);

/* ---- prepared key sets, device pointers -----------------------------------------------------------------------------
 * A key set is validated once and then serves any number of Encaps / Decaps calls whose items name their key by index.  Per key it
 * holds the ek or dk bytes, H(ek) and the k x k matrix A-hat^T (k^2 x 256 uint16): about 7.0 KB per ML-KEM-768 dk key
 * (2400 + 32 + 4608 bytes; device_bytes reports the footprint).  Nothing in it depends on the conformance mode: each call uses
 * its context's mode for J and PRF.
 * Import: exactly one of ek (n_keys x ek_len), dk (n_keys x dk_len) or seed (n_keys x 64, d || z) is non-NULL.  ek / dk imports
 * run the checks of the key-validation call on ek or dk alone (FIPS 203 §7.2 modulus, §7.3 hash, in BOTH conformance modes);
 * key_status (n_keys int32, or NULL) gets exactly the MLKEM_KEYCHECK_* bits that call writes.  If any key fails, the call returns
 * MLKEM_ERR_KEY, leaves *out NULL and frees what it allocated.  A seed import runs KeyGen_internal (in the context's mode) into the
 * set; key_status is then all zero.  The call runs on `stream`, uses the context's scratch and synchronises the stream.
 * Results: for every key a set accepts, c / K are byte-identical to the per-item calls on the gathered keys
 * (mlkem_encaps_dev on ek[key_index[i]], mlkem_decaps_dev on dk[key_index[i]]), implicit rejection included.  The one intended
 * difference: in REFERENCE mode the per-item calls accept ek coefficients >= q (F3); a key set refuses such keys.
 * key_index: n uint32 (device), NULL = key 0 for every item.  An index >= n_keys reads nothing outside the set: the item's c and K
 * are written as zeros and status[i] = MLKEM_ERR_ARG (when status is given); status[i] = 0 for every other item (the checks ran at
 * import, so there is no per-call hash status).  A set made from dk or seed serves Encaps (with the ek embedded in dk) and Decaps;
 * a set made from ek serves Encaps only (Decaps returns MLKEM_ERR_ARG).
 * Lifetime and threading: a set is bound to the device of the context that created it (a call through a context on another
 * device returns MLKEM_ERR_ARG) and is read-only after creation, so any number of contexts and streams on that device may use it
 * at once.  Destroy synchronises the set's device, zeroes every table and frees.  n == 0 is a no-op; n_keys == 0, a NULL set and
 * misaligned pointers are MLKEM_ERR_ARG.  The key-set calls ignore the debug stage mask and always run every stage. */
typedef struct mlkem_keyset mlkem_keyset;
MLKEM_API int mlkem_keyset_create(mlkem_ctx* ctx, int param_set, size_t n_keys, const uint8_t* ek, const uint8_t* dk,
                                  const uint8_t* seed, int32_t* key_status, mlkem_keyset** out, void* stream);
MLKEM_API void mlkem_keyset_destroy(mlkem_keyset* ks);
MLKEM_API int mlkem_keyset_info(const mlkem_keyset* ks, int* param_set, size_t* n_keys, int* has_dk, size_t* device_bytes);
/* item i uses key key_index[i]: m : n x 32 ; c : n x c_len ; K : n x 32 ; status : n int32 or NULL */
MLKEM_API int mlkem_encaps_keyset_dev(mlkem_ctx* ctx, const mlkem_keyset* ks, size_t n, const uint32_t* key_index,
                                      const uint8_t* m, uint8_t* c, uint8_t* K, int32_t* status, void* stream);
MLKEM_API int mlkem_decaps_keyset_dev(mlkem_ctx* ctx, const mlkem_keyset* ks, size_t n, const uint32_t* key_index,
                                      const uint8_t* c, uint8_t* K, int32_t* status, void* stream);

/* ---- randomised KeyGen / Encaps, device pointers: seeds derived on the device -----------------------------------------
 * ML-KEM.KeyGen() and ML-KEM.Encaps(ek) (FIPS 203 algorithms 19, 20) for device-resident batches.  The context owns a generator:
 * a 32-byte root in DEVICE memory (allocated with the first use, never copied back to the host, zeroed and freed with the context)
 * and a 64-bit position on the host that starts at 0 after every (re)seed.  Item randomness is
 *   block(root, dom, pos) = SHAKE256(root[32] || dom[1] || LE64(pos))     (41-byte message, one permutation)
 *   KeyGen item:  d || z = first 64 bytes of block(root, 0x01, pos)
 *   Encaps item:  m      = first 32 bytes of block(root, 0x02, pos)
 * A call of n items uses positions pos .. pos + n - 1 and then sets pos += n, whatever its domain: calls of 5 and 3 items produce
 * exactly the items of one call of 8.  Given the derived seeds every output is byte-identical to the seeded calls
 * (mlkem_keygen_dev, mlkem_encaps_status_dev, mlkem_encaps_keyset_dev) in the context's conformance mode; the derivation itself
 * does not depend on the mode.  d, z and m never exist in host memory or on the bus: they pass through a region of
 * chunk_items x 64 bytes the context allocates with its first random call (larger calls are sliced) and zeroes in stream order
 * before the call returns control of it.  This is a SHAKE256 expansion of the root, not an SP 800-90A DRBG; reseeding is explicit.
 * STREAM CAPTURE: a captured call would replay the same positions and so the same keys; the random calls return MLKEM_ERR_ARG
 * (and launch nothing) when `stream` is capturing.
 * n == 0 is a no-op that leaves the position unchanged.  Without any HIP device a NULL context is MLKEM_ERR_NO_DEVICE.
 *
 * mlkem_ctx_rng_seed: seed != NULL gives a deterministic stream (tests, reproducible key generation, callers with their own
 * approved RBG); seed == NULL draws the root from getrandom(2) (MLKEM_ERR_RNG on failure; the draw comes first).  A random call on a
 * context that was never seeded seeds it from the OS first, with the same error.  The host copy of the root is wiped after the
 * upload.  Ordering: the call SYNCHRONISES THE DEVICE and then copies synchronously, so the new stream starts after all earlier
 * work of the context, whichever stream it was queued on. */
MLKEM_API int mlkem_ctx_rng_seed(mlkem_ctx* ctx, const uint8_t* seed);
/* ek : n x ek_len ; dk : n x dk_len or NULL ; seed_out : n x 64 (d || z, the seed format of mlkem_decaps_seed_dev) or NULL.
 * dk may be NULL only when seed_out is given: the call then returns ek plus seed-format keys; the expanded dk of every slice goes
 * through the staging region of mlkem_decaps_seed_dev, which is zeroed afterwards as it is there. */
MLKEM_API int mlkem_keygen_random_dev(mlkem_ctx* ctx, int param_set, size_t n, uint8_t* ek, uint8_t* dk, uint8_t* seed_out, void* stream);
/* status (n int32, or NULL) as mlkem_encaps_status_dev */
MLKEM_API int mlkem_encaps_random_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* ek, uint8_t* c, uint8_t* K, int32_t* status,
                                      void* stream);
/* key_index and status as mlkem_encaps_keyset_dev: an out-of-range index zeroes the item and still consumes its position */
MLKEM_API int mlkem_encaps_keyset_random_dev(mlkem_ctx* ctx, const mlkem_keyset* ks, size_t n, const uint32_t* key_index, uint8_t* c,
                                             uint8_t* K, int32_t* status, void* stream);

/* ---- batched X25519 and the X-Wing hybrid KEM, device pointers -----------------------------------------------------------
 * X25519 is RFC 7748 section 5: the scalar is clamped, bit 255 of u is ignored, u is taken mod 2^255 - 19 (non-canonical u is
 * accepted), the output is canonical; u == NULL is the base point u = 9.  One item per SIMD lane, constant time: no branch,
 * address or loop bound depends on the scalar or on field data, and both live in registers only.
 *   mlkem_x25519_dev: scalar, u, out : n x 32; status (n int32, or NULL): MLKEM_ERR_LOW_ORDER where out_i is all zero, else 0.
 *
 * X-Wing is ML-KEM-768 + X25519 + a SHA3-256 combiner, as stated here (the draft's own test vectors have not been run):
 *   Label = 5c 2e 2f 2f 5e 5c
 *   expand(sk[32]):  e = SHAKE256(sk, 96);  d = e[0:32], z = e[32:64], sk_X = e[64:96]
 *                    (pk_M, dk_M) = ML-KEM-768.KeyGen_internal(d, z);  pk_X = X25519(sk_X, 9)
 *   KeyGen(sk)            -> pk = pk_M || pk_X                                              (1184 + 32 bytes)
 *   Encaps(pk, eseed[64]) -> (ct_M, ss_M) = ML-KEM-768.Encaps_internal(pk[0:1184], eseed[0:32]); ek_X = eseed[32:64];
 *                            ct_X = X25519(ek_X, 9); ss_X = X25519(ek_X, pk[1184:1216]); ct = ct_M || ct_X   (1088 + 32 bytes)
 *   Decaps(sk, ct)        -> expand(sk); ss_M = ML-KEM-768.Decaps_internal(dk_M, ct[0:1088]); ss_X = X25519(sk_X, ct[1088:1120])
 *   ss = SHA3-256(ss_M || ss_X || ct_X || pk_X || Label)
 * ML-KEM here is always FIPS 203 (PRF and J on SHAKE256), whatever the context's conformance mode; the context may have been
 * created for any parameter set.  There is no all-zero check on ss_X: the combiner binds ct_X and pk_X instead.
 * Rows are the wire formats: sk n x 32, pk n x 1216, ct n x 1120, ss n x 32, eseed n x 64.  d, z, sk_X, m, ss_M, ss_X and the
 * expanded dk_M pass through staging regions the context owns -- its own (2560 bytes x min(chunk_items, 2^18) items, allocated
 * with the first X-Wing call; larger calls are sliced) and, for KeyGen and for Decaps of more than 768 items, the region of
 * mlkem_decaps_seed_dev -- and what a call used of them is zeroed in stream order before the call returns control of them.
 * mlkem_ctx_scratch_bytes does not change.  Conventions as above: base pointers 16-byte aligned, n == 0 is a no-op, MLKEM_ERR_ARG
 * for a NULL or misaligned pointer or a context of another device, MLKEM_ERR_NO_DEVICE for a NULL context without any device;
 * nothing synchronises.
 * STREAM CAPTURE: the seeded calls are pure functions of their inputs, but the first call of a context allocates the staging (and
 * KeyGen / large Decaps the region of mlkem_decaps_seed_dev): capture a call only after an uncaptured call of the same kind and
 * size class has run on the context.  The X-Wing calls stay on the caller's stream (no fork to the side stream).
 *
 * mlkem_xwing_encaps_dev: status (n int32, or NULL): MLKEM_ERR_MODULUS where pk_M fails the FIPS 203 section 7.2 check (ct_i and
 *   ss_i are still written and must be discarded, as with mlkem_encaps_status_dev), else 0.
 * mlkem_xwing_decaps_dev: pk (n x 1216, or NULL) saves the second multiplication: pk_X is read from the last 32 bytes of pk_i
 *   instead of being recomputed from sk_X.  Nothing checks that pk belongs to sk: A WRONG pk GIVES A WRONG SECRET SILENTLY.
 * The random calls extend the generator above with two domains that share its position counter:
 *   X-Wing KeyGen item:  sk    = first 32 bytes of block(root, 0x03, pos)   (written to sk_out: it is the caller's private key)
 *   X-Wing Encaps item:  eseed = first 64 bytes of block(root, 0x04, pos)
 * They advance the position by n, refuse a capturing stream and seed an unseeded context from the OS, as the random calls above. */
#define MLKEM_XWING_SK_BYTES 32
#define MLKEM_XWING_PK_BYTES 1216
#define MLKEM_XWING_CT_BYTES 1120
#define MLKEM_XWING_SS_BYTES 32
#define MLKEM_XWING_ESEED_BYTES 64
#define MLKEM_ERR_LOW_ORDER (-7)   /* per-item status of mlkem_x25519_dev: the output is all zero */
MLKEM_API int mlkem_x25519_dev(mlkem_ctx* ctx, size_t n, const uint8_t* scalar, const uint8_t* u, uint8_t* out, int32_t* status, void* stream);
MLKEM_API int mlkem_xwing_keygen_dev(mlkem_ctx* ctx, size_t n, const uint8_t* sk, uint8_t* pk, void* stream);
MLKEM_API int mlkem_xwing_encaps_dev(mlkem_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* eseed, uint8_t* ct, uint8_t* ss,
                                     int32_t* status, void* stream);
MLKEM_API int mlkem_xwing_decaps_dev(mlkem_ctx* ctx, size_t n, const uint8_t* sk, const uint8_t* ct, const uint8_t* pk, uint8_t* ss,
                                     void* stream);
MLKEM_API int mlkem_xwing_keygen_random_dev(mlkem_ctx* ctx, size_t n, uint8_t* sk_out, uint8_t* pk, void* stream);
MLKEM_API int mlkem_xwing_encaps_random_dev(mlkem_ctx* ctx, size_t n, const uint8_t* pk, uint8_t* ct, uint8_t* ss, int32_t* status,
                                            void* stream);

/* ---- shared-key batches, device pointers ---------------------------------------------------------------------------
 * n encapsulations to ONE encapsulation key / n decapsulations under ONE decapsulation key (a server's long-lived key):
 * the same bytes as mlkem_encaps_dev / mlkem_decaps_dev on n replicated keys, but H(ek), the dk hash check and the
 * k x k matrix are computed once per call instead of per item (35 of 44 / 36 of 51 Keccak-f per item at k = 3).
 * ek : 384k+32 bytes, dk : 768k+96 bytes (one key); m, c, K, status as in the per-item calls. */
MLKEM_API int mlkem_encaps_shared_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* ek, const uint8_t* m, uint8_t* c, uint8_t* K,
                            void* stream);
MLKEM_API int mlkem_decaps_shared_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* dk, const uint8_t* c, uint8_t* K,
                            int32_t* status, void* stream);

/* ---- K-PKE on its own, device pointers -----------------------------------------------------
 * replaces PKE_KeyGen(params, d)          ml_kem.c:651-769  d : n x 32  ->  ek : n x (384k+32), dk_pke : n x 384k
 * replaces PKE_Encrypt(params, ek, m, r)  ml_kem.c:776-936  m, r : n x 32  ->  c : n x 32(du k + dv)
 * replaces PKE_Decrypt(params, dk, c)     ml_kem.c:942-1023 dk_pke : n x 384k  ->  m : n x 32
 * (static in the reference: reached there through KeyGen_internal / Encaps_internal / Decaps_internal) */
MLKEM_API int mlkem_pke_keygen_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* d, uint8_t* ek, uint8_t* dk_pke, void* stream);
MLKEM_API int mlkem_pke_encrypt_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* ek, const uint8_t* m, const uint8_t* r,
                          uint8_t* c, void* stream);
MLKEM_API int mlkem_pke_decrypt_dev(mlkem_ctx* ctx, int param_set, size_t n, const uint8_t* dk_pke, const uint8_t* c, uint8_t* m,
                          void* stream);

/* ---- batched primitives, device pointers (BASELINE config 2 and component parity tests) ------------ */
/* replaces NTT(f)              ml_kem.c:287-329 ; in/out : n x uint16[256].  Inputs are taken mod 2^12 like the reference's
 * `union integer.t`; the result is bit-identical to the reference for EVERY 12-bit input: coefficients in [0, q) (FIPS 203's
 * domain, all the reference's own call sites) give the canonical transform, and coefficients >= q take an exact integer
 * path that reproduces the reference's non-modular step (ml_kem.c:317 stores f[j] - t unreduced), whose outputs can stay
 * >= q (NTT of 4095 x^0 has 4095 at index 254).  f_hat may not alias f partially (equal pointers are fine). */
MLKEM_API int mlkem_ntt_dev(mlkem_ctx* ctx, size_t n, const uint16_t* f, uint16_t* f_hat, void* stream);
/* replaces InverseNTT(fh)      ml_kem.c:336-384 ; coefficients in [0, q).  For coefficients >= q the reference's own result
 * is undefined (ml_kem.c:364-367 overflows a signed int: its -O0 and -O2 builds disagree); this entry then returns the
 * inverse transform of the input reduced mod q. */
MLKEM_API int mlkem_intt_dev(mlkem_ctx* ctx, size_t n, const uint16_t* f_hat, uint16_t* f, void* stream);
/* replaces MultiplyNTTs(f, g)  ml_kem.c:415-442 ; inputs may be any 12-bit value (as ByteDecode_12 yields) */
MLKEM_API int mlkem_multiply_ntts_dev(mlkem_ctx* ctx, size_t n, const uint16_t* f_hat, const uint16_t* g_hat, uint16_t* h_hat, void* stream);
/* replaces VectorMultiply(u, v, k) ml_kem.c:618-638 ; u, v : n x k x uint16[256] (k = 1..4, any 12-bit values),
 * w : n x uint16[256] = sum_i MultiplyNTTs(u[i], v[i]), every partial sum reduced as PolyAddition does */
MLKEM_API int mlkem_vector_multiply_dev(mlkem_ctx* ctx, int k, size_t n, const uint16_t* u, const uint16_t* v, uint16_t* w, void* stream);
/* replaces PolyAddition(u, v) / PolySubtraction(u, v)  ml_kem.c:580-592 / :599-613, coefficient by coefficient over n_values
 * uint16 values (256 per polynomial), inputs taken mod 2^12 like the reference's `union integer.t`:
 *   add: (u + v) % q ;  sub: u < v ? q - (v - u) : u - v, stored into the reference's 12-bit field.  In-place allowed. */
MLKEM_API int mlkem_poly_add_dev(mlkem_ctx* ctx, size_t n_values, const uint16_t* u, const uint16_t* v, uint16_t* z, void* stream);
MLKEM_API int mlkem_poly_sub_dev(mlkem_ctx* ctx, size_t n_values, const uint16_t* u, const uint16_t* v, uint16_t* z, void* stream);
/* replaces ByteEncode(Compress(f, d), d)   ml_kem.c:83-97 + :125-145 ; f : n x uint16[256] -> bytes : n x 32d ;
 *          d in {1, 4, 5, 10, 11} (coefficients taken mod 2^12, then mod q) ; d = 12 : ByteEncode_12 alone (ml_kem.c:736-756) */
MLKEM_API int mlkem_compress_encode_dev(mlkem_ctx* ctx, int d, size_t n, const uint16_t* f, uint8_t* bytes, void* stream);
/* replaces Decompress(ByteDecode(B, d), d) ml_kem.c:153-177 + :104-119 ; d = 12 : the raw 12-bit values, NOT reduced mod q
 *          (ml_kem.c:170) */
MLKEM_API int mlkem_decode_decompress_dev(mlkem_ctx* ctx, int d, size_t n, const uint8_t* bytes, uint16_t* f, void* stream);
/* replaces Compress(x, d) / Decompress(y, d)  ml_kem.c:83-97 / :104-119, value by value, for ANY d in 1..12 and any 12-bit
 * input (taken mod 2^12 like the reference's `union integer.t`; d = 12 is the identity; the rounded quotient wraps at 12
 * bits like the reference's field does).  n uint16 values in, n out; in-place allowed. */
MLKEM_API int mlkem_compress_dev(mlkem_ctx* ctx, int d, size_t n, const uint16_t* x, uint16_t* y, void* stream);
MLKEM_API int mlkem_decompress_dev(mlkem_ctx* ctx, int d, size_t n, const uint16_t* y, uint16_t* x, void* stream);
/* replaces SampleNTT(B)        ml_kem.c:189-245 ; seeds : n x 34 bytes (packed) */
MLKEM_API int mlkem_sample_ntt_dev(mlkem_ctx* ctx, size_t n, const uint8_t* seeds34, uint16_t* a_hat, void* stream);
/* The same with retries[i] (n bytes, may be NULL) = how often the reference's SampleNTT would have incremented B[32] and B[33] of
 * seed i before it succeeded (ml_kem.c:221-242: more than 278 triples consumed; probability < 2^-300 per seed, so always 0 in
 * practice).  a_hat[i] is the polynomial of the seed with bytes 32, 33 advanced by retries[i]; the shim writes the advanced bytes
 * back into the caller's buffer like the reference does. */
MLKEM_API int mlkem_sample_ntt_retries_dev(mlkem_ctx* ctx, size_t n, const uint8_t* seeds34, uint16_t* a_hat, uint8_t* retries, void* stream);
/* replaces SamplePolyCBD(B, eta) ml_kem.c:253-275 ; bytes : n x 64*eta */
MLKEM_API int mlkem_sample_cbd_dev(mlkem_ctx* ctx, int eta, size_t n, const uint8_t* bytes, uint16_t* f, void* stream);
/* replaces PRF(s, b, eta)      ml_kem.c:496-515 (SHAKE128!) ; in : n x 33 bytes (s || b) ; out : n x 64*eta */
MLKEM_API int mlkem_prf_dev(mlkem_ctx* ctx, int eta, size_t n, const uint8_t* in33, uint8_t* out, void* stream);
/* replaces H / G / J           ml_kem.c:521-572 on n equal-length messages; message i starts at
 * msg + i*stride (stride % 8 == 0, stride >= len).  kind: 0 = H (32 B out), 1 = G (64 B), 2 = J (32 B, SHAKE128) */
MLKEM_API int mlkem_hash_dev(mlkem_ctx* ctx, int kind, size_t n, const uint8_t* msg, unsigned len, size_t stride, uint8_t* out, void* stream);

/* replaces Sponge[Keccak-f[1600], pad10*1, r] sha3.c:257-317 on n PRE-PADDED messages of `nblocks` rate blocks each,
 * `outlen` bytes squeezed per message into rows of `out_stride`.  rate in bytes: ANY value 1..199 (the reference's Sponge takes
 * any capacity; byte-aligned ones are served: sha3_b(..., c, ...) with (1600 - c) % 8 == 0).  The five SHA-3 / SHAKE rates
 * 72 / 104 / 136 / 144 / 168 have lane-sliced kernels for large n (out_stride % 4 == 0 there); every other rate, and every call
 * of at most MLKEM_WIDE_HASH_ITEMS messages, runs one sponge per wavefront.  Used by the sha3.h front-ends of the drop-in shim. */
MLKEM_API int mlkem_keccak_sponge_dev(mlkem_ctx* ctx, unsigned rate, size_t n, const uint8_t* padded, unsigned nblocks, uint8_t* out,
                            unsigned outlen, size_t out_stride, void* stream);
/* ---- SHA-3 / SHAKE over device-resident messages of unequal length ---------------------------------------------------
 * Message i = head[i*head_stride .. +head_len) || body[body_off[i] .. +body_len[i]): a fixed-length per-item prefix (typically the
 * K rows an Encaps / Decaps call has just written, or K || H(ek)) followed by a per-item context of its own length.  Padding and
 * the domain suffix are applied on the device: nothing is copied to the host, padded there or aligned.
 * alg: MLKEM_SHA3_224 .. MLKEM_SHAKE256.  outlen must equal the digest length for the four SHA-3 algorithms; the two SHAKEs take
 * any outlen of 1 .. 65536.
 * head: optional, NULL means head_len = 0.  Base and head_stride 8-byte aligned, head_len % 8 == 0, head_stride >= head_len.
 * body: starts at ANY byte address.  body_off (n x uint64) and body_len (n x uint32) are DEVICE arrays; offsets may come in any
 * order, overlap or repeat; a length may be 0; head_len + body_len[i] must be < 2^31.  body may be NULL when body_bytes = 0.
 * Bounds: an item with body_off[i] + body_len[i] > body_bytes (the sum taken without wrapping at 2^64), or one that breaks the
 * 2^31 limit, reads nothing of the body: its out row is written as zeros and status[i] = MLKEM_ERR_ARG when status (n int32, or
 * NULL) is given; every other item gets status[i] = 0 -- the rule mlkem_encaps_keyset_dev has for an index out of range.
 * Memory: message bytes are read with naturally aligned 8-byte loads that each hold at least one byte of the item's own head or
 * body, so a body may end at the last byte of an allocation (and begin at its first).
 * out: 16-byte aligned, out_stride >= outlen, out_stride % 4 == 0; bytes [outlen, out_stride) of every row are left untouched.
 * n == 0 is a no-op.  A bad alg, a bad outlen, bad alignment, or a NULL required pointer (body_off, body_len, out; body when
 * body_bytes > 0) with n > 0 returns MLKEM_ERR_ARG and launches nothing; so does a context on another device.
 * The call uses none of the context's scratch and is a pure function of its inputs: unlike the random calls it may be captured.
 * Calls of at most MLKEM_SHA3_WIDE_ITEMS messages (env; default 4096; mlkem_sha3_ragged_wide_max reads it back) run one sponge per
 * wavefront, larger ones one sponge per SIMD lane.  The limit is the call's own, not the MLKEM_WIDE_HASH_ITEMS of
 * mlkem_keccak_sponge_dev (2048): measured, the two forms cross between 4096 and 8192 messages of 1184 bytes and between 8192 and
 * 16384 short ones (profiles/sha3_ragged.txt).  A wave of the lane-sliced form runs as long as its longest message, and nothing
 * sorts or bins the batch -- callers with very skewed lengths should group messages of similar length into one call.
 * Control flow and addresses depend on lengths and offsets only, never on message bytes: the head may be a secret. */
#define MLKEM_SHA3_224 0   /* rate 144, 28 bytes */
#define MLKEM_SHA3_256 1   /* rate 136, 32 */
#define MLKEM_SHA3_384 2   /* rate 104, 48 */
#define MLKEM_SHA3_512 3   /* rate  72, 64 */
#define MLKEM_SHAKE128 4   /* rate 168, any outlen */
#define MLKEM_SHAKE256 5   /* rate 136, any outlen */
MLKEM_API int mlkem_sha3_ragged_dev(mlkem_ctx* ctx, int alg, size_t n, const uint8_t* head, unsigned head_len, size_t head_stride,
                                    const uint8_t* body, size_t body_bytes, const uint64_t* body_off, const uint32_t* body_len,
                                    uint8_t* out, unsigned outlen, size_t out_stride, int32_t* status, void* stream);
MLKEM_API size_t mlkem_sha3_ragged_wide_max(const mlkem_ctx* ctx);
/* ---- SP 800-185 cSHAKE / KMAC over device-resident messages of unequal length, keyed by device rows in place -------------------
 * The approved keyed constructions on Keccak, for the KDF or MAC a protocol applies to a shared secret (SP 800-56C, SP 800-108):
 *   mlkem_cshake_dev  out[i] = cSHAKE<bits>(X_i, 8 * outlen, N = fname, S = custom); fname = custom = "" is SHAKE<bits>
 *   mlkem_kmac_dev    out[i] = KMAC<bits>(K_i, X_i, 8 * outlen, S = custom), or KMACXOF<bits> (right_encode(0))
 *   X_i = lead || head[i] || body_i.  lead: 0..8 bytes given on the HOST, the same for every item (e.g. the counter 00 00 00 01
 *   of the SP 800-56C one-step KDF in front of the shared secret).  head, body, body_off, body_len, out, status: exactly the
 *   arguments, alignment rules, bounds rule (zero row and status MLKEM_ERR_ARG for an item outside body_bytes or with
 *   lead_len + head_len + body_len[i] >= 2^31) and memory rule of mlkem_sha3_ragged_dev.
 * bits: 128 | 256.  alg: MLKEM_KMAC128 .. MLKEM_KMACXOF256.  outlen: 1 .. 65536.
 * fname (<= 32 bytes) and custom (<= 256 bytes) are HOST pointers to public bytes, read during the call.
 * key, per item (key_stride >= key_len > 0): device rows used in place, base and key_stride 8-byte aligned, key_len % 8 == 0 and
 *   8 .. 128 (typically the K rows of the Encaps / Decaps call before, key_stride 32).
 * key, shared (key_stride == 0): ONE device key of any length 0 .. 512 at any address for all items (e.g. the 164 / 132-byte
 *   default salt of SP 800-56C).
 * The call-uniform prefix (the N / S block and a shared key's blocks) is absorbed once per call by a one-wavefront kernel into a
 * 200-byte midstate region the CONTEXT owns, allocated with the context: no call allocates, every call is a pure function of its
 * inputs and may be captured from the first one on.  After a shared-key call the region is zeroed in stream order.  The region
 * serves one call at a time: calls on one context are made on one stream, or ordered by the caller.
 * The form switch is mlkem_sha3_ragged_dev's (MLKEM_SHA3_WIDE_ITEMS).  Control flow and addresses depend on lengths and offsets
 * only: key, head and body may be secrets.  n == 0 is a no-op; a bad argument returns MLKEM_ERR_ARG and launches nothing. */
#define MLKEM_KMAC128 0
#define MLKEM_KMAC256 1
#define MLKEM_KMACXOF128 2
#define MLKEM_KMACXOF256 3
MLKEM_API int mlkem_cshake_dev(mlkem_ctx* ctx, int bits, size_t n, const uint8_t* fname, unsigned fname_len, const uint8_t* custom,
                               unsigned custom_len, const uint8_t* lead, unsigned lead_len, const uint8_t* head, unsigned head_len,
                               size_t head_stride, const uint8_t* body, size_t body_bytes, const uint64_t* body_off,
                               const uint32_t* body_len, uint8_t* out, unsigned outlen, size_t out_stride, int32_t* status, void* stream);
MLKEM_API int mlkem_kmac_dev(mlkem_ctx* ctx, int alg, size_t n, const uint8_t* key, unsigned key_len, size_t key_stride,
                             const uint8_t* custom, unsigned custom_len, const uint8_t* lead, unsigned lead_len, const uint8_t* head,
                             unsigned head_len, size_t head_stride, const uint8_t* body, size_t body_bytes, const uint64_t* body_off,
                             const uint32_t* body_len, uint8_t* out, unsigned outlen, size_t out_stride, int32_t* status, void* stream);
/* host helper, no device work: message bits (one per byte) + suffix ("01" hash / "1111" XOF: sha3.c:408-436) + pad10*1
 * (sha3.c:226-240) -> whole rate blocks in `padded`; returns the number of blocks or a negative error */
MLKEM_API int mlkem_sha3_pad_bits(const uint8_t* msg_bits, size_t nbits, int xof, unsigned rate, uint8_t* padded, size_t padded_cap);
/* the same with the caller's own suffix bits, appended verbatim as sha3_b does (sha3.c:414-429: two bits sfx[0], sfx[1],
 * or four bits sfx[0..3]; e.g. "11" = RawSHAKE): nsfx in 0..8, bit i of the suffix = sfx_bits[i] & 1 */
MLKEM_API int mlkem_sha3_pad_suffix(const uint8_t* msg_bits, size_t nbits, const uint8_t* sfx_bits, unsigned nsfx, unsigned rate,
                          uint8_t* padded, size_t padded_cap);

/* ---- on-device exhaustive self-test of the exact fp32-pipe arithmetic ---------------------------------------------
 * The kernels evaluate `% q` (ml_kem.c:83-97, :253-275, :287-442) with fp32 FMAs on integers below 2^24.  Sweep `which`
 * (0 .. mlkem_selftest_count() - 1) checks one helper over its WHOLE input domain on the context's device against integer
 * arithmetic (fred: |x| <= 2^24; twiddle products: 258 multipliers x |b| <= 10082; Compress_d: d = 1..11 x |x| <= 4095;
 * CBD eta = 2 / 3: all 2^16 / 2^24 lane inputs; the base-case multiply-accumulate at the corners of its bound;
 * canonicalisation).  Synchronises; *violations == 0 means the property holds on this device and build. */
MLKEM_API int mlkem_selftest_count(void);
MLKEM_API int mlkem_selftest(mlkem_ctx* ctx, int which, unsigned long long* violations);

/* ---- batched KEM, host pointers (stage + run + synchronise) ----------------------------------------
 * These are the streaming front-end below with its default chunking: staging buffers, stream and context are cached
 * between calls (mlkem_stream_release() frees them), so a call allocates nothing after the first. */
MLKEM_API int mlkem_keygen(int param_set, size_t n, const uint8_t* d, const uint8_t* z, uint8_t* ek, uint8_t* dk);
MLKEM_API int mlkem_encaps(int param_set, size_t n, const uint8_t* ek, const uint8_t* m, uint8_t* c, uint8_t* K);
MLKEM_API int mlkem_decaps(int param_set, size_t n, const uint8_t* dk, const uint8_t* c, uint8_t* K, int32_t* status);
/* mlkem_decaps_seed_dev over host pointers */
MLKEM_API int mlkem_decaps_seed(int param_set, size_t n, const uint8_t* seed, const uint8_t* c, uint8_t* K);
/* mlkem_check_keys_dev over host pointers */
MLKEM_API int mlkem_check_keys(int param_set, size_t n, const uint8_t* ek, const uint8_t* dk, const uint8_t* seed, const uint8_t* m,
                               int32_t* status);
MLKEM_API int mlkem_ntt(size_t n, const uint16_t* f, uint16_t* f_hat);
MLKEM_API int mlkem_intt(size_t n, const uint16_t* f_hat, uint16_t* f);
/* SampleNTT (ml_kem.c:189-245) and SamplePolyCBD (ml_kem.c:253-275) over host buffers: n x 34 seed bytes /
 * n x 64*eta bytes -> n x uint16[256].  They back the reference's externally visible primitives in the drop-in shim. */
MLKEM_API int mlkem_sample_ntt(size_t n, const uint8_t* seeds34, uint16_t* a_hat);
MLKEM_API int mlkem_sample_ntt_retries(size_t n, const uint8_t* seeds34, uint16_t* a_hat, uint8_t* retries);
MLKEM_API int mlkem_sample_cbd(int eta, size_t n, const uint8_t* bytes, uint16_t* f);
MLKEM_API int mlkem_keccak_sponge(unsigned rate, size_t n, const uint8_t* padded, unsigned nblocks, uint8_t* out, unsigned outlen);
/* mlkem_sha3_ragged_dev over host pointers: stage, run, synchronise.  Every array is a host array and no pointer needs any
 * alignment (out_stride >= outlen is all an out row needs).  The offsets are validated on the host arrays before anything is
 * staged: the 2^31 limit fails the call with MLKEM_ERR_ARG, an out-of-bounds item gets its zero row and status as above. */
MLKEM_API int mlkem_sha3_ragged(int alg, size_t n, const uint8_t* head, unsigned head_len, size_t head_stride, const uint8_t* body,
                                size_t body_bytes, const uint64_t* body_off, const uint32_t* body_len, uint8_t* out, unsigned outlen,
                                size_t out_stride, int32_t* status);
/* mlkem_cshake_dev / mlkem_kmac_dev over host pointers: stage, run, synchronise, as mlkem_sha3_ragged.  Every array (the key
 * included) is a host array and no pointer needs any alignment; a per-item key still has key_len % 8 == 0, 8 .. 128. */
MLKEM_API int mlkem_cshake(int bits, size_t n, const uint8_t* fname, unsigned fname_len, const uint8_t* custom, unsigned custom_len,
                           const uint8_t* lead, unsigned lead_len, const uint8_t* head, unsigned head_len, size_t head_stride,
                           const uint8_t* body, size_t body_bytes, const uint64_t* body_off, const uint32_t* body_len, uint8_t* out,
                           unsigned outlen, size_t out_stride, int32_t* status);
MLKEM_API int mlkem_kmac(int alg, size_t n, const uint8_t* key, unsigned key_len, size_t key_stride, const uint8_t* custom,
                         unsigned custom_len, const uint8_t* lead, unsigned lead_len, const uint8_t* head, unsigned head_len,
                         size_t head_stride, const uint8_t* body, size_t body_bytes, const uint64_t* body_off, const uint32_t* body_len,
                         uint8_t* out, unsigned outlen, size_t out_stride, int32_t* status);
/* Compress / Decompress (ml_kem.c:83-119) over n host values, any d in 1..12 (reference test Test_Archive/CompressDecompress_test04.c) */
MLKEM_API int mlkem_compress(int d, size_t n, const uint16_t* x, uint16_t* y);
MLKEM_API int mlkem_decompress(int d, size_t n, const uint16_t* y, uint16_t* x);
/* All state the host-pointer calls cache is kept PER DEVICE (the HIP device current in the calling thread): threads that
 * work on different devices share nothing.  mlkem_host_release() zeroes and frees all of it (contexts, streams, pinned and
 * device staging) on every device; mlkem_stream_release() only the streaming engines.  Both may be called from any thread
 * at any time: the cached state is reference-counted, a release waits for calls in flight on the same device's locks, and
 * a call that overlaps a release simply rebuilds (and afterwards frees) what it needs.
 * Threads that call the host-pointer KEM entry points on the SAME device at the same time each get a streaming engine of
 * their own (streams, staging buffers, context; up to 1 + MLKEM_HOST_LANES = 8 per device, further callers queue), so that
 * the one-item calls of a multi-threaded host run side by side on the GPU; the host-pointer primitives (mlkem_ntt, ...)
 * share one context per device and queue.  KEM calls of at most 4 items (the ml_kem.h shim makes calls of one) that arrive
 * while others of the same operation and parameter set are in flight are COMBINED into one launch by whichever caller finds
 * fewer than MLKEM_HOST_COMBINE (default 2; 0: never) batches in flight; a lone caller never waits.  Results and error codes
 * are those of the separate calls. */
MLKEM_API void mlkem_host_release(void);

/* ---- layout converters and streaming front-end --------------------------------------------------
 * The reference stores every byte in a 4-byte `union byte` cell (ml_kem.h:35-38; value in bits 0-7, upper bits
 * undefined).  Device-side converters at memory bandwidth: */
MLKEM_API int mlkem_cells_to_bytes_dev(mlkem_ctx* ctx, size_t n_cells, const uint32_t* cells, uint8_t* bytes, void* stream);
MLKEM_API int mlkem_bytes_to_cells_dev(mlkem_ctx* ctx, size_t n_cells, const uint8_t* bytes, uint32_t* cells, void* stream);
/* Host-resident batches of any size in chunks (chunk_items = 0 -> 2^15, env MLKEM_STREAM_CHUNK_ITEMS): three streams
 * (H2D / kernels / D2H) and three buffer sets ordered by events, so that H2D(i+1), kernels(i) and D2H(i-1) overlap (PCIe is
 * full duplex).  Caller buffers that are pinned (hipHostMalloc, hipHostRegister or mlkem_host_register below) are handed to
 * the DMA engines directly; pageable buffers go through pinned staging with threaded copies.  Same results as the
 * plain host-pointer calls; PCIe-bound. */
MLKEM_API int mlkem_keygen_stream(int param_set, size_t n, const uint8_t* d, const uint8_t* z, uint8_t* ek, uint8_t* dk, size_t chunk_items);
MLKEM_API int mlkem_encaps_stream(int param_set, size_t n, const uint8_t* ek, const uint8_t* m, uint8_t* c, uint8_t* K, size_t chunk_items);
MLKEM_API int mlkem_decaps_stream(int param_set, size_t n, const uint8_t* dk, const uint8_t* c, uint8_t* K, int32_t* status, size_t chunk_items);
/* The streaming calls keep their engine (streams, events, a context, pinned + device staging buffers) cached per device
 * between calls; this zeroes and frees the engines of all devices. */
MLKEM_API void mlkem_stream_release(void);
/* pin / unpin caller memory (hipHostRegister, portable across devices) so that the streaming and *_multi calls skip the
 * staging copy for it */
/* Which operands of the calling thread's last *_stream / host-pointer KEM call were copied through the engine's pinned staging
 * buffers: bit j = span j in argument order (keygen: d z ek dk ; encaps: ek m c K ; decaps: dk c K status); 0 = every operand
 * was handed to the DMA engines in place; -1 before the first call.  Calls of at most 16 KB per operand always copy (cheaper than
 * asking the runtime what kind of memory each pointer is). */
MLKEM_API int mlkem_stream_last_staged(void);
MLKEM_API int mlkem_host_register(void* p, size_t bytes);
MLKEM_API int mlkem_host_unregister(void* p);

/* ---- in-process sharding over several devices (BASELINE configs[4]: 2^23 items over 8 x MI355X) ------------
 * The batch dimension is embarrassingly parallel: an mlkem_multi is a list of MEMBERS, each bound to one HIP device
 * (`devices[r]`; NULL = devices 0 .. n_members-1; n_members = 0 and NULL = every visible device once).  A device may be
 * listed more than once, which is how the sharded path is rehearsed on one GPU.  Member r of R takes the contiguous item
 * range mlkem_shard_range(n, r, R) (item i -> member floor(i / (n/R)), remainder spread over the first members); there is
 * no exchange between members, no collective and no RCCL.  The reference has no counterpart (single-threaded C). */
typedef struct mlkem_multi mlkem_multi;
MLKEM_API int mlkem_multi_create(mlkem_multi** out, int n_members, const int* devices, size_t chunk_items);
MLKEM_API void mlkem_multi_destroy(mlkem_multi* mm);
MLKEM_API int mlkem_multi_members(const mlkem_multi* mm);
MLKEM_API int mlkem_multi_device(const mlkem_multi* mm, int member);
MLKEM_API int mlkem_shard_range(size_t n, int member, int n_members, size_t* start, size_t* stop);
/* host-resident batch (same arguments as the *_stream calls): one host thread per member drives that member's own
 * streaming engine on its device over its item range; returns when all members are done */
MLKEM_API int mlkem_keygen_multi(mlkem_multi* mm, int param_set, size_t n, const uint8_t* d, const uint8_t* z, uint8_t* ek, uint8_t* dk,
                       size_t chunk_items);
MLKEM_API int mlkem_encaps_multi(mlkem_multi* mm, int param_set, size_t n, const uint8_t* ek, const uint8_t* m, uint8_t* c, uint8_t* K,
                       size_t chunk_items);
MLKEM_API int mlkem_decaps_multi(mlkem_multi* mm, int param_set, size_t n, const uint8_t* dk, const uint8_t* c, uint8_t* K, int32_t* status,
                       size_t chunk_items);
/* device-resident shards: arrays of length mlkem_multi_members(); shard r (n_shard[r] items, layout as in the *_dev calls)
 * lives on member r's device.  The work is enqueued on the member's own stream and the call returns without
 * synchronising; the member streams are not ordered after any other stream, so the inputs must be complete when the
 * call is made.  mlkem_multi_sync waits for every member. */
MLKEM_API int mlkem_keygen_multi_dev(mlkem_multi* mm, int param_set, const size_t* n_shard, const uint8_t* const* d, const uint8_t* const* z,
                           uint8_t* const* ek, uint8_t* const* dk);
MLKEM_API int mlkem_encaps_multi_dev(mlkem_multi* mm, int param_set, const size_t* n_shard, const uint8_t* const* ek, const uint8_t* const* m,
                           uint8_t* const* c, uint8_t* const* K);
MLKEM_API int mlkem_decaps_multi_dev(mlkem_multi* mm, int param_set, const size_t* n_shard, const uint8_t* const* dk, const uint8_t* const* c,
                           uint8_t* const* K, int32_t* const* status);
MLKEM_API int mlkem_multi_sync(mlkem_multi* mm);
/* The hipStream_t (as void*) member `member` enqueues its device-resident work on.  A caller orders it after the producers
 * of its inputs (hipStreamWaitEvent on it) and times or consumes the member's work with events recorded on it.  Member
 * streams come from a per-device pool that lives as long as the process: the handle remains a valid stream after
 * mlkem_multi_destroy (which synchronises it and returns it to the pool), so allocator bookkeeping or events that still
 * refer to it stay harmless.  NULL on a bad argument. */
MLKEM_API void* mlkem_multi_stream(mlkem_multi* mm, int member);

/* ---- randomised wrappers: seeds drawn on the host with getrandom(2) ---------------- */
/* replaces KEM_KeyGen(params)  ml_kem.c:1233-1252 for n key pairs */
MLKEM_API int mlkem_keygen_random(int param_set, size_t n, uint8_t* ek, uint8_t* dk);
/* replaces KEM_Encaps(params, ek, ek_len) ml_kem.c:1257-1305 for n encapsulations; ek_len is checked (-3) */
MLKEM_API int mlkem_encaps_random(int param_set, size_t n, const uint8_t* ek, unsigned ek_len, uint8_t* c, uint8_t* K);

#ifdef __cplusplus
}
#endif
#endif
