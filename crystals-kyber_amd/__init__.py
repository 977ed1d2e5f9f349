"""crystals-kyber_amd — Python host side of the MI355X batched ML-KEM engine.

Thin ctypes binding over the C-ABI of libmlkem_amd.so (include/mlkem_batch.h).  PyTorch is used only as
plumbing: device memory (uint8 / int16 CUDA tensors) and the current HIP stream.  The class mirrors the
reference's operator surface for the hot path (rsjahnige/CRYSTALS-Kyber, ml_kem.c):

    KeyGen_internal(d, z)   ml_kem.c:1034      Encaps_internal(ek, m)  ml_kem.c:1093
    KEM_Decaps(dk, c)       ml_kem.c:1310      Decaps_internal(dk, c)  ml_kem.c:1136
    NTT / InverseNTT / MultiplyNTTs / SampleNTT / SamplePolyCBD / PRF / H / G / J

There is NO CPU fallback: importing works anywhere, but constructing `MLKEM` without a HIP device (or
without the built extension) raises.  The directory name contains a hyphen, so import it through
`__graft_entry__.load_package()` (importlib) — the module is registered as `crystals_kyber_amd`.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MLKEM_LIB_PATH") or os.path.join(HERE, "libmlkem_amd.so")   # override: A/B builds in experiments
SHIM_PATH = os.path.join(HERE, "libml_kem.so")

SIZES = {512: (800, 1632, 768), 768: (1184, 2400, 1088), 1024: (1568, 3168, 1568)}  # ek, dk, c (ml_kem.h:52-59)
ERR_RNG = -2                # MLKEM_ERR_RNG: the OS entropy source failed
ERR_MODULUS = -4            # per-item status of encaps in "fips203" conformance: an ek coefficient >= q
ERR_HASH = -5
ERR_KEY = -6                # MLKEM_ERR_KEY: a key failed validation, no key set was created (MLKEMError.key_status says which)
ERR_LOW_ORDER = -7          # MLKEM_ERR_LOW_ORDER: per-item status of MLKEM.x25519, the output is all zero
# X-Wing (ML-KEM-768 + X25519): bytes of sk, pk, ct, ss and of the encapsulation seed (include/mlkem_batch.h)
XWING_SIZES = {"sk": 32, "pk": 1216, "ct": 1120, "ss": 32, "eseed": 64}
ERR_ARG = -101              # MLKEM_ERR_ARG; also the per-item status of a key-set call whose key index is out of range
# per-item result bits of MLKEM.check_keys / mlkem_check_keys[_dev] (include/mlkem_batch.h); 0 = every requested check passed
KEYCHECK_EK_MODULUS = 1     # ek: a ByteDecode_12 coefficient >= q (FIPS 203 §7.2)
KEYCHECK_DK_MODULUS = 2     # the ek embedded in dk: a coefficient >= q
KEYCHECK_DK_HASH = 4        # H(dk.ek) != dk.h (FIPS 203 §7.3)
KEYCHECK_EK_MISMATCH = 8    # dk.ek != ek
KEYCHECK_SEED = 16          # KeyGen_internal(d, z) != (ek, dk)
KEYCHECK_PCT = 32           # pair-wise consistency test failed

# every symbol include/mlkem_batch.h declares (checked by tests/test_abi.py without a GPU)
ABI_SYMBOLS = (
    "mlkem_sizes", "mlkem_params", "mlkem_device_count", "mlkem_strerror", "mlkem_last_hip_error",
    "mlkem_ctx_create", "mlkem_ctx_destroy", "mlkem_ctx_scratch_bytes", "mlkem_timing_begin", "mlkem_timing_end",
    "mlkem_keygen_dev", "mlkem_encaps_dev", "mlkem_decaps_dev", "mlkem_encaps_status_dev", "mlkem_ctx_set_conformance", "mlkem_ctx_debug_stages",
    "mlkem_encaps_shared_dev", "mlkem_decaps_shared_dev",
    "mlkem_pke_keygen_dev", "mlkem_pke_encrypt_dev", "mlkem_pke_decrypt_dev",
    "mlkem_ntt_dev", "mlkem_intt_dev", "mlkem_multiply_ntts_dev", "mlkem_sample_ntt_dev", "mlkem_sample_cbd_dev",
    "mlkem_compress_encode_dev", "mlkem_decode_decompress_dev",
    "mlkem_prf_dev", "mlkem_hash_dev", "mlkem_keccak_sponge_dev", "mlkem_sha3_pad_bits",
    "mlkem_keygen", "mlkem_encaps", "mlkem_decaps", "mlkem_ntt", "mlkem_intt", "mlkem_keccak_sponge",
    "mlkem_sample_ntt", "mlkem_sample_ntt_retries", "mlkem_sample_ntt_retries_dev", "mlkem_sample_cbd",
    "mlkem_keygen_random", "mlkem_encaps_random",
    "mlkem_cells_to_bytes_dev", "mlkem_bytes_to_cells_dev", "mlkem_keygen_stream", "mlkem_encaps_stream", "mlkem_decaps_stream", "mlkem_stream_release",
    "mlkem_compress_dev", "mlkem_decompress_dev", "mlkem_compress", "mlkem_decompress", "mlkem_sha3_pad_suffix",
    "mlkem_selftest_count", "mlkem_selftest", "mlkem_host_release", "mlkem_host_register", "mlkem_host_unregister",
    "mlkem_multi_create", "mlkem_multi_destroy", "mlkem_multi_members", "mlkem_multi_device", "mlkem_shard_range",
    "mlkem_keygen_multi", "mlkem_encaps_multi", "mlkem_decaps_multi",
    "mlkem_keygen_multi_dev", "mlkem_encaps_multi_dev", "mlkem_decaps_multi_dev", "mlkem_multi_sync", "mlkem_multi_stream", "mlkem_stream_last_staged",
    "mlkem_vector_multiply_dev", "mlkem_poly_add_dev", "mlkem_poly_sub_dev",
    "mlkem_decaps_seed_dev", "mlkem_decaps_seed",
    "mlkem_check_keys_dev", "mlkem_check_keys",
    "mlkem_keyset_create", "mlkem_keyset_destroy", "mlkem_keyset_info", "mlkem_encaps_keyset_dev", "mlkem_decaps_keyset_dev",
    "mlkem_ctx_rng_seed", "mlkem_keygen_random_dev", "mlkem_encaps_random_dev", "mlkem_encaps_keyset_random_dev",
    "mlkem_sha3_ragged_dev", "mlkem_sha3_ragged", "mlkem_sha3_ragged_wide_max",
    "mlkem_cshake_dev", "mlkem_kmac_dev", "mlkem_cshake", "mlkem_kmac",
    "mlkem_x25519_dev", "mlkem_xwing_keygen_dev", "mlkem_xwing_encaps_dev", "mlkem_xwing_decaps_dev",
    "mlkem_xwing_keygen_random_dev", "mlkem_xwing_encaps_random_dev",
)
# MLKEM.sha3 / mlkem_sha3_ragged[_dev]: name -> (alg code MLKEM_SHA3_224 .. MLKEM_SHAKE256, rate in bytes, digest bytes; 0 = any outlen)
SHA3_ALGS = {"sha3_224": (0, 144, 28), "sha3_256": (1, 136, 32), "sha3_384": (2, 104, 48), "sha3_512": (3, 72, 64),
             "shake128": (4, 168, 0), "shake256": (5, 136, 0)}
# MLKEM.kmac / mlkem_kmac[_dev]: name -> (alg code MLKEM_KMAC128 .. MLKEM_KMACXOF256, security strength in bits, rate in bytes, XOF)
KMAC_ALGS = {"kmac128": (0, 128, 168, False), "kmac256": (1, 256, 136, False),
             "kmacxof128": (2, 128, 168, True), "kmacxof256": (3, 256, 136, True)}


def pack_messages(msgs):
    """Host helper of MLKEM.sha3: a list of bytes-like objects (bytes, numpy / torch uint8 arrays) -> (buffer uint8, offsets uint64,
    lengths uint32) as numpy arrays, the messages back to back with NO alignment padding."""
    import numpy as np
    raw = []
    for m in msgs:
        if hasattr(m, "detach"):                       # a torch tensor, wherever it lives
            m = m.detach().cpu().contiguous().numpy()
        raw.append(m.tobytes() if hasattr(m, "tobytes") else bytes(m))
    lens = np.array([len(r) for r in raw], np.uint32)
    offs = np.zeros(len(raw), np.uint64)
    if len(raw) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(raw), np.uint8).copy(), offs, lens
SHIM_SYMBOLS = ("init", "KEM_KeyGen", "KEM_Encaps", "KEM_Decaps", "ml_errno", "sha3_b", "sha3_h", "sha3_s", "h2b", "b2h",
                "SampleNTT", "SamplePolyCBD", "NTT", "InverseNTT")


class MLKEMError(RuntimeError):
    def __init__(self, code, msg, key_status=None):
        super().__init__(f"mlkem error {code}: {msg}")
        self.code = code
        self.key_status = key_status   # MLKEM.prepare_keys refusals (code ERR_KEY): the KEYCHECK_* bits per key


_lib = None


def load_library():
    """dlopen libmlkem_amd.so (fails loudly when the HIP extension has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    # torch must load its HIP runtime BEFORE this library is mapped: the process then has exactly one
    # libamdhip64/ROCr instance, shared by torch (allocator, streams) and the engine (measured: the other
    # order leaves the second runtime without a visible device).
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    L.mlkem_strerror.restype = C.c_char_p
    L.mlkem_last_hip_error.restype = C.c_char_p
    L.mlkem_ctx_create.argtypes = [C.POINTER(vp), i32, sz]
    L.mlkem_ctx_destroy.argtypes = [vp]
    L.mlkem_ctx_destroy.restype = None
    L.mlkem_ctx_scratch_bytes.argtypes = [vp]
    L.mlkem_ctx_scratch_bytes.restype = sz
    L.mlkem_keygen_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp]
    L.mlkem_encaps_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp]
    L.mlkem_decaps_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp]
    L.mlkem_decaps_seed_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp]
    L.mlkem_decaps_seed.argtypes = [i32, sz, vp, vp, vp]
    L.mlkem_check_keys_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp, vp]
    L.mlkem_check_keys.argtypes = [i32, sz, vp, vp, vp, vp, vp]
    L.mlkem_keyset_create.argtypes = [vp, i32, sz, vp, vp, vp, vp, C.POINTER(vp), vp]
    L.mlkem_keyset_destroy.argtypes = [vp]
    L.mlkem_keyset_destroy.restype = None
    L.mlkem_keyset_info.argtypes = [vp, C.POINTER(i32), C.POINTER(sz), C.POINTER(i32), C.POINTER(sz)]
    L.mlkem_encaps_keyset_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp]
    L.mlkem_decaps_keyset_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    L.mlkem_ctx_rng_seed.argtypes = [vp, vp]
    L.mlkem_keygen_random_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp]
    L.mlkem_encaps_random_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp]
    L.mlkem_encaps_keyset_random_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    L.mlkem_x25519_dev.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.mlkem_xwing_keygen_dev.argtypes = [vp, sz, vp, vp, vp]
    L.mlkem_xwing_encaps_dev.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp]
    L.mlkem_xwing_decaps_dev.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.mlkem_xwing_keygen_random_dev.argtypes = [vp, sz, vp, vp, vp]
    L.mlkem_xwing_encaps_random_dev.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    L.mlkem_encaps_status_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp, vp]
    L.mlkem_ctx_set_conformance.argtypes = [vp, i32]
    L.mlkem_ctx_debug_stages.argtypes = [vp, C.c_uint]
    L.mlkem_encaps_shared_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp]
    L.mlkem_decaps_shared_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp]
    L.mlkem_pke_keygen_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp]
    L.mlkem_pke_encrypt_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp, vp]
    L.mlkem_pke_decrypt_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp]
    L.mlkem_ntt_dev.argtypes = [vp, sz, vp, vp, vp]
    L.mlkem_intt_dev.argtypes = [vp, sz, vp, vp, vp]
    L.mlkem_multiply_ntts_dev.argtypes = [vp, sz, vp, vp, vp, vp]
    L.mlkem_sample_ntt_dev.argtypes = [vp, sz, vp, vp, vp]
    L.mlkem_sample_cbd_dev.argtypes = [vp, i32, sz, vp, vp, vp]
    L.mlkem_prf_dev.argtypes = [vp, i32, sz, vp, vp, vp]
    L.mlkem_compress_encode_dev.argtypes = [vp, i32, sz, vp, vp, vp]
    L.mlkem_decode_decompress_dev.argtypes = [vp, i32, sz, vp, vp, vp]
    L.mlkem_hash_dev.argtypes = [vp, i32, sz, vp, C.c_uint, sz, vp, vp]
    L.mlkem_keygen.argtypes = [i32, sz, vp, vp, vp, vp]
    L.mlkem_encaps.argtypes = [i32, sz, vp, vp, vp, vp]
    L.mlkem_decaps.argtypes = [i32, sz, vp, vp, vp, vp]
    L.mlkem_ntt.argtypes = [sz, vp, vp]
    L.mlkem_intt.argtypes = [sz, vp, vp]
    L.mlkem_keygen_random.argtypes = [i32, sz, vp, vp]
    L.mlkem_encaps_random.argtypes = [i32, sz, vp, C.c_uint, vp, vp]
    L.mlkem_timing_end.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int), i32]
    L.mlkem_keccak_sponge_dev.argtypes = [vp, C.c_uint, sz, vp, C.c_uint, vp, C.c_uint, sz, vp]
    L.mlkem_keccak_sponge.argtypes = [C.c_uint, sz, vp, C.c_uint, vp, C.c_uint]
    L.mlkem_sha3_ragged_dev.argtypes = [vp, i32, sz, vp, C.c_uint, sz, vp, sz, vp, vp, vp, C.c_uint, sz, vp, vp]
    L.mlkem_sha3_ragged.argtypes = [i32, sz, vp, C.c_uint, sz, vp, sz, vp, vp, vp, C.c_uint, sz, vp]
    L.mlkem_sha3_ragged_wide_max.argtypes = [vp]
    ragged = [vp, C.c_uint, vp, C.c_uint, sz, vp, sz, vp, vp, vp, C.c_uint, sz, vp]   # lead, head, body, offsets, lengths, out, status
    L.mlkem_cshake_dev.argtypes = [vp, i32, sz, vp, C.c_uint, vp, C.c_uint] + ragged + [vp]
    L.mlkem_kmac_dev.argtypes = [vp, i32, sz, vp, C.c_uint, sz, vp, C.c_uint] + ragged + [vp]
    L.mlkem_cshake.argtypes = [i32, sz, vp, C.c_uint, vp, C.c_uint] + ragged
    L.mlkem_kmac.argtypes = [i32, sz, vp, C.c_uint, sz, vp, C.c_uint] + ragged
    L.mlkem_sha3_ragged_wide_max.restype = sz
    L.mlkem_sha3_pad_bits.argtypes = [vp, sz, i32, C.c_uint, vp, sz]
    L.mlkem_cells_to_bytes_dev.argtypes = [vp, sz, vp, vp, vp]
    L.mlkem_bytes_to_cells_dev.argtypes = [vp, sz, vp, vp, vp]
    L.mlkem_keygen_stream.argtypes = [i32, sz, vp, vp, vp, vp, sz]
    L.mlkem_encaps_stream.argtypes = [i32, sz, vp, vp, vp, vp, sz]
    L.mlkem_decaps_stream.argtypes = [i32, sz, vp, vp, vp, vp, sz]
    L.mlkem_compress_dev.argtypes = [vp, i32, sz, vp, vp, vp]
    L.mlkem_decompress_dev.argtypes = [vp, i32, sz, vp, vp, vp]
    L.mlkem_compress.argtypes = [i32, sz, vp, vp]
    L.mlkem_decompress.argtypes = [i32, sz, vp, vp]
    L.mlkem_sha3_pad_suffix.argtypes = [vp, sz, vp, C.c_uint, C.c_uint, vp, sz]
    L.mlkem_selftest.argtypes = [vp, i32, C.POINTER(C.c_ulonglong)]
    L.mlkem_host_release.restype = None
    L.mlkem_stream_release.restype = None
    L.mlkem_host_register.argtypes = [vp, sz]
    L.mlkem_host_unregister.argtypes = [vp]
    L.mlkem_multi_create.argtypes = [C.POINTER(vp), i32, C.POINTER(C.c_int), sz]
    L.mlkem_multi_destroy.argtypes = [vp]
    L.mlkem_multi_destroy.restype = None
    L.mlkem_multi_members.argtypes = [vp]
    L.mlkem_multi_device.argtypes = [vp, i32]
    L.mlkem_shard_range.argtypes = [sz, i32, i32, C.POINTER(sz), C.POINTER(sz)]
    L.mlkem_keygen_multi.argtypes = [vp, i32, sz, vp, vp, vp, vp, sz]
    L.mlkem_encaps_multi.argtypes = [vp, i32, sz, vp, vp, vp, vp, sz]
    L.mlkem_decaps_multi.argtypes = [vp, i32, sz, vp, vp, vp, vp, sz]
    pp = C.POINTER(vp)
    L.mlkem_keygen_multi_dev.argtypes = [vp, i32, C.POINTER(sz), pp, pp, pp, pp]
    L.mlkem_encaps_multi_dev.argtypes = [vp, i32, C.POINTER(sz), pp, pp, pp, pp]
    L.mlkem_decaps_multi_dev.argtypes = [vp, i32, C.POINTER(sz), pp, pp, pp, pp]
    L.mlkem_multi_sync.argtypes = [vp]
    L.mlkem_multi_stream.argtypes = [vp, i32]
    L.mlkem_multi_stream.restype = vp
    L.mlkem_vector_multiply_dev.argtypes = [vp, i32, sz, vp, vp, vp, vp]
    L.mlkem_poly_add_dev.argtypes = [vp, sz, vp, vp, vp, vp]
    L.mlkem_poly_sub_dev.argtypes = [vp, sz, vp, vp, vp, vp]
    _lib = L
    return L


class kernel_timing:
    """Context manager: per-kernel HIP-event timing of everything launched inside (bench.py roofline leg).
    After exit, `.rows` = {label: (total_ms, launches)}."""

    def __enter__(self):
        self.lib = load_library()
        rc = self.lib.mlkem_timing_begin()
        if rc:
            raise MLKEMError(rc, "timing already active")
        self.rows = {}
        return self

    def __exit__(self, *exc):
        labels = C.create_string_buffer(32 * 64)
        ms = (C.c_double * 64)()
        cnt = (C.c_int * 64)()
        n = self.lib.mlkem_timing_end(labels, ms, cnt, 64)
        for i in range(max(n, 0)):
            name = labels.raw[32 * i:32 * i + 32].split(b"\0")[0].decode()
            self.rows[name] = (ms[i], cnt[i])
        return False


def sizes(param_set):
    if param_set not in SIZES:
        raise MLKEMError(-1, "invalid parameter set (reference ml_errno -1, ml_kem.c:1389)")
    return SIZES[param_set]


class MLKEM:
    """One engine context = one device + its scratch HBM.  Work is enqueued on torch's current stream."""

    def __init__(self, param_set=768, device=0, chunk_items=0, conformance="reference"):
        """conformance: "reference" (default; bit-identical to ml_kem.c incl. PRF/J on SHAKE128) or "fips203"
        (PRF/J on SHAKE256, encapsulation-key modulus check reported by `encaps(..., return_status=True)`)."""
        import torch
        self.torch = torch
        self.lib = load_library()
        self.ek_len, self.dk_len, self.c_len = sizes(param_set)
        self.k = (self.ek_len - 32) // 384
        self.param_set = param_set
        if not torch.cuda.is_available():
            raise MLKEMError(-100, "no HIP device visible (the engine has no CPU fallback)")
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        self._check(self.lib.mlkem_ctx_create(C.byref(h), device, chunk_items))
        self._ctx = h
        if conformance not in ("reference", "fips203"):
            raise MLKEMError(-101, "conformance must be 'reference' or 'fips203'")
        self.conformance = conformance
        self._check(self.lib.mlkem_ctx_set_conformance(self._ctx, 1 if conformance == "fips203" else 0))

    def close(self):
        if getattr(self, "_ctx", None):
            self.lib.mlkem_ctx_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    # -- helpers -------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            msg = self.lib.mlkem_strerror(rc).decode()
            hip = self.lib.mlkem_last_hip_error().decode()
            raise MLKEMError(rc, msg + (f" [{hip}]" if hip and rc == -100 else ""))

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, t, dtype, last):
        torch = self.torch
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(t)
        t = t.to(device=self.device, dtype=dtype).contiguous()
        if t.dim() == 1:
            t = t.reshape(-1, last)
        if t.dim() != 2 or t.shape[1] != last:
            raise MLKEMError(-3, f"type check failed: expected rows of {last}, got {tuple(t.shape)} (reference ml_errno -3)")
        return t

    def _out(self, n, last, dtype=None, given=None):
        """A fresh [n, last] output (or [n] when last is None), or the caller's tensor after checking that the raw pointer
        handed to the C-ABI really is n x last elements of `dtype`, contiguous, on this engine's device."""
        torch = self.torch
        dtype = dtype or torch.uint8
        shape = (n,) if last is None else (n, last)
        if given is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if not isinstance(given, torch.Tensor):
            raise MLKEMError(-101, "output must be a torch tensor")
        if given.device != self.device or given.dtype != dtype or tuple(given.shape) != shape or not given.is_contiguous():
            raise MLKEMError(-101, f"output tensor must be contiguous {dtype} {shape} on {self.device}, got "
                                   f"{given.dtype} {tuple(given.shape)} on {given.device}"
                                   f"{'' if given.is_contiguous() else ' (non-contiguous)'}")
        return given

    @property
    def scratch_bytes(self):
        return self.lib.mlkem_ctx_scratch_bytes(self._ctx)

    # -- batched KEM (device resident) -------------------------------------------------------------
    def keygen(self, d, z, ek=None, dk=None):
        """KeyGen_internal (ml_kem.c:1034): d, z [n,32] -> ek [n,ek_len], dk [n,dk_len]."""
        u8 = self.torch.uint8
        d, z = self._dev(d, u8, 32), self._dev(z, u8, 32)
        n = d.shape[0]
        if z.shape[0] != n:
            raise MLKEMError(-101, "d and z batch sizes differ")
        ek = self._out(n, self.ek_len, given=ek)
        dk = self._out(n, self.dk_len, given=dk)
        self._check(self.lib.mlkem_keygen_dev(self._ctx, self.param_set, n, d.data_ptr(), z.data_ptr(), ek.data_ptr(),
                                              dk.data_ptr(), self._stream()))
        return ek, dk

    def encaps(self, ek, m, c=None, K=None, return_status=False):
        """Encaps_internal (ml_kem.c:1093): ek [n,ek_len], m [n,32] -> c [n,c_len], K [n,32]
        (+ status [n]: 0 or -4 = modulus check of KEM_Encaps / FIPS 203 7.2, when return_status)."""
        u8 = self.torch.uint8
        ek, m = self._dev(ek, u8, self.ek_len), self._dev(m, u8, 32)
        n = m.shape[0]
        if ek.shape[0] != n:
            raise MLKEMError(-101, "ek and m batch sizes differ")
        c = self._out(n, self.c_len, given=c)
        K = self._out(n, 32, given=K)
        if return_status:
            st = self.torch.empty(n, dtype=self.torch.int32, device=self.device)
            self._check(self.lib.mlkem_encaps_status_dev(self._ctx, self.param_set, n, ek.data_ptr(), m.data_ptr(), c.data_ptr(),
                                                         K.data_ptr(), st.data_ptr(), self._stream()))
            return c, K, st
        self._check(self.lib.mlkem_encaps_dev(self._ctx, self.param_set, n, ek.data_ptr(), m.data_ptr(), c.data_ptr(),
                                              K.data_ptr(), self._stream()))
        return c, K

    def decaps(self, dk, c, K=None, status=None, hash_check=True):
        """KEM_Decaps (ml_kem.c:1310) incl. the dk hash check: -> K [n,32], status [n] (0 or -5).
        hash_check=False gives Decaps_internal (ml_kem.c:1136) and status None."""
        torch = self.torch
        dk, c = self._dev(dk, torch.uint8, self.dk_len), self._dev(c, torch.uint8, self.c_len)
        n = c.shape[0]
        if dk.shape[0] != n:
            raise MLKEMError(-101, "dk and c batch sizes differ")
        K = self._out(n, 32, given=K)
        if hash_check:
            status = self._out(n, None, torch.int32, given=status)
        sp = status.data_ptr() if hash_check else None
        self._check(self.lib.mlkem_decaps_dev(self._ctx, self.param_set, n, dk.data_ptr(), c.data_ptr(), K.data_ptr(), sp,
                                              self._stream()))
        return K, (status if hash_check else None)

    def decaps_seed(self, seed, c, K=None):
        """Decapsulation from 64-byte seed-format keys (FIPS 203 §3.3): seed [n,64] = d || z, c [n,c_len] -> K [n,32]
        = Decaps_internal(KeyGen_internal(d, z).dk, c), without the expanded dk ever reaching memory the caller sees."""
        torch = self.torch
        seed, c = self._dev(seed, torch.uint8, 64), self._dev(c, torch.uint8, self.c_len)
        n = c.shape[0]
        if seed.shape[0] != n:
            raise MLKEMError(-101, "seed and c batch sizes differ")
        K = self._out(n, 32, given=K)
        self._check(self.lib.mlkem_decaps_seed_dev(self._ctx, self.param_set, n, seed.data_ptr(), c.data_ptr(), K.data_ptr(),
                                                   self._stream()))
        return K

    def check_keys(self, ek=None, dk=None, seed=None, m=None, status=None):
        """Batched key validation: ek [n,ek_len] and / or dk [n,dk_len], optionally seed [n,64] = d || z (seed consistency) and
        m [n,32] (pair-wise consistency test, needs dk) -> int32 status [n] of KEYCHECK_* bits, 0 = every requested check passed.
        The modulus and hash checks follow FIPS 203 in both conformance modes; the seed and PCT legs use this engine's mode."""
        torch = self.torch
        if ek is None and dk is None:
            raise MLKEMError(-101, "check_keys needs ek or dk")
        if m is not None and dk is None:
            raise MLKEMError(-101, "the pair-wise consistency test (m) needs dk")
        args = [None if t is None else self._dev(t, torch.uint8, w)
                for t, w in ((ek, self.ek_len), (dk, self.dk_len), (seed, 64), (m, 32))]
        n = next(t.shape[0] for t in args if t is not None)
        if any(t is not None and t.shape[0] != n for t in args):
            raise MLKEMError(-101, "ek, dk, seed and m batch sizes differ")
        status = self._out(n, None, torch.int32, given=status)
        ptr = [None if t is None else t.data_ptr() for t in args]
        self._check(self.lib.mlkem_check_keys_dev(self._ctx, self.param_set, n, *ptr, status.data_ptr(), self._stream()))
        return status

    def prepare_keys(self, ek=None, dk=None, seed=None):
        """A prepared key set (KeySet) from exactly one of ek [n_keys,ek_len], dk [n_keys,dk_len] or seed [n_keys,64] = d || z:
        validated once (the FIPS 203 modulus and hash checks of check_keys on ek or dk alone), H(ek) and A-hat^T stored on the
        device.  Raises MLKEMError with code ERR_KEY and a `key_status` tensor (KEYCHECK_* bits per key) when any key fails."""
        torch = self.torch
        given = [(t, w) for t, w in ((ek, self.ek_len), (dk, self.dk_len), (seed, 64))]
        if sum(t is not None for t, _ in given) != 1:
            raise MLKEMError(-101, "prepare_keys takes exactly one of ek, dk and seed")
        args = [None if t is None else self._dev(t, torch.uint8, w) for t, w in given]
        n = next(t.shape[0] for t in args if t is not None)
        status = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        h = C.c_void_p()
        ptr = [None if t is None else t.data_ptr() for t in args]
        rc = self.lib.mlkem_keyset_create(self._ctx, self.param_set, n, *ptr, status.data_ptr(), C.byref(h), self._stream())
        if rc == ERR_KEY:
            raise MLKEMError(rc, self.lib.mlkem_strerror(rc).decode(), key_status=status[:n])
        self._check(rc)
        return KeySet(self, h)

    # -- randomised KeyGen / Encaps: seeds derived on the device (mlkem_rng.hpp) -------------------
    def rng_seed(self, seed=None):
        """(Re)seed the engine's generator: 32 bytes give a deterministic stream, None draws the root from the OS.  The position
        restarts at 0.  Synchronises the device.  A random call on an engine that was never seeded seeds it from the OS itself."""
        if seed is None:
            self._check(self.lib.mlkem_ctx_rng_seed(self._ctx, None))
            return
        if isinstance(seed, self.torch.Tensor):
            seed = seed.detach().cpu().numpy()
        if not isinstance(seed, (bytes, bytearray)):
            import numpy as np
            seed = np.ascontiguousarray(seed, np.uint8).tobytes()
        if len(seed) != 32:
            raise MLKEMError(-101, "the generator's seed is 32 bytes")
        buf = (C.c_uint8 * 32).from_buffer_copy(bytes(seed))
        self._check(self.lib.mlkem_ctx_rng_seed(self._ctx, C.addressof(buf)))

    def keygen_random(self, n, return_seed=False, dk=True, ek=None):
        """ML-KEM.KeyGen() for n key pairs: d || z of item i = SHAKE256(root || 0x01 || LE64(pos + i))[:64], derived on the device.
        -> (ek, dk), with return_seed (ek, dk, seed [n,64]); dk=False (needs return_seed) -> (ek, seed): seed-format keys for
        decaps_seed / prepare_keys(seed=...), the expanded dk is never kept.  Not capturable (MLKEMError -101 on a capturing stream)."""
        if not dk and not return_seed:
            raise MLKEMError(-101, "keygen_random(dk=False) needs return_seed=True")
        n = int(n)
        ek = self._out(n, self.ek_len, given=ek)
        dk_t = self._out(n, self.dk_len) if dk else None
        seed = self._out(n, 64) if return_seed else None
        self._check(self.lib.mlkem_keygen_random_dev(self._ctx, self.param_set, n, ek.data_ptr(), None if dk_t is None else dk_t.data_ptr(),
                                                     None if seed is None else seed.data_ptr(), self._stream()))
        return tuple(t for t in (ek, dk_t, seed) if t is not None)

    def encaps_random(self, ek, c=None, K=None, return_status=False):
        """ML-KEM.Encaps(ek): m of item i = SHAKE256(root || 0x02 || LE64(pos + i))[:32], derived on the device.
        ek [n,ek_len] -> c [n,c_len], K [n,32] (+ status [n] as encaps).  Not capturable."""
        ek = self._dev(ek, self.torch.uint8, self.ek_len)
        n = ek.shape[0]
        c = self._out(n, self.c_len, given=c)
        K = self._out(n, 32, given=K)
        st = self.torch.empty(n, dtype=self.torch.int32, device=self.device) if return_status else None
        self._check(self.lib.mlkem_encaps_random_dev(self._ctx, self.param_set, n, ek.data_ptr(), c.data_ptr(), K.data_ptr(),
                                                     None if st is None else st.data_ptr(), self._stream()))
        return (c, K, st) if return_status else (c, K)

    # -- batched X25519 and the X-Wing hybrid KEM (mlkem_x25519.hpp, mlkem_xwing.hpp) ----------------
    def _rows(self, t, last, what):
        """An input of secret or wire rows: as _dev, but a tensor of another dtype or on another device is refused instead of being
        converted or copied (a silent host copy of a secret is what these calls exist to avoid)."""
        torch = self.torch
        if isinstance(t, torch.Tensor) and (t.dtype != torch.uint8 or t.device != self.device):
            raise MLKEMError(ERR_ARG, f"{what} must be a uint8 tensor on {self.device}, got {t.dtype} on {t.device}")
        return self._dev(t, torch.uint8, last)

    def x25519(self, scalar, u=None, return_status=False):
        """X25519 (RFC 7748 section 5): scalar [n,32], u [n,32] or None (the base point u = 9) -> out [n,32], canonical
        (+ status [n] int32 with return_status: ERR_LOW_ORDER where the output is all zero).  Constant time, one item per lane."""
        scalar = self._rows(scalar, 32, "scalar")
        n = scalar.shape[0]
        if u is not None:
            u = self._rows(u, 32, "u")
            if u.shape[0] != n:
                raise MLKEMError(ERR_ARG, "scalar and u batch sizes differ")
        out = self._out(n, 32)
        st = self.torch.empty(n, dtype=self.torch.int32, device=self.device) if return_status else None
        self._check(self.lib.mlkem_x25519_dev(self._ctx, n, scalar.data_ptr(), None if u is None else u.data_ptr(), out.data_ptr(),
                                              None if st is None else st.data_ptr(), self._stream()))
        return (out, st) if return_status else out

    def xwing_keygen(self, sk):
        """X-Wing.KeyGen: sk [n,32] -> pk [n,1216] = pk_M || pk_X.  Works on an engine of any param_set (X-Wing fixes ML-KEM-768 in
        FIPS 203 mode, whatever the engine's conformance)."""
        sk = self._rows(sk, 32, "sk")
        n = sk.shape[0]
        pk = self._out(n, 1216)
        self._check(self.lib.mlkem_xwing_keygen_dev(self._ctx, n, sk.data_ptr(), pk.data_ptr(), self._stream()))
        return pk

    def xwing_encaps(self, pk, eseed, return_status=False):
        """X-Wing.Encaps: pk [n,1216], eseed [n,64] -> ct [n,1120], ss [n,32] (+ status [n] int32 with return_status: ERR_MODULUS
        where pk_M fails the FIPS 203 modulus check; that item's ct and ss are to be discarded)."""
        pk, eseed = self._rows(pk, 1216, "pk"), self._rows(eseed, 64, "eseed")
        n = pk.shape[0]
        if eseed.shape[0] != n:
            raise MLKEMError(ERR_ARG, "pk and eseed batch sizes differ")
        ct, ss = self._out(n, 1120), self._out(n, 32)
        st = self.torch.empty(n, dtype=self.torch.int32, device=self.device) if return_status else None
        self._check(self.lib.mlkem_xwing_encaps_dev(self._ctx, n, pk.data_ptr(), eseed.data_ptr(), ct.data_ptr(), ss.data_ptr(),
                                                    None if st is None else st.data_ptr(), self._stream()))
        return (ct, ss, st) if return_status else (ct, ss)

    def xwing_decaps(self, sk, ct, pk=None):
        """X-Wing.Decaps: sk [n,32], ct [n,1120] -> ss [n,32].  pk [n,1216] (optional) saves the second curve multiplication: pk_X is
        read from its last 32 bytes instead of being recomputed.  A pk that does not belong to sk gives a wrong secret silently."""
        sk, ct = self._rows(sk, 32, "sk"), self._rows(ct, 1120, "ct")
        n = sk.shape[0]
        if pk is not None:
            pk = self._rows(pk, 1216, "pk")
        if ct.shape[0] != n or (pk is not None and pk.shape[0] != n):
            raise MLKEMError(ERR_ARG, "sk, ct and pk batch sizes differ")
        ss = self._out(n, 32)
        self._check(self.lib.mlkem_xwing_decaps_dev(self._ctx, n, sk.data_ptr(), ct.data_ptr(), None if pk is None else pk.data_ptr(),
                                                    ss.data_ptr(), self._stream()))
        return ss

    def xwing_keygen_random(self, n):
        """X-Wing.KeyGen for n fresh keys: sk of item i = SHAKE256(root || 0x03 || LE64(pos + i))[:32], derived on the device
        -> (sk [n,32], pk [n,1216]).  Shares the position counter of keygen_random / encaps_random.  Not capturable."""
        n = int(n)
        sk, pk = self._out(n, 32), self._out(n, 1216)
        self._check(self.lib.mlkem_xwing_keygen_random_dev(self._ctx, n, sk.data_ptr(), pk.data_ptr(), self._stream()))
        return sk, pk

    def xwing_encaps_random(self, pk, return_status=False):
        """X-Wing.Encaps with eseed of item i = SHAKE256(root || 0x04 || LE64(pos + i))[:64], derived on the device:
        pk [n,1216] -> ct [n,1120], ss [n,32] (+ status as xwing_encaps).  Not capturable."""
        pk = self._rows(pk, 1216, "pk")
        n = pk.shape[0]
        ct, ss = self._out(n, 1120), self._out(n, 32)
        st = self.torch.empty(n, dtype=self.torch.int32, device=self.device) if return_status else None
        self._check(self.lib.mlkem_xwing_encaps_random_dev(self._ctx, n, pk.data_ptr(), ct.data_ptr(), ss.data_ptr(),
                                                           None if st is None else st.data_ptr(), self._stream()))
        return (ct, ss, st) if return_status else (ct, ss)

    # reference-style aliases
    KeyGen_internal = keygen
    Encaps_internal = encaps
    KEM_Decaps = decaps

    def Decaps_internal(self, dk, c):
        return self.decaps(dk, c, hash_check=False)[0]

    # -- shared-key batches: one ek / dk for all items ----------------------------------------------
    def encaps_shared(self, ek, m):
        """n encapsulations to ONE key: ek [ek_len] or [1,ek_len], m [n,32] -> c [n,c_len], K [n,32]; same bytes as
        encaps() on the replicated key, H(ek) and the matrix computed once."""
        u8 = self.torch.uint8
        ek = self._dev(self.torch.as_tensor(ek).reshape(1, -1), u8, self.ek_len)
        m = self._dev(m, u8, 32)
        n = m.shape[0]
        c, K = self._out(n, self.c_len), self._out(n, 32)
        self._check(self.lib.mlkem_encaps_shared_dev(self._ctx, self.param_set, n, ek.data_ptr(), m.data_ptr(), c.data_ptr(),
                                                     K.data_ptr(), self._stream()))
        return c, K

    def decaps_shared(self, dk, c, hash_check=True):
        """n decapsulations under ONE key: dk [dk_len] or [1,dk_len], c [n,c_len] -> K [n,32], status [n] (0 / -5)."""
        torch = self.torch
        dk = self._dev(torch.as_tensor(dk).reshape(1, -1), torch.uint8, self.dk_len)
        c = self._dev(c, torch.uint8, self.c_len)
        n = c.shape[0]
        K = self._out(n, 32)
        status = torch.empty(n, dtype=torch.int32, device=self.device) if hash_check else None
        self._check(self.lib.mlkem_decaps_shared_dev(self._ctx, self.param_set, n, dk.data_ptr(), c.data_ptr(), K.data_ptr(),
                                                     status.data_ptr() if hash_check else None, self._stream()))
        return K, status

    # -- K-PKE on its own ---------------------------------------------------
    def PKE_KeyGen(self, d):
        """K-PKE.KeyGen (ml_kem.c:651): d [n,32] -> ek [n,ek_len], dk_pke [n,384k]."""
        d = self._dev(d, self.torch.uint8, 32)
        n = d.shape[0]
        ek, dk = self._out(n, self.ek_len), self._out(n, 384 * self.k)
        self._check(self.lib.mlkem_pke_keygen_dev(self._ctx, self.param_set, n, d.data_ptr(), ek.data_ptr(), dk.data_ptr(), self._stream()))
        return ek, dk

    def PKE_Encrypt(self, ek, m, r):
        """K-PKE.Encrypt (ml_kem.c:776): ek [n,ek_len], m, r [n,32] -> c [n,c_len]."""
        u8 = self.torch.uint8
        ek, m, r = self._dev(ek, u8, self.ek_len), self._dev(m, u8, 32), self._dev(r, u8, 32)
        n = m.shape[0]
        if ek.shape[0] != n or r.shape[0] != n:
            raise MLKEMError(-101, "ek, m and r batch sizes differ")
        c = self._out(n, self.c_len)
        self._check(self.lib.mlkem_pke_encrypt_dev(self._ctx, self.param_set, n, ek.data_ptr(), m.data_ptr(), r.data_ptr(),
                                                   c.data_ptr(), self._stream()))
        return c

    def PKE_Decrypt(self, dk_pke, c):
        """K-PKE.Decrypt (ml_kem.c:942): dk_pke [n,384k], c [n,c_len] -> m [n,32]."""
        u8 = self.torch.uint8
        dk, c = self._dev(dk_pke, u8, 384 * self.k), self._dev(c, u8, self.c_len)
        n = c.shape[0]
        if dk.shape[0] != n:
            raise MLKEMError(-101, "dk_pke and c batch sizes differ")
        m = self._out(n, 32)
        self._check(self.lib.mlkem_pke_decrypt_dev(self._ctx, self.param_set, n, dk.data_ptr(), c.data_ptr(), m.data_ptr(), self._stream()))
        return m

    # -- batched primitives --------------------------------------------------------------------------
    def _poly(self, f):
        torch = self.torch
        if not isinstance(f, torch.Tensor):
            f = torch.as_tensor(f)
        if f.dtype == torch.uint16:
            f = f.view(torch.int16)
        return self._dev(f, torch.int16, 256)

    def ntt(self, f):
        """NTT (ml_kem.c:287): [n,256] coefficients in [0,q) (int16 storage of uint16 values)."""
        f = self._poly(f)
        out = self.torch.empty_like(f)
        self._check(self.lib.mlkem_ntt_dev(self._ctx, f.shape[0], f.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def intt(self, fh):
        """InverseNTT (ml_kem.c:336)."""
        fh = self._poly(fh)
        out = self.torch.empty_like(fh)
        self._check(self.lib.mlkem_intt_dev(self._ctx, fh.shape[0], fh.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def multiply_ntts(self, a, b):
        """MultiplyNTTs (ml_kem.c:415)."""
        a, b = self._poly(a), self._poly(b)
        out = self.torch.empty_like(a)
        self._check(self.lib.mlkem_multiply_ntts_dev(self._ctx, a.shape[0], a.data_ptr(), b.data_ptr(), out.data_ptr(),
                                                     self._stream()))
        return out

    def vector_multiply(self, u, v):
        """VectorMultiply (ml_kem.c:618): u, v [n,k,256] -> [n,256] = sum_i MultiplyNTTs(u[:,i], v[:,i])."""
        torch = self.torch
        u, v = (t.view(torch.int16) if t.dtype == torch.uint16 else t for t in (torch.as_tensor(u), torch.as_tensor(v)))
        u = u.to(device=self.device, dtype=torch.int16).contiguous()
        v = v.to(device=self.device, dtype=torch.int16).contiguous()
        if u.dim() != 3 or u.shape != v.shape or u.shape[2] != 256 or not 1 <= u.shape[1] <= 4:
            raise MLKEMError(-101, f"vector_multiply expects two [n, k, 256] operands with k in 1..4, got {tuple(u.shape)} and {tuple(v.shape)}")
        out = self._out(u.shape[0], 256, torch.int16)
        self._check(self.lib.mlkem_vector_multiply_dev(self._ctx, u.shape[1], u.shape[0], u.data_ptr(), v.data_ptr(), out.data_ptr(),
                                                       self._stream()))
        return out

    def _addsub(self, fn, a, b):
        a, b = self._poly(a), self._poly(b)
        if a.shape != b.shape:
            raise MLKEMError(-101, "operands differ in shape")
        out = self.torch.empty_like(a)
        self._check(fn(self._ctx, a.numel(), a.data_ptr(), b.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def poly_add(self, a, b):
        """PolyAddition (ml_kem.c:580): [n,256] + [n,256] coefficient-wise mod q."""
        return self._addsub(self.lib.mlkem_poly_add_dev, a, b)

    def poly_sub(self, a, b):
        """PolySubtraction (ml_kem.c:599)."""
        return self._addsub(self.lib.mlkem_poly_sub_dev, a, b)

    def sample_ntt(self, seeds34):
        """SampleNTT (ml_kem.c:189): [n,34] -> [n,256]."""
        s = self._dev(seeds34, self.torch.uint8, 34)
        out = self._out(s.shape[0], 256, self.torch.int16)
        self._check(self.lib.mlkem_sample_ntt_dev(self._ctx, s.shape[0], s.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def sample_cbd(self, data, eta):
        """SamplePolyCBD (ml_kem.c:253): [n,64*eta] -> [n,256]."""
        b = self._dev(data, self.torch.uint8, 64 * eta)
        out = self._out(b.shape[0], 256, self.torch.int16)
        self._check(self.lib.mlkem_sample_cbd_dev(self._ctx, eta, b.shape[0], b.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def compress_encode(self, f, d):
        """ByteEncode_d(Compress_d(f)) (ml_kem.c:83, :125) for d in {1,4,5,10,11}; d = 12: ByteEncode_12 of canonical f."""
        f = self._poly(f)
        out = self._out(f.shape[0], 32 * d)
        self._check(self.lib.mlkem_compress_encode_dev(self._ctx, d, f.shape[0], f.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def decode_decompress(self, data, d):
        """Decompress_d(ByteDecode_d(B)) (ml_kem.c:153, :104); d = 12: raw 12-bit values (no reduction, F3)."""
        b = self._dev(data, self.torch.uint8, 32 * d)
        out = self._out(b.shape[0], 256, self.torch.int16)
        self._check(self.lib.mlkem_decode_decompress_dev(self._ctx, d, b.shape[0], b.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def compress(self, x, d):
        """Compress(x, d) (ml_kem.c:83) value by value, any d in 1..12, any 12-bit x: tensor of int16/uint16 -> same shape."""
        return self._compress(x, d, False)

    def decompress(self, y, d):
        """Decompress(y, d) (ml_kem.c:104) value by value, any d in 1..12."""
        return self._compress(y, d, True)

    def _compress(self, v, d, inverse):
        torch = self.torch
        if not isinstance(v, torch.Tensor):
            v = torch.as_tensor(v)
        if v.dtype == torch.uint16:
            v = v.view(torch.int16)
        v = v.to(device=self.device, dtype=torch.int16).contiguous()
        out = torch.empty_like(v)
        fn = self.lib.mlkem_decompress_dev if inverse else self.lib.mlkem_compress_dev
        self._check(fn(self._ctx, int(d), v.numel(), v.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def selftest(self):
        """On-device exhaustive sweeps of the exact fp32-pipe arithmetic (include/mlkem_batch.h: mlkem_selftest);
        returns the list of violation counts, one per sweep (all zero = every helper exact over its whole domain)."""
        self.torch.cuda.synchronize(self.device)
        out = []
        for w in range(self.lib.mlkem_selftest_count()):
            v = C.c_ulonglong(12345)
            self._check(self.lib.mlkem_selftest(self._ctx, w, C.byref(v)))
            out.append(v.value)
        return out

    def prf(self, in33, eta):
        """PRF (ml_kem.c:496; SHAKE128 in the reference): [n,33] (s || b) -> [n,64*eta]."""
        s = self._dev(in33, self.torch.uint8, 33)
        out = self._out(s.shape[0], 64 * eta)
        self._check(self.lib.mlkem_prf_dev(self._ctx, eta, s.shape[0], s.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def _hash(self, kind, msgs, outlen):
        torch = self.torch
        if not isinstance(msgs, torch.Tensor):
            msgs = torch.as_tensor(msgs)
        msgs = msgs.to(device=self.device, dtype=torch.uint8)
        n, ln = msgs.shape
        stride = (ln + 7) // 8 * 8 + 8
        padded = torch.zeros((n, stride), dtype=torch.uint8, device=self.device)
        padded[:, :ln] = msgs
        out = self._out(n, outlen)
        self._check(self.lib.mlkem_hash_dev(self._ctx, kind, n, padded.data_ptr(), ln, stride, out.data_ptr(), self._stream()))
        return out

    def H(self, msgs):
        """H = SHA3-256 (ml_kem.c:521) over equal-length messages [n,len] -> [n,32]."""
        return self._hash(0, msgs, 32)

    def G(self, msgs):
        """G = SHA3-512 (ml_kem.c:559) -> [n,64]."""
        return self._hash(1, msgs, 64)

    def J(self, msgs):
        """J (ml_kem.c:540; SHAKE128 in the reference) -> [n,32]."""
        return self._hash(2, msgs, 32)

    @property
    def sha3_wide_max(self):
        """calls of MLKEM.sha3 with at most this many messages run one sponge per wavefront (env MLKEM_SHA3_WIDE_ITEMS; default 4096)"""
        return self.lib.mlkem_sha3_ragged_wide_max(self._ctx)

    def sha3(self, alg, body, body_off=None, body_len=None, *, head=None, outlen=None, return_status=False):
        """SHA-3 / SHAKE of n messages of unequal length, all on the device: message i = head[i] || body_i (mlkem_sha3_ragged_dev).
        alg: "sha3_224" | "sha3_256" | "sha3_384" | "sha3_512" | "shake128" | "shake256" (the SHAKEs need `outlen`, 1..65536).
        body: a list of bytes / uint8 arrays, packed back to back without padding into one device buffer; or ONE uint8 device tensor
        used in place with `body_off` (n x int64 / uint64) and `body_len` (n x int32 / uint32): offsets in any order, overlapping or
        repeated, lengths of 0 allowed.  head: [n, head_len] uint8 device tensor, head_len % 8 == 0, rows 8-byte aligned; a view with a
        row stride is passed on as it is (e.g. the K of encaps_random: no copy).  -> [n, outlen] uint8 (+ status [n] int32 with
        return_status: MLKEM_ERR_ARG and a zero row for an item whose body lies outside `body`)."""
        torch = self.torch
        if alg not in SHA3_ALGS:
            raise MLKEMError(ERR_ARG, f"unknown SHA-3 algorithm {alg!r}")
        code, _, digest = SHA3_ALGS[alg]
        if outlen is None:
            outlen = digest
        outlen = int(outlen)
        if (digest and outlen != digest) or not 1 <= outlen <= 65536:
            raise MLKEMError(ERR_ARG, f"{alg}: outlen must be {digest or '1..65536'}")
        if isinstance(body, (list, tuple)):
            if body_off is not None or body_len is not None:
                raise MLKEMError(ERR_ARG, "a list of messages carries its own offsets and lengths")
            buf, offs, lens = pack_messages(body)
            body = torch.from_numpy(buf).to(self.device)
            body_off = torch.from_numpy(offs.view("int64")).to(self.device)
            body_len = torch.from_numpy(lens.view("int32")).to(self.device)
        else:
            if not isinstance(body, torch.Tensor) or body.dtype != torch.uint8 or body.device != self.device or not body.is_contiguous():
                raise MLKEMError(ERR_ARG, f"body must be a list or a contiguous uint8 tensor on {self.device}")
            if body_off is None or body_len is None:
                raise MLKEMError(ERR_ARG, "a body tensor needs body_off and body_len")
            body_off = torch.as_tensor(body_off)
            body_len = torch.as_tensor(body_len)
            if body_off.dtype not in (torch.int64, torch.uint64) or body_len.dtype not in (torch.int32, torch.uint32):
                raise MLKEMError(ERR_ARG, "body_off must be 64-bit and body_len 32-bit integers")
            body_off = body_off.to(self.device).contiguous()
            body_len = body_len.to(self.device).contiguous()
        n = body_off.numel()
        if body_len.numel() != n:
            raise MLKEMError(ERR_ARG, "body_off and body_len differ in length")
        head_ptr, head_len, head_stride = None, 0, 0
        if head is not None:
            if (not isinstance(head, torch.Tensor) or head.dtype != torch.uint8 or head.device != self.device or head.dim() != 2
                    or head.shape[0] != n or (head.shape[1] > 1 and head.stride(1) != 1)):
                raise MLKEMError(ERR_ARG, f"head must be a [n, head_len] uint8 tensor on {self.device} with contiguous rows")
            head_ptr, head_len, head_stride = head.data_ptr(), head.shape[1], head.stride(0)
        stride = (outlen + 3) // 4 * 4
        out = torch.empty((n, stride), dtype=torch.uint8, device=self.device)
        st = torch.empty(n, dtype=torch.int32, device=self.device) if return_status else None
        self._check(self.lib.mlkem_sha3_ragged_dev(self._ctx, code, n, head_ptr, head_len, head_stride, body.data_ptr() or None, body.numel(),
                                                   body_off.data_ptr(), body_len.data_ptr(), out.data_ptr(), outlen, stride,
                                                   None if st is None else st.data_ptr(), self._stream()))
        out = out[:, :outlen]
        return (out, st) if return_status else out

    def _ragged_args(self, body, body_off, body_len, head, lead, outlen):
        """the checks and conversions MLKEM.cshake / MLKEM.kmac share with MLKEM.sha3 -> (n, body, body_off, body_len, head triple, lead)"""
        torch = self.torch
        if not 1 <= outlen <= 65536:
            raise MLKEMError(ERR_ARG, "outlen must be 1..65536")
        lead = bytes(lead)
        if len(lead) > 8:
            raise MLKEMError(ERR_ARG, "lead is at most 8 bytes")
        if isinstance(body, (list, tuple)):
            if body_off is not None or body_len is not None:
                raise MLKEMError(ERR_ARG, "a list of messages carries its own offsets and lengths")
            buf, offs, lens = pack_messages(body)
            body = torch.from_numpy(buf).to(self.device)
            body_off = torch.from_numpy(offs.view("int64")).to(self.device)
            body_len = torch.from_numpy(lens.view("int32")).to(self.device)
        else:
            if not isinstance(body, torch.Tensor) or body.dtype != torch.uint8 or body.device != self.device or not body.is_contiguous():
                raise MLKEMError(ERR_ARG, f"body must be a list or a contiguous uint8 tensor on {self.device}")
            if body_off is None or body_len is None:
                raise MLKEMError(ERR_ARG, "a body tensor needs body_off and body_len")
            body_off = torch.as_tensor(body_off)
            body_len = torch.as_tensor(body_len)
            if body_off.dtype not in (torch.int64, torch.uint64) or body_len.dtype not in (torch.int32, torch.uint32):
                raise MLKEMError(ERR_ARG, "body_off must be 64-bit and body_len 32-bit integers")
            body_off = body_off.to(self.device).contiguous()
            body_len = body_len.to(self.device).contiguous()
        n = body_off.numel()
        if body_len.numel() != n:
            raise MLKEMError(ERR_ARG, "body_off and body_len differ in length")
        hd = (None, 0, 0)
        if head is not None:
            if (not isinstance(head, torch.Tensor) or head.dtype != torch.uint8 or head.device != self.device or head.dim() != 2
                    or head.shape[0] != n or (head.shape[1] > 1 and head.stride(1) != 1)):
                raise MLKEMError(ERR_ARG, f"head must be a [n, head_len] uint8 tensor on {self.device} with contiguous rows")
            hd = (head.data_ptr(), head.shape[1], head.stride(0))
        return n, body, body_off, body_len, hd, lead

    def _ragged_call(self, fn, front, n, body, body_off, body_len, hd, lead, outlen, return_status):
        torch = self.torch
        stride = (outlen + 3) // 4 * 4
        out = torch.empty((n, stride), dtype=torch.uint8, device=self.device)
        st = torch.empty(n, dtype=torch.int32, device=self.device) if return_status else None
        self._check(fn(self._ctx, *front, lead or None, len(lead), *hd, body.data_ptr() or None, body.numel(), body_off.data_ptr(),
                       body_len.data_ptr(), out.data_ptr(), outlen, stride, None if st is None else st.data_ptr(), self._stream()))
        out = out[:, :outlen]
        return (out, st) if return_status else out

    def cshake(self, bits, body, body_off=None, body_len=None, *, head=None, lead=b"", outlen, function_name=b"", custom=b"",
               return_status=False):
        """SP 800-185 cSHAKE128 / 256 (bits) of n messages of unequal length, all on the device (mlkem_cshake_dev):
        out[i] = cSHAKE(lead || head[i] || body_i, 8 * outlen, N = function_name, S = custom); N = S = b"" is SHAKE.
        lead: 0..8 host bytes, the same for every item.  body / body_off / body_len / head / return_status: as MLKEM.sha3.
        function_name (<= 32 bytes) and custom (<= 256 bytes) are public host bytes."""
        if bits not in (128, 256):
            raise MLKEMError(ERR_ARG, "bits must be 128 or 256")
        N, S = bytes(function_name), bytes(custom)
        if len(N) > 32 or len(S) > 256:
            raise MLKEMError(ERR_ARG, "function_name is at most 32 bytes and custom at most 256")
        outlen = int(outlen)
        n, body, body_off, body_len, hd, lead = self._ragged_args(body, body_off, body_len, head, lead, outlen)
        return self._ragged_call(self.lib.mlkem_cshake_dev, (bits, n, N or None, len(N), S or None, len(S)), n, body, body_off, body_len, hd,
                                 lead, outlen, return_status)

    def kmac(self, bits, key, body, body_off=None, body_len=None, *, head=None, lead=b"", outlen, custom=b"", xof=False, return_status=False):
        """SP 800-185 KMAC128 / 256 (bits; KMACXOF with xof=True) of n messages of unequal length, all on the device (mlkem_kmac_dev):
        out[i] = KMAC(key_i, lead || head[i] || body_i, 8 * outlen, S = custom).
        key: a [n, key_len] uint8 device tensor USED IN PLACE (key_len % 8 == 0, 8..128, rows 8-byte aligned; a view with a row stride
        is passed on as it is, e.g. the K of encaps_random), or ONE shared key for all items: a 1-D uint8 device tensor or bytes
        (0..512 bytes; bytes are copied to the device).  Everything else as MLKEM.cshake."""
        torch = self.torch
        name = ("kmacxof%d" if xof else "kmac%d") % bits if bits in (128, 256) else None
        if name not in KMAC_ALGS:
            raise MLKEMError(ERR_ARG, "bits must be 128 or 256")
        S = bytes(custom)
        if len(S) > 256:
            raise MLKEMError(ERR_ARG, "custom is at most 256 bytes")
        if isinstance(key, (bytes, bytearray, memoryview)):
            if len(key) > 512:
                raise MLKEMError(ERR_ARG, "a shared key is at most 512 bytes")
            import numpy as np
            key = torch.from_numpy(np.frombuffer(bytes(key), np.uint8).copy()).to(self.device)
        if not isinstance(key, torch.Tensor) or key.dtype != torch.uint8 or key.device != self.device or key.dim() not in (1, 2):
            raise MLKEMError(ERR_ARG, f"key must be bytes or a 1-D / 2-D uint8 tensor on {self.device}")
        outlen = int(outlen)
        n, body, body_off, body_len, hd, lead = self._ragged_args(body, body_off, body_len, head, lead, outlen)
        if key.dim() == 1:
            if key.numel() > 512 or (key.numel() > 1 and key.stride(0) != 1):
                raise MLKEMError(ERR_ARG, "a shared key is a contiguous tensor of at most 512 bytes")
            kd = (key.data_ptr() if key.numel() else None, key.numel(), 0)
        else:
            kl = key.shape[1]
            if key.shape[0] != n or kl % 8 or not 8 <= kl <= 128 or key.stride(1) != 1 or (n > 1 and key.stride(0) < kl):
                raise MLKEMError(ERR_ARG, "per-item keys: [n, key_len] with key_len % 8 == 0, 8..128, and contiguous rows")
            kd = (key.data_ptr(), kl, max(key.stride(0), kl))
        return self._ragged_call(self.lib.mlkem_kmac_dev, (KMAC_ALGS[name][0], n, *kd, S or None, len(S)), n, body, body_off, body_len, hd,
                                 lead, outlen, return_status)

    def kdf_onestep(self, Z, fixed_info, outlen, bits=256, salt=None):
        """SP 800-56C r2 section 4.1, option 3 (H = KMAC#) with H_outputBits = L, i.e. one repetition, all on the device:
        out[i] = KMAC#(salt, 00000001 || Z[i] || FixedInfo_i, 8 * outlen, "KDF").  Z: [n, len] uint8 device tensor used in place as the
        head (len % 8 == 0: the K rows of encaps / decaps); fixed_info: a list of bytes or (body, body_off, body_len) as MLKEM.kmac;
        salt: bytes or a 1-D device tensor, None = the default all-zero salt of 164 (KMAC128) / 132 (KMAC256) bytes."""
        if bits not in (128, 256):
            raise MLKEMError(ERR_ARG, "bits must be 128 or 256")
        if salt is None:
            salt = bytes(164 if bits == 128 else 132)
        in_place = isinstance(fixed_info, tuple) and len(fixed_info) == 3 and isinstance(fixed_info[0], self.torch.Tensor)
        body, off, ln = fixed_info if in_place else (fixed_info, None, None)
        return self.kmac(bits, salt, body, off, ln, head=Z, lead=b"\x00\x00\x00\x01", outlen=outlen, custom=b"KDF")

    def cells_to_bytes(self, cells):
        """`union byte` cells (int32 storage, value in bits 0-7) -> packed uint8, on the device."""
        torch = self.torch
        cells = cells.to(device=self.device).contiguous().view(torch.int32)
        out = torch.empty(cells.numel(), dtype=torch.uint8, device=self.device)
        self._check(self.lib.mlkem_cells_to_bytes_dev(self._ctx, cells.numel(), cells.data_ptr(), out.data_ptr(), self._stream()))
        return out.reshape(cells.shape)

    def bytes_to_cells(self, data):
        torch = self.torch
        data = data.to(device=self.device, dtype=torch.uint8).contiguous()
        out = torch.empty(data.numel(), dtype=torch.int32, device=self.device)
        self._check(self.lib.mlkem_bytes_to_cells_dev(self._ctx, data.numel(), data.data_ptr(), out.data_ptr(), self._stream()))
        return out.reshape(data.shape)

    def sha3_bits(self, bits_list, xof, rate, outlen, suffix=None):
        """SHA-3 / SHAKE of bit-granular messages (sha3_b, sha3.c:408): `bits_list` = equal-length sequences of 0/1;
        suffix + pad10*1 on the host (mlkem_sha3_pad_suffix), sponge on the device.  -> [n, outlen] bytes.
        `suffix`: explicit suffix bits (e.g. (1, 1) = RawSHAKE) instead of the hash "01" / XOF "1111"."""
        import numpy as np
        torch = self.torch
        n = len(bits_list)
        nbits = len(bits_list[0]) if n else 0
        sfx = np.ascontiguousarray(suffix if suffix is not None else ((1, 1, 1, 1) if xof else (0, 1)), np.uint8)
        nblocks = (nbits + sfx.size + 2 + 8 * rate - 1) // (8 * rate)
        padded = np.zeros((n, nblocks * rate), np.uint8)
        for i, b in enumerate(bits_list):
            b = np.ascontiguousarray(b, np.uint8)
            assert b.size == nbits
            rc = self.lib.mlkem_sha3_pad_suffix(b.ctypes.data, nbits, sfx.ctypes.data, sfx.size, rate, padded[i].ctypes.data,
                                                padded[i].size)
            if rc != nblocks:
                raise MLKEMError(rc, "sha3 padding failed")
        dp = torch.from_numpy(padded).to(self.device)
        stride = (outlen + 3) // 4 * 4
        out = torch.zeros((n, stride), dtype=torch.uint8, device=self.device)
        self._check(self.lib.mlkem_keccak_sponge_dev(self._ctx, rate, n, dp.data_ptr(), nblocks, out.data_ptr(), outlen, stride,
                                                     self._stream()))
        return out[:, :outlen]

    # NTT-only workload of BASELINE config 2
    NTT = ntt
    InverseNTT = intt
    MultiplyNTTs = multiply_ntts
    VectorMultiply = vector_multiply
    PolyAddition = poly_add
    PolySubtraction = poly_sub
    SampleNTT = sample_ntt
    SamplePolyCBD = sample_cbd
    PRF = prf


class MLKEMMulti:
    """In-process sharding over several devices (include/mlkem_batch.h: mlkem_multi_*): member r of R works on
    the contiguous item range shard_range(n, r, R) on its own device; no exchange between members, no collective.
    `devices` may repeat a device (rehearsal of the sharded path on one GPU)."""

    def __init__(self, param_set=768, devices=None, chunk_items=0):
        import torch
        self.torch = torch
        self.lib = load_library()
        self.ek_len, self.dk_len, self.c_len = sizes(param_set)
        self.param_set = param_set
        if not torch.cuda.is_available():
            raise MLKEMError(-100, "no HIP device visible (the engine has no CPU fallback)")
        devices = list(range(torch.cuda.device_count())) if devices is None else list(devices)
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = self.lib.mlkem_multi_create(C.byref(h), len(devices), arr, chunk_items)
        if rc:
            raise MLKEMError(rc, self.lib.mlkem_strerror(rc).decode())
        self._mm = h
        self.devices = devices
        self.members = len(devices)

    def close(self):
        if getattr(self, "_mm", None):
            self._ext = None
            self.lib.mlkem_multi_destroy(self._mm)
            self._mm = None

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise MLKEMError(rc, self.lib.mlkem_strerror(rc).decode() + " [" + self.lib.mlkem_last_hip_error().decode() + "]")

    def ranges(self, n):
        return [shard_range(n, r, self.members) for r in range(self.members)]

    # -- host-resident batches (numpy uint8 arrays), one host thread + streaming engine per member --------------------
    def _host(self, a, last):
        import numpy as np
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, last)
        return a

    def keygen(self, d, z, chunk_items=0):
        import numpy as np
        d, z = self._host(d, 32), self._host(z, 32)
        n = d.shape[0]
        ek, dk = np.empty((n, self.ek_len), np.uint8), np.empty((n, self.dk_len), np.uint8)
        self._check(self.lib.mlkem_keygen_multi(self._mm, self.param_set, n, d.ctypes.data, z.ctypes.data, ek.ctypes.data,
                                                dk.ctypes.data, chunk_items))
        return ek, dk

    def encaps(self, ek, m, chunk_items=0):
        import numpy as np
        ek, m = self._host(ek, self.ek_len), self._host(m, 32)
        n = m.shape[0]
        c, K = np.empty((n, self.c_len), np.uint8), np.empty((n, 32), np.uint8)
        self._check(self.lib.mlkem_encaps_multi(self._mm, self.param_set, n, ek.ctypes.data, m.ctypes.data, c.ctypes.data,
                                                K.ctypes.data, chunk_items))
        return c, K

    def decaps(self, dk, c, chunk_items=0):
        import numpy as np
        dk, c = self._host(dk, self.dk_len), self._host(c, self.c_len)
        n = c.shape[0]
        K, st = np.empty((n, 32), np.uint8), np.empty(n, np.int32)
        self._check(self.lib.mlkem_decaps_multi(self._mm, self.param_set, n, dk.ctypes.data, c.ctypes.data, K.ctypes.data,
                                                st.ctypes.data, chunk_items))
        return K, st

    # -- device-resident shards: lists (one tensor per member, on that member's device) ---------------------------------
    def _shards(self, ts, last, dtype=None):
        torch = self.torch
        dtype = dtype or torch.uint8
        if len(ts) != self.members:
            raise MLKEMError(-101, f"need one shard per member ({self.members}), got {len(ts)}")
        for r, t in enumerate(ts):
            want_dev = torch.device("cuda", self.devices[r])
            ok = isinstance(t, torch.Tensor) and t.device == want_dev and t.dtype == dtype and t.is_contiguous() and \
                (t.dim() == 2 and t.shape[1] == last if last is not None else t.dim() == 1)
            if not ok:
                raise MLKEMError(-101, f"shard {r}: expected a contiguous {dtype} tensor [n, {last}] on {want_dev}")
        return (C.c_void_p * self.members)(*[t.data_ptr() for t in ts])

    def _sizes(self, ts, *others):
        ns = [int(t.shape[0]) for t in ts]
        for o in others:
            if [int(t.shape[0]) for t in o] != ns:
                raise MLKEMError(-101, "shard sizes differ between operands")
        return (C.c_size_t * self.members)(*ns), ns

    def _empty(self, ns, last, dtype=None):
        torch = self.torch
        return [torch.empty((n, last) if last is not None else (n,), dtype=dtype or torch.uint8, device=torch.device("cuda", dv))
                for n, dv in zip(ns, self.devices)]

    # Stream discipline of the device-resident calls.  The members enqueue on their own non-blocking streams (C-ABI:
    # mlkem_multi_stream), torch allocates and produces on ITS current stream.  Around every call the wrapper therefore
    #   1. makes each member stream wait for torch's current stream on that device (the producers of the input shards and
    #      whatever last used the memory the caching allocator hands out for the outputs),
    #   2. tells the allocator that inputs and outputs are in use on the member stream (record_stream), so that dropping a
    #      tensor before sync() cannot hand its memory to other work while the member still reads or writes it.
    # Results are ordered for torch by sync() (or by streams()[r] events).
    def streams(self):
        """torch views (ExternalStream) of the members' HIP streams, one per member."""
        torch = self.torch
        if getattr(self, "_ext", None) is None:
            ext = []
            for r, dv in enumerate(self.devices):
                h = self.lib.mlkem_multi_stream(self._mm, r)
                if not h:
                    raise MLKEMError(-100, "member stream unavailable [" + self.lib.mlkem_last_hip_error().decode() + "]")
                ext.append(torch.cuda.ExternalStream(h, device=torch.device("cuda", dv)))
            self._ext = ext
        return self._ext

    def _order(self, *tensor_lists):
        torch = self.torch
        for r, (dv, ext) in enumerate(zip(self.devices, self.streams())):
            ext.wait_stream(torch.cuda.current_stream(torch.device("cuda", dv)))
            for ts in tensor_lists:
                ts[r].record_stream(ext)

    def keygen_dev(self, d, z):
        """shards d[r], z[r] [n_r, 32] on device r -> ek[r], dk[r].  Enqueued on the member streams behind torch's current
        streams; call sync() (or wait on streams()[r]) before reading the outputs from another stream."""
        ns_c, ns = self._sizes(d, z)
        ek, dk = self._empty(ns, self.ek_len), self._empty(ns, self.dk_len)
        pd, pz, pek, pdk = self._shards(d, 32), self._shards(z, 32), self._shards(ek, self.ek_len), self._shards(dk, self.dk_len)
        self._order(d, z, ek, dk)
        self._check(self.lib.mlkem_keygen_multi_dev(self._mm, self.param_set, ns_c, pd, pz, pek, pdk))
        return ek, dk

    def encaps_dev(self, ek, m, c=None, K=None):
        ns_c, ns = self._sizes(m, ek)
        c = self._empty(ns, self.c_len) if c is None else c
        K = self._empty(ns, 32) if K is None else K
        pek, pm, pc, pK = self._shards(ek, self.ek_len), self._shards(m, 32), self._shards(c, self.c_len), self._shards(K, 32)
        self._sizes(m, c, K)
        self._order(ek, m, c, K)
        self._check(self.lib.mlkem_encaps_multi_dev(self._mm, self.param_set, ns_c, pek, pm, pc, pK))
        return c, K

    def decaps_dev(self, dk, c, K=None, status=None):
        ns_c, ns = self._sizes(c, dk)
        K = self._empty(ns, 32) if K is None else K
        st = self._empty(ns, None, self.torch.int32) if status is None else status
        pdk, pc, pK = self._shards(dk, self.dk_len), self._shards(c, self.c_len), self._shards(K, 32)
        pst = self._shards(st, None, self.torch.int32)
        self._sizes(c, K, st)
        self._order(dk, c, K, st)
        self._check(self.lib.mlkem_decaps_multi_dev(self._mm, self.param_set, ns_c, pdk, pc, pK, pst))
        return K, st

    def sync(self):
        self._check(self.lib.mlkem_multi_sync(self._mm))


def shard_range(n_total, rank, world):
    """Contiguous shard of a batch for rank `rank` of `world` (item i -> GPU floor(i / (B/G)));
    the remainder is spread over the first ranks.  Returns (start, stop)."""
    if world <= 0 or not (0 <= rank < world):
        raise ValueError("bad rank/world")
    base, rem = divmod(n_total, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


class KeySet:
    """A prepared key set on an engine's device (mlkem_keyset_*): items of encaps / decaps name their key by index.
    Read-only after creation: any engine (context) of the same parameter set on the same device may use it.  close() (or the
    end of a `with` block, or garbage collection) synchronises the device, zeroes the tables and frees them."""

    def __init__(self, engine, handle):
        self._eng = engine
        self.lib = engine.lib
        self._h = handle
        ps, nk, hd, nb = C.c_int(), C.c_size_t(), C.c_int(), C.c_size_t()
        engine._check(self.lib.mlkem_keyset_info(handle, C.byref(ps), C.byref(nk), C.byref(hd), C.byref(nb)))
        self.param_set, self.n_keys, self.has_dk, self.device_bytes = ps.value, nk.value, bool(hd.value), nb.value

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mlkem_keyset_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _engine(self, engine):
        eng = engine or self._eng
        if not self._h:
            raise MLKEMError(-101, "key set is closed")
        if eng.param_set != self.param_set:
            raise MLKEMError(-101, "engine and key set have different parameter sets")
        return eng

    def _index(self, eng, key_index, n):
        torch = eng.torch
        if key_index is None:
            return None
        t = key_index if isinstance(key_index, torch.Tensor) else torch.as_tensor(key_index)
        if t.dtype not in (torch.int32, torch.uint32):
            raise MLKEMError(-101, "key_index must be an int32 or uint32 tensor")
        t = t.to(device=eng.device).contiguous().reshape(-1)
        if t.shape[0] != n:
            raise MLKEMError(-101, "key_index and the batch have different sizes")
        return t

    def encaps(self, m, key_index=None, c=None, K=None, return_status=False, engine=None):
        """Encaps_internal to key key_index[i] for item i (None: key 0): m [n,32] -> c [n,c_len], K [n,32] (+ int32 status [n]:
        0, or ERR_ARG where the index is out of range -- c and K are then zero)."""
        eng = self._engine(engine)
        torch = eng.torch
        m = eng._dev(m, torch.uint8, 32)
        n = m.shape[0]
        idx = self._index(eng, key_index, n)
        c = eng._out(n, eng.c_len, given=c)
        K = eng._out(n, 32, given=K)
        st = torch.empty(n, dtype=torch.int32, device=eng.device) if return_status else None
        eng._check(self.lib.mlkem_encaps_keyset_dev(eng._ctx, self._h, n, None if idx is None else idx.data_ptr(), m.data_ptr(), c.data_ptr(),
                                                    K.data_ptr(), None if st is None else st.data_ptr(), eng._stream()))
        return (c, K, st) if return_status else (c, K)

    def decaps(self, c, key_index=None, K=None, return_status=False, engine=None):
        """Decaps_internal under key key_index[i] for item i (None: key 0): c [n,c_len] -> K [n,32] (+ int32 status [n]: 0, or
        ERR_ARG where the index is out of range -- K is then zero).  Needs a set made from dk or seed."""
        eng = self._engine(engine)
        torch = eng.torch
        c = eng._dev(c, torch.uint8, eng.c_len)
        n = c.shape[0]
        idx = self._index(eng, key_index, n)
        K = eng._out(n, 32, given=K)
        st = torch.empty(n, dtype=torch.int32, device=eng.device) if return_status else None
        eng._check(self.lib.mlkem_decaps_keyset_dev(eng._ctx, self._h, n, None if idx is None else idx.data_ptr(), c.data_ptr(), K.data_ptr(),
                                                    None if st is None else st.data_ptr(), eng._stream()))
        return (K, st) if return_status else K

    def encaps_random(self, n=None, key_index=None, c=None, K=None, return_status=False, engine=None):
        """ML-KEM.Encaps to key key_index[i] for item i with m derived on the device from the engine's generator (MLKEM.rng_seed):
        n items to key 0, or one item per entry of key_index.  Outputs and status as encaps; an out-of-range index still consumes
        its position of the generator.  Not capturable."""
        eng = self._engine(engine)
        torch = eng.torch
        if n is None:
            if key_index is None:
                raise MLKEMError(-101, "encaps_random needs n or key_index")
            n = int((key_index if isinstance(key_index, torch.Tensor) else torch.as_tensor(key_index)).numel())
        n = int(n)
        idx = self._index(eng, key_index, n)
        c = eng._out(n, eng.c_len, given=c)
        K = eng._out(n, 32, given=K)
        st = torch.empty(n, dtype=torch.int32, device=eng.device) if return_status else None
        eng._check(self.lib.mlkem_encaps_keyset_random_dev(eng._ctx, self._h, n, None if idx is None else idx.data_ptr(), c.data_ptr(),
                                                           K.data_ptr(), None if st is None else st.data_ptr(), eng._stream()))
        return (c, K, st) if return_status else (c, K)
