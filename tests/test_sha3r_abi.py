"""CPU tier: the C-ABI and Python face of SHA-3 / SHAKE over messages of unequal length (mlkem_sha3_ragged_dev,
mlkem_sha3_ragged, mlkem_sha3_ragged_wide_max).  The library exports them and the header declares exactly what is exported; the
algorithm constants are 0..5; the Python table carries the right rates and digest lengths; a list of messages is packed back to back
without padding; and without a device the host-pointer call fails loudly with MLKEM_ERR_NO_DEVICE after its argument checks."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge

MLKEM_ERR_NO_DEVICE, MLKEM_ERR_ARG = -100, -101
SHA3R_SYMBOLS = ("mlkem_sha3_ragged_dev", "mlkem_sha3_ragged")


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def hdr():
    with open(os.path.join(ge.ROOT, "include", "mlkem_batch.h")) as f:
        return f.read()


def test_symbols_exported_and_declared(pkg, hdr):
    lib = C.CDLL(pkg.LIB_PATH)
    for s in SHA3R_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in pkg.ABI_SYMBOLS, s
        assert re.search(r"MLKEM_API int %s\(" % s, hdr), s
    assert hasattr(lib, "mlkem_sha3_ragged_wide_max") and re.search(r"MLKEM_API size_t mlkem_sha3_ragged_wide_max\(", hdr)
    assert hasattr(pkg.MLKEM, "sha3") and hasattr(pkg.MLKEM, "sha3_wide_max")


def test_header_declares_exactly_the_exports(pkg, hdr):
    api = set(re.findall(r"^MLKEM_API [^;(]*?\b(mlkem_[a-z0-9_]+)\(", hdr, re.M))
    assert set(SHA3R_SYMBOLS) <= api
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert names == api, names ^ api
    assert api == set(pkg.ABI_SYMBOLS), api ^ set(pkg.ABI_SYMBOLS)


def test_algorithm_constants_and_python_table(pkg, hdr):
    consts = dict(re.findall(r"^#define (MLKEM_SHA(?:3_\d+|KE\d+)) (\d+)", hdr, re.M))
    assert consts == {"MLKEM_SHA3_224": "0", "MLKEM_SHA3_256": "1", "MLKEM_SHA3_384": "2", "MLKEM_SHA3_512": "3",
                      "MLKEM_SHAKE128": "4", "MLKEM_SHAKE256": "5"}
    assert pkg.SHA3_ALGS == {"sha3_224": (0, 144, 28), "sha3_256": (1, 136, 32), "sha3_384": (2, 104, 48), "sha3_512": (3, 72, 64),
                             "shake128": (4, 168, 0), "shake256": (5, 136, 0)}
    # the table against hashlib's own view of the six functions: rate = 200 - 2 * security strength in bytes
    for name, (code, rate, digest) in pkg.SHA3_ALGS.items():
        h = getattr(hashlib, name.replace("shake", "shake_"))()
        assert h.block_size == rate, name
        if digest:
            assert h.digest_size == digest, name
        assert consts["MLKEM_" + name.upper()] == str(code)


def test_pack_messages_no_padding(pkg):
    msgs = [b"abc", b"", bytes(range(9)), np.arange(5, dtype=np.uint8), b"x" * 137, b""]
    buf, offs, lens = pkg.pack_messages(msgs)
    assert buf.dtype == np.uint8 and offs.dtype == np.uint64 and lens.dtype == np.uint32
    assert list(lens) == [3, 0, 9, 5, 137, 0]
    assert list(offs) == [0, 3, 3, 12, 17, 154]
    assert buf.size == 154 and buf.tobytes() == b"".join(bytes(m) if not isinstance(m, np.ndarray) else m.tobytes() for m in msgs)
    import torch
    buf, offs, lens = pkg.pack_messages([torch.arange(7, dtype=torch.uint8), b"zz"])
    assert list(offs) == [0, 7] and list(lens) == [7, 2] and buf.tobytes() == bytes(range(7)) + b"zz"
    buf, offs, lens = pkg.pack_messages([])
    assert buf.size == 0 and offs.size == 0 and lens.size == 0


def test_host_call_argument_errors_and_no_device(pkg):
    lib = pkg.load_library()
    if lib.mlkem_device_count() > 0:
        pytest.skip("GPU present: tests/test_gpu_sha3r.py covers the entry points")
    body = np.zeros(64, np.uint8)
    off, ln = np.zeros(2, np.uint64), np.array([8, 64], np.uint32)
    out = np.zeros((2, 32), np.uint8)
    st = np.zeros(2, np.int32)
    b, o, l, d, s = (a.ctypes.data for a in (body, off, ln, out, st))
    call = lib.mlkem_sha3_ragged
    # argument errors first
    assert call(6, 2, None, 0, 0, b, 64, o, l, d, 32, 32, s) == MLKEM_ERR_ARG            # alg
    assert call(1, 2, None, 0, 0, b, 64, o, l, d, 31, 32, s) == MLKEM_ERR_ARG            # SHA3-256 has 32 bytes
    assert call(4, 2, None, 0, 0, b, 64, o, l, d, 0, 32, s) == MLKEM_ERR_ARG             # SHAKE outlen 1..65536
    assert call(5, 2, None, 0, 0, b, 64, o, l, d, 65537, 65540, s) == MLKEM_ERR_ARG
    assert call(1, 2, None, 0, 0, b, 64, None, l, d, 32, 32, s) == MLKEM_ERR_ARG         # no offsets
    assert call(1, 2, None, 0, 0, b, 64, o, None, d, 32, 32, s) == MLKEM_ERR_ARG
    assert call(1, 2, None, 0, 0, b, 64, o, l, None, 32, 32, s) == MLKEM_ERR_ARG         # no out
    assert call(1, 2, None, 0, 0, None, 64, o, l, d, 32, 32, s) == MLKEM_ERR_ARG         # no body, but bytes of it
    assert call(1, 2, None, 0, 0, b, 64, o, l, d, 32, 28, s) == MLKEM_ERR_ARG            # rows shorter than the digest
    assert call(1, 2, b, 12, 16, b, 64, o, l, d, 32, 32, s) == MLKEM_ERR_ARG             # head_len % 8
    assert call(1, 2, b, 16, 8, b, 64, o, l, d, 32, 32, s) == MLKEM_ERR_ARG              # head_stride < head_len
    big = np.array([8, 0x7FFFFFFF], np.uint32)
    assert call(1, 2, b, 8, 8, b, 64, o, big.ctypes.data, d, 32, 32, s) == MLKEM_ERR_ARG   # head_len + body_len >= 2^31: checked on the host
    # valid arguments: nothing runs without a device, and nothing falls back to the CPU
    assert call(1, 2, None, 0, 0, b, 64, o, l, d, 32, 32, s) == MLKEM_ERR_NO_DEVICE
    assert call(5, 2, b, 8, 8, b, 64, o, l, d, 32, 32, None) == MLKEM_ERR_NO_DEVICE
    assert call(1, 0, None, 0, 0, None, 0, None, None, None, 32, 32, None) == MLKEM_ERR_NO_DEVICE
    assert not out.any()
    # the device-pointer call needs a context, and no context exists without a device
    assert lib.mlkem_sha3_ragged_dev(None, 1, 2, None, 0, 0, b, 64, o, l, d, 32, 32, s, None) == MLKEM_ERR_ARG
    assert lib.mlkem_sha3_ragged_wide_max(None) == 0


def test_python_argument_checks_without_gpu(pkg):
    """a bad algorithm name, a bad outlen and a body tensor without offsets are refused before any library call"""
    import torch
    e = pkg.MLKEM.__new__(pkg.MLKEM)
    e._ctx = None
    e.torch = torch
    e.device = torch.device("cpu")
    for kw in (dict(alg="sha3", body=[b"a"]), dict(alg="sha3_256", body=[b"a"], outlen=31), dict(alg="shake128", body=[b"a"]),
               dict(alg="shake256", body=[b"a"], outlen=65537), dict(alg="sha3_256", body=torch.zeros(8, dtype=torch.uint8)),
               dict(alg="sha3_256", body=[b"a"], body_off=torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(pkg.MLKEMError) as ex:
            e.sha3(**kw)
        assert ex.value.code == MLKEM_ERR_ARG, kw
