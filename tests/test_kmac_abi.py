"""CPU tier: the C-ABI and Python face of SP 800-185 cSHAKE / KMAC over messages of unequal length (mlkem_cshake_dev, mlkem_kmac_dev,
mlkem_cshake, mlkem_kmac).  The library exports them, the header declares them and ABI_SYMBOLS lists them; the algorithm constants are
0..3 and KMAC_ALGS agrees with the header; the host-pointer calls return MLKEM_ERR_ARG for each argument rule before they look for a
device, and without a device MLKEM_ERR_NO_DEVICE for valid arguments, the output untouched; the Python argument checks run before any
library call; and the restatement the other tiers take their expected values from is pinned against hashlib and the NIST samples."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import sp800185_py as sp

MLKEM_ERR_NO_DEVICE, MLKEM_ERR_ARG = -100, -101
KMAC_SYMBOLS = ("mlkem_cshake_dev", "mlkem_kmac_dev", "mlkem_cshake", "mlkem_kmac")


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


@pytest.fixture(scope="module")
def hdr():
    with open(os.path.join(ge.ROOT, "include", "mlkem_batch.h")) as f:
        return f.read()


def test_restatement_pinned_against_hashlib_and_nist_samples():
    sp.check_pinned()
    assert len(sp.SAMPLES) == 10
    # the encodings, from the text of SP 800-185 section 2.3
    assert sp.left_encode(0) == b"\x01\x00" and sp.right_encode(0) == b"\x00\x01"
    assert sp.left_encode(256) == b"\x02\x01\x00" and sp.right_encode(65536) == b"\x01\x00\x00\x03"
    assert sp.encode_string(b"") == b"\x01\x00" and sp.bytepad(b"ab", 8) == b"\x01\x08ab\x00\x00\x00\x00"
    assert sp.kdf_onestep(256, bytes(32), b"info", 32) == sp.kmac(256, bytes(132), b"\x00\x00\x00\x01" + bytes(32) + b"info", 32, b"KDF")


def test_symbols_exported_and_declared(pkg, hdr):
    lib = C.CDLL(pkg.LIB_PATH)
    for s in KMAC_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in pkg.ABI_SYMBOLS, s
        assert re.search(r"MLKEM_API int %s\(" % s, hdr), s
    for m in ("cshake", "kmac", "kdf_onestep"):
        assert hasattr(pkg.MLKEM, m), m


def test_algorithm_constants_and_python_table(pkg, hdr):
    consts = dict(re.findall(r"^#define (MLKEM_KMAC(?:XOF)?\d+) (\d+)", hdr, re.M))
    assert consts == {"MLKEM_KMAC128": "0", "MLKEM_KMAC256": "1", "MLKEM_KMACXOF128": "2", "MLKEM_KMACXOF256": "3"}
    assert pkg.KMAC_ALGS == {"kmac128": (0, 128, 168, False), "kmac256": (1, 256, 136, False),
                             "kmacxof128": (2, 128, 168, True), "kmacxof256": (3, 256, 136, True)}
    for name, (code, bits, rate, xof) in pkg.KMAC_ALGS.items():
        assert consts["MLKEM_" + name.upper()] == str(code)
        assert rate == sp.rate_of(bits) == 200 - 2 * bits // 8 and xof == ("xof" in name)
    # the SHA-3 table and its constants are untouched: the new functions have entry points of their own
    assert len(pkg.SHA3_ALGS) == 6 and not any(k.startswith("MLKEM_SHA") for k in consts)


def test_host_calls_argument_errors_then_device_check(pkg):
    lib = pkg.load_library()
    have_gpu = lib.mlkem_device_count() > 0
    body = np.arange(64, dtype=np.uint8)
    off, ln = np.zeros(2, np.uint64), np.array([8, 64], np.uint32)
    out = np.zeros((2, 32), np.uint8)
    st = np.full(2, 7, np.int32)
    key = np.arange(80, dtype=np.uint8).reshape(2, 40)
    b, o, l, d, s, k = (a.ctypes.data for a in (body, off, ln, out, st, key))
    S, lead = b"custom", b"\x00\x00\x00\x01"

    def kmac(alg=1, n=2, key=k, key_len=32, key_stride=40, custom=S, custom_len=6, lead=lead, lead_len=4, head=None, head_len=0, head_stride=0,
             body=b, body_bytes=64, off=o, ln=l, out=d, outlen=32, out_stride=32, status=s):
        return lib.mlkem_kmac(alg, n, key, key_len, key_stride, custom, custom_len, lead, lead_len, head, head_len, head_stride, body, body_bytes,
                              off, ln, out, outlen, out_stride, status)

    def cshake(bits=256, n=2, fname=b"N", fname_len=1, custom=S, custom_len=6, lead=lead, lead_len=4, head=None, head_len=0, head_stride=0,
               body=b, body_bytes=64, off=o, ln=l, out=d, outlen=32, out_stride=32, status=s):
        return lib.mlkem_cshake(bits, n, fname, fname_len, custom, custom_len, lead, lead_len, head, head_len, head_stride, body, body_bytes,
                                off, ln, out, outlen, out_stride, status)
    big = np.array([8, 0x7FFFFFFF], np.uint32)
    for kw in (dict(alg=4), dict(alg=-1), dict(outlen=0), dict(outlen=65537, out_stride=65540), dict(key_len=0), dict(key_len=12),
               dict(key_len=136, key_stride=136), dict(key_len=40, key_stride=32), dict(key=None), dict(key_stride=0, key_len=513),
               dict(key_stride=0, key=None), dict(custom_len=257), dict(custom=None), dict(lead_len=9, lead=bytes(9)), dict(lead=None),
               dict(off=None), dict(ln=None), dict(out=None), dict(body=None), dict(out_stride=28), dict(head=b, head_len=12, head_stride=16),
               dict(head=b, head_len=16, head_stride=8), dict(head=b, head_len=8, head_stride=8, ln=big.ctypes.data)):
        assert kmac(**kw) == MLKEM_ERR_ARG, kw
    for kw in (dict(bits=192), dict(bits=0), dict(fname_len=33, fname=bytes(33)), dict(fname=None), dict(custom_len=257), dict(outlen=0),
               dict(out=None), dict(lead_len=9, lead=bytes(9)), dict(off=None), dict(out_stride=28), dict(head=b, head_len=12, head_stride=16),
               dict(ln=big.ctypes.data)):
        assert cshake(**kw) == MLKEM_ERR_ARG, kw
    assert not out.any() and list(st) == [7, 7]
    # the device-pointer calls need a context
    assert lib.mlkem_kmac_dev(None, 1, 2, k, 32, 40, S, 6, lead, 4, None, 0, 0, b, 64, o, l, d, 32, 32, s, None) == MLKEM_ERR_ARG
    assert lib.mlkem_cshake_dev(None, 256, 2, b"N", 1, S, 6, lead, 4, None, 0, 0, b, 64, o, l, d, 32, 32, s, None) == MLKEM_ERR_ARG
    if not have_gpu:
        # valid arguments: nothing runs without a device, and nothing falls back to the CPU
        assert kmac() == MLKEM_ERR_NO_DEVICE and cshake() == MLKEM_ERR_NO_DEVICE
        assert kmac(key_stride=0, key_len=80) == MLKEM_ERR_NO_DEVICE and kmac(n=0) == MLKEM_ERR_NO_DEVICE
        assert not out.any() and list(st) == [7, 7]
    else:
        assert kmac() == 0 and list(st) == [0, 0]
        for i, n in enumerate((8, 64)):
            assert out[i].tobytes() == sp.kmac(256, key[i, :32].tobytes(), lead + body[:n].tobytes(), 32, S), i
        assert cshake() == 0
        assert out[1].tobytes() == sp.cshake(256, lead + body.tobytes(), 32, b"N", S)


def test_python_argument_checks_without_gpu(pkg):
    """bad bits, outlen, lead, strings and keys are refused before any library call"""
    import torch
    e = pkg.MLKEM.__new__(pkg.MLKEM)
    e._ctx = None
    e.torch = torch
    e.device = torch.device("cpu")
    key2 = torch.zeros((1, 32), dtype=torch.uint8)
    for kw in (dict(bits=192, body=[b"a"], outlen=32), dict(bits=128, body=[b"a"], outlen=0), dict(bits=128, body=[b"a"], outlen=65537),
               dict(bits=256, body=[b"a"], outlen=32, lead=bytes(9)), dict(bits=256, body=[b"a"], outlen=32, function_name=bytes(33)),
               dict(bits=256, body=[b"a"], outlen=32, custom=bytes(257)), dict(bits=256, body=torch.zeros(8, dtype=torch.uint8), outlen=32),
               dict(bits=256, body=[b"a"], body_off=torch.zeros(1, dtype=torch.int64), outlen=32)):
        with pytest.raises(pkg.MLKEMError) as ex:
            e.cshake(**kw)
        assert ex.value.code == MLKEM_ERR_ARG, kw
    for kw in (dict(bits=512, key=key2, body=[b"a"], outlen=32), dict(bits=256, key=key2, body=[b"a"], outlen=0),
               dict(bits=256, key=bytes(513), body=[b"a"], outlen=32), dict(bits=256, key=key2[:, :12], body=[b"a"], outlen=32),
               dict(bits=256, key=torch.zeros((1, 136), dtype=torch.uint8), body=[b"a"], outlen=32),
               dict(bits=256, key=torch.zeros((2, 32), dtype=torch.uint8), body=[b"a"], outlen=32),
               dict(bits=256, key=torch.zeros((1, 32), dtype=torch.int32), body=[b"a"], outlen=32),
               dict(bits=256, key=key2, body=[b"a"], outlen=32, custom=bytes(257)), dict(bits=256, key=key2, body=[b"a"], outlen=32, lead=bytes(9)),
               dict(bits=256, key="secret", body=[b"a"], outlen=32)):
        with pytest.raises(pkg.MLKEMError) as ex:
            e.kmac(**kw)
        assert ex.value.code == MLKEM_ERR_ARG, kw
    with pytest.raises(pkg.MLKEMError) as ex:
        e.kdf_onestep(torch.zeros((1, 32), dtype=torch.uint8), [b"info"], 32, bits=384)
    assert ex.value.code == MLKEM_ERR_ARG
