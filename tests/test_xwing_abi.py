"""CPU tier: the X25519 / X-Wing entry points of the C-ABI (mlkem_x25519_dev, mlkem_xwing_keygen_dev, mlkem_xwing_encaps_dev,
mlkem_xwing_decaps_dev, mlkem_xwing_keygen_random_dev, mlkem_xwing_encaps_random_dev) and their Python face: the header carries the
size macros and the new status code, argument errors come first, without a device every call fails loudly with MLKEM_ERR_NO_DEVICE
and writes nothing, and the Python wrappers refuse wrong shapes, dtypes and devices before any pointer reaches C."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

MLKEM_ERR_LENGTH, MLKEM_ERR_LOW_ORDER, MLKEM_ERR_NO_DEVICE, MLKEM_ERR_ARG = -3, -7, -100, -101
XWING_SYMBOLS = ("mlkem_x25519_dev", "mlkem_xwing_keygen_dev", "mlkem_xwing_encaps_dev", "mlkem_xwing_decaps_dev",
                 "mlkem_xwing_keygen_random_dev", "mlkem_xwing_encaps_random_dev")


@pytest.fixture(scope="module")
def pkg():
    ge.build()
    return ge.load_package()


def test_header_macros_symbols_and_error_text(pkg):
    with open(os.path.join(ge.ROOT, "include", "mlkem_batch.h")) as f:
        hdr = f.read()
    for name, value in (("SK", 32), ("PK", 1216), ("CT", 1120), ("SS", 32), ("ESEED", 64)):
        assert re.search(r"^#define MLKEM_XWING_%s_BYTES %d\b" % (name, value), hdr, re.M), name
    assert re.search(r"^#define MLKEM_ERR_LOW_ORDER \(-7\)", hdr, re.M)
    assert "WRONG SECRET SILENTLY" in hdr.upper()
    lib = C.CDLL(pkg.LIB_PATH)
    for s in XWING_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in pkg.ABI_SYMBOLS, s
        assert re.search(r"^MLKEM_API int %s\(" % s, hdr, re.M), s
    assert pkg.ERR_LOW_ORDER == MLKEM_ERR_LOW_ORDER
    assert pkg.XWING_SIZES == {"sk": 32, "pk": 1216, "ct": 1120, "ss": 32, "eseed": 64}
    for name in ("x25519", "xwing_keygen", "xwing_encaps", "xwing_decaps", "xwing_keygen_random", "xwing_encaps_random"):
        assert hasattr(pkg.MLKEM, name), name
    lib.mlkem_strerror.restype = C.c_char_p
    text = lib.mlkem_strerror(MLKEM_ERR_LOW_ORDER)
    assert text and text != lib.mlkem_strerror(-9999) and b"unknown" not in text


def calls(lib, p, ctx):
    """the six entry points on valid, aligned host buffers (never dereferenced: every call fails before any device work)"""
    return (("x25519", lambda: lib.mlkem_x25519_dev(ctx, 1, p, p, p, p, None)),
            ("x25519_base", lambda: lib.mlkem_x25519_dev(ctx, 1, p, None, p, None, None)),
            ("keygen", lambda: lib.mlkem_xwing_keygen_dev(ctx, 1, p, p, None)),
            ("encaps", lambda: lib.mlkem_xwing_encaps_dev(ctx, 1, p, p, p, p, p, None)),
            ("decaps", lambda: lib.mlkem_xwing_decaps_dev(ctx, 1, p, p, None, p, None)),
            ("decaps_pk", lambda: lib.mlkem_xwing_decaps_dev(ctx, 1, p, p, p, p, None)),
            ("keygen_random", lambda: lib.mlkem_xwing_keygen_random_dev(ctx, 1, p, p, None)),
            ("encaps_random", lambda: lib.mlkem_xwing_encaps_random_dev(ctx, 1, p, p, p, p, None)))


def test_null_context(pkg):
    """a NULL context: MLKEM_ERR_NO_DEVICE on a machine without a device (the cause, not the symptom), MLKEM_ERR_ARG with one; either
    way nothing is written.  Argument errors come first."""
    lib = pkg.load_library()
    h = np.full(8192, 0x5A, np.uint8)
    p = h.ctypes.data
    assert p % 16 == 0
    want = MLKEM_ERR_NO_DEVICE if lib.mlkem_device_count() == 0 else MLKEM_ERR_ARG
    for name, call in calls(lib, p, None):
        assert call() == want, name
    assert (h == 0x5A).all()
    # n == 0 is a no-op only for a usable context
    assert lib.mlkem_xwing_keygen_dev(None, 0, None, None, None) == want
    # NULL and misaligned pointers
    assert lib.mlkem_x25519_dev(None, 1, None, p, p, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_x25519_dev(None, 1, p, p, None, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_x25519_dev(None, 1, p, p + 8, p, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_x25519_dev(None, 1, p, p, p, p + 2, None) == MLKEM_ERR_ARG
    assert lib.mlkem_xwing_keygen_dev(None, 1, p, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_xwing_keygen_dev(None, 1, p + 4, p, None) == MLKEM_ERR_ARG
    assert lib.mlkem_xwing_encaps_dev(None, 1, p, None, p, p, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_xwing_encaps_dev(None, 1, p, p, p, p + 8, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_xwing_encaps_dev(None, 1, p, p, p, p, p + 1, None) == MLKEM_ERR_ARG
    assert lib.mlkem_xwing_decaps_dev(None, 1, p, p, None, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_xwing_decaps_dev(None, 1, p, p, p + 8, p, None) == MLKEM_ERR_ARG
    assert lib.mlkem_xwing_keygen_random_dev(None, 1, None, p, None) == MLKEM_ERR_ARG
    assert lib.mlkem_xwing_encaps_random_dev(None, 1, p, p, None, None, None) == MLKEM_ERR_ARG
    assert (h == 0x5A).all()
    if want == MLKEM_ERR_NO_DEVICE:   # and no engine can exist to call the methods on
        with pytest.raises(pkg.MLKEMError) as e:
            pkg.MLKEM(512).xwing_keygen_random(4)
        assert e.value.code == MLKEM_ERR_NO_DEVICE


def test_python_wrappers_validate_inputs(pkg):
    """On CPU tensors through a bare instance (no engine can be created without a GPU): wrong row lengths, element types, devices
    and batch sizes are refused before the library is called -- the instance has no library and no context to call with."""
    import torch
    e = pkg.MLKEM.__new__(pkg.MLKEM)
    e.torch, e.device, e._ctx = torch, torch.device("cpu"), None
    u8 = torch.uint8
    sk, pk, ct, es = (torch.zeros((4, w), dtype=u8) for w in (32, 1216, 1120, 64))

    def refused(code, fn, *a, **k):
        with pytest.raises(pkg.MLKEMError) as ex:
            fn(*a, **k)
        assert ex.value.code == code, (fn.__name__, a)

    # row lengths: the reference's type check (-3)
    refused(MLKEM_ERR_LENGTH, e.x25519, torch.zeros((4, 31), dtype=u8))
    refused(MLKEM_ERR_LENGTH, e.x25519, sk, torch.zeros((4, 33), dtype=u8))
    refused(MLKEM_ERR_LENGTH, e.xwing_keygen, torch.zeros((4, 64), dtype=u8))
    refused(MLKEM_ERR_LENGTH, e.xwing_encaps, torch.zeros((4, 1184), dtype=u8), es)
    refused(MLKEM_ERR_LENGTH, e.xwing_encaps, pk, torch.zeros((4, 32), dtype=u8))
    refused(MLKEM_ERR_LENGTH, e.xwing_decaps, sk, torch.zeros((4, 1088), dtype=u8))
    refused(MLKEM_ERR_LENGTH, e.xwing_decaps, sk, ct, torch.zeros((4, 1184), dtype=u8))
    refused(MLKEM_ERR_LENGTH, e.xwing_encaps_random, torch.zeros((4, 1215), dtype=u8))
    # element types and devices: refused, never converted or copied
    refused(MLKEM_ERR_ARG, e.x25519, sk.to(torch.int64))
    refused(MLKEM_ERR_ARG, e.x25519, sk, sk.to(torch.float32))
    refused(MLKEM_ERR_ARG, e.xwing_keygen, sk.to(torch.int8))
    refused(MLKEM_ERR_ARG, e.xwing_encaps, pk, es.to(torch.int32))
    refused(MLKEM_ERR_ARG, e.xwing_decaps, sk, ct.to(torch.int16))
    refused(MLKEM_ERR_ARG, e.xwing_keygen, torch.zeros((4, 32), dtype=u8, device="meta"))
    refused(MLKEM_ERR_ARG, e.xwing_decaps, sk, ct, torch.zeros((4, 1216), dtype=u8, device="meta"))
    refused(MLKEM_ERR_ARG, e.xwing_encaps_random, torch.zeros((4, 1216), dtype=u8, device="meta"))
    # batch sizes
    refused(MLKEM_ERR_ARG, e.x25519, sk, sk[:3])
    refused(MLKEM_ERR_ARG, e.xwing_encaps, pk, es[:2])
    refused(MLKEM_ERR_ARG, e.xwing_decaps, sk, ct[:3])
    refused(MLKEM_ERR_ARG, e.xwing_decaps, sk, ct, pk[:1])
