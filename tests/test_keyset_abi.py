"""CPU tier: the prepared-key-set entry points of the C-ABI (mlkem_keyset_create / _destroy / _info, mlkem_encaps_keyset_dev,
mlkem_decaps_keyset_dev) and their Python face.  The library exports them and the package declares them; without a GPU they fail
loudly (MLKEM_ERR_NO_DEVICE) once the arguments are valid, argument errors come first, and nothing falls back to the CPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

MLKEM_ERR_PARAM_SET, MLKEM_ERR_KEY, MLKEM_ERR_NO_DEVICE, MLKEM_ERR_ARG = -1, -6, -100, -101
KEYSET_SYMBOLS = ("mlkem_keyset_create", "mlkem_keyset_destroy", "mlkem_keyset_info", "mlkem_encaps_keyset_dev", "mlkem_decaps_keyset_dev")


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


def test_keyset_symbols_exported_and_declared(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    with open(os.path.join(ge.ROOT, "include", "mlkem_batch.h")) as f:
        hdr = f.read()
    for s in KEYSET_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in pkg.ABI_SYMBOLS, s
        assert re.search(r"MLKEM_API \w+\*? ?%s\(" % s, hdr), s
    assert re.search(r"#define MLKEM_ERR_KEY \(-6\)", hdr)
    assert pkg.ERR_KEY == MLKEM_ERR_KEY and pkg.ERR_ARG == MLKEM_ERR_ARG
    assert hasattr(pkg, "KeySet") and hasattr(pkg.MLKEM, "prepare_keys")
    e = pkg.MLKEMError(MLKEM_ERR_KEY, "x", key_status=np.array([4], np.int32))
    assert e.code == MLKEM_ERR_KEY and e.key_status[0] == 4


def test_keyset_strerror(pkg):
    lib = pkg.load_library()
    assert lib.mlkem_strerror(MLKEM_ERR_KEY) != lib.mlkem_strerror(12345)
    assert b"key" in lib.mlkem_strerror(MLKEM_ERR_KEY)


def test_keyset_fails_loudly_without_gpu(pkg):
    lib = pkg.load_library()
    if lib.mlkem_device_count() > 0:
        pytest.skip("GPU present: tests/test_gpu_keyset.py covers the entry points")
    h = np.zeros(8192, np.uint8)
    p = h.ctypes.data
    out = C.c_void_p(1234)
    # argument errors first: parameter set, NULL out, NULL set, no context
    assert lib.mlkem_keyset_create(None, 1000, 1, None, p, None, None, C.byref(out), None) == MLKEM_ERR_PARAM_SET
    assert lib.mlkem_keyset_create(None, 768, 1, None, p, None, None, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_keyset_create(None, 768, 1, None, p, None, None, C.byref(out), None) == MLKEM_ERR_ARG
    assert out.value is None   # *out is cleared before anything else can fail
    assert lib.mlkem_keyset_info(None, None, None, None, None) == MLKEM_ERR_ARG
    lib.mlkem_keyset_destroy(None)   # no-op
    assert lib.mlkem_encaps_keyset_dev(None, None, 1, None, p, p, p, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_decaps_keyset_dev(None, None, 1, None, p, p, None, None) == MLKEM_ERR_ARG
    # no context can exist without a device: there is no CPU path to a key set
    ctx = C.c_void_p()
    assert lib.mlkem_ctx_create(C.byref(ctx), 0, 0) == MLKEM_ERR_NO_DEVICE
    with pytest.raises(pkg.MLKEMError) as e:
        pkg.MLKEM(768).prepare_keys(dk=np.zeros((1, 2400), np.uint8))
    assert e.value.code == MLKEM_ERR_NO_DEVICE
