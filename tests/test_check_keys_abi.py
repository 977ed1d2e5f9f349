"""CPU tier: the key-validation entry points of the C-ABI (mlkem_check_keys_dev, mlkem_check_keys) and their Python face.
The library exports them and the package declares them; without a GPU they fail loudly (MLKEM_ERR_NO_DEVICE) once the
arguments are valid, and argument errors come first, as for the other host-pointer KEM calls."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge

MLKEM_ERR_PARAM_SET, MLKEM_ERR_NO_DEVICE, MLKEM_ERR_ARG = -1, -100, -101


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


def test_check_keys_symbols_exported(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    for s in ("mlkem_check_keys_dev", "mlkem_check_keys"):
        assert hasattr(lib, s), s
        assert s in pkg.ABI_SYMBOLS


def test_keycheck_bits_match_header(pkg):
    import os
    import re
    with open(os.path.join(ge.ROOT, "include", "mlkem_batch.h")) as f:
        hdr = dict(re.findall(r"#define MLKEM_(KEYCHECK_\w+) (\d+)", f.read()))
    assert hdr == {"KEYCHECK_EK_MODULUS": "1", "KEYCHECK_DK_MODULUS": "2", "KEYCHECK_DK_HASH": "4",
                   "KEYCHECK_EK_MISMATCH": "8", "KEYCHECK_SEED": "16", "KEYCHECK_PCT": "32"}
    for name, v in hdr.items():
        assert getattr(pkg, name) == int(v)


def test_check_keys_fails_loudly_without_gpu(pkg):
    lib = pkg.load_library()
    if lib.mlkem_device_count() > 0:
        pytest.skip("GPU present: tests/test_gpu_check_keys.py covers the entry points")
    h = np.zeros(4096, np.uint8)
    st = np.zeros(4, np.int32)
    p, s = h.ctypes.data, st.ctypes.data
    # argument errors first
    assert lib.mlkem_check_keys(1000, 1, p, p, None, None, s) == MLKEM_ERR_PARAM_SET
    assert lib.mlkem_check_keys(768, 1, None, None, None, None, s) == MLKEM_ERR_ARG
    assert lib.mlkem_check_keys(768, 1, p, None, None, p, s) == MLKEM_ERR_ARG
    assert lib.mlkem_check_keys(768, 1, p, p, None, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_check_keys_dev(None, 1000, 1, p, p, None, None, s, None) == MLKEM_ERR_PARAM_SET
    assert lib.mlkem_check_keys_dev(None, 768, 1, p, p, None, None, s, None) == MLKEM_ERR_ARG
    # then: no device, no CPU fallback (every combination of the optional inputs)
    for ek, dk, seed, m in ((p, None, None, None), (None, p, None, None), (p, p, p, None), (None, p, None, p), (p, p, p, p)):
        assert lib.mlkem_check_keys(768, 2, ek, dk, seed, m, s) == MLKEM_ERR_NO_DEVICE
    assert (st == 0).all()
