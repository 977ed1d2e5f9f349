"""CPU tier: the device-side seed derivation entry points of the C-ABI (mlkem_ctx_rng_seed, mlkem_keygen_random_dev,
mlkem_encaps_random_dev, mlkem_encaps_keyset_random_dev) and their Python face.  The library exports them and the package declares
them; argument errors come first; without a device every one of them fails loudly with MLKEM_ERR_NO_DEVICE (nothing falls back to
the CPU); and a failing getrandom(2) is reported as MLKEM_ERR_RNG before any device work."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as ge

MLKEM_ERR_PARAM_SET, MLKEM_ERR_RNG, MLKEM_ERR_NO_DEVICE, MLKEM_ERR_ARG = -1, -2, -100, -101
RNG_SYMBOLS = ("mlkem_ctx_rng_seed", "mlkem_keygen_random_dev", "mlkem_encaps_random_dev", "mlkem_encaps_keyset_random_dev")


@pytest.fixture(scope="module")
def pkg():
    return ge.load_package()


def test_rng_symbols_exported_and_declared(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    with open(os.path.join(ge.ROOT, "include", "mlkem_batch.h")) as f:
        hdr = f.read()
    for s in RNG_SYMBOLS:
        assert hasattr(lib, s), s
        assert s in pkg.ABI_SYMBOLS, s
        assert re.search(r"MLKEM_API int %s\(" % s, hdr), s
    for name in ("rng_seed", "keygen_random", "encaps_random"):
        assert hasattr(pkg.MLKEM, name), name
    assert hasattr(pkg.KeySet, "encaps_random")
    assert pkg.ERR_RNG == MLKEM_ERR_RNG
    # the host-pointer wrappers stay
    assert hasattr(lib, "mlkem_keygen_random") and hasattr(lib, "mlkem_encaps_random")


def test_export_table_equals_the_header(pkg):
    """every MLKEM_API declaration of the header is a defined dynamic symbol of the library, and nothing else is"""
    with open(os.path.join(ge.ROOT, "include", "mlkem_batch.h")) as f:
        hdr = f.read()
    api = set(re.findall(r"^MLKEM_API [^;(]*?\b(mlkem_[a-z0-9_]+)\(", hdr, re.M))
    assert set(RNG_SYMBOLS) <= api
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert names == api, names ^ api
    assert api == set(pkg.ABI_SYMBOLS), api ^ set(pkg.ABI_SYMBOLS)


def test_rng_argument_errors_and_no_device(pkg):
    lib = pkg.load_library()
    if lib.mlkem_device_count() > 0:
        pytest.skip("GPU present: tests/test_gpu_rng.py covers the entry points")
    h = np.zeros(8192, np.uint8)
    p = h.ctypes.data
    assert p % 16 == 0
    seed = (C.c_uint8 * 32)()
    # argument errors first
    assert lib.mlkem_keygen_random_dev(None, 1000, 1, p, p, p, None) == MLKEM_ERR_PARAM_SET
    assert lib.mlkem_encaps_random_dev(None, 0, 1, p, p, p, None, None) == MLKEM_ERR_PARAM_SET
    assert lib.mlkem_keygen_random_dev(None, 768, 1, None, p, p, None) == MLKEM_ERR_ARG          # no ek
    assert lib.mlkem_keygen_random_dev(None, 768, 1, p, None, None, None) == MLKEM_ERR_ARG       # neither dk nor seed_out
    assert lib.mlkem_keygen_random_dev(None, 768, 1, p + 8, p, p, None) == MLKEM_ERR_ARG         # misaligned
    assert lib.mlkem_keygen_random_dev(None, 768, 1, p, p, p + 4, None) == MLKEM_ERR_ARG
    assert lib.mlkem_encaps_random_dev(None, 768, 1, None, p, p, None, None) == MLKEM_ERR_ARG    # no ek
    assert lib.mlkem_encaps_random_dev(None, 768, 1, p, p, None, None, None) == MLKEM_ERR_ARG    # no K
    assert lib.mlkem_encaps_random_dev(None, 768, 1, p, p, p, p + 2, None) == MLKEM_ERR_ARG      # misaligned status
    assert lib.mlkem_encaps_keyset_random_dev(None, None, 1, None, None, p, None, None) == MLKEM_ERR_ARG   # no c
    assert lib.mlkem_encaps_keyset_random_dev(None, None, 1, p + 4, p, p, None, None) == MLKEM_ERR_ARG     # misaligned index
    # valid arguments: no context can exist without a device, and every entry point says so
    assert lib.mlkem_ctx_rng_seed(None, C.addressof(seed)) == MLKEM_ERR_NO_DEVICE
    assert lib.mlkem_ctx_rng_seed(None, None) == MLKEM_ERR_NO_DEVICE
    assert lib.mlkem_keygen_random_dev(None, 768, 1, p, p, p, None) == MLKEM_ERR_NO_DEVICE
    assert lib.mlkem_keygen_random_dev(None, 512, 4, p, None, p, None) == MLKEM_ERR_NO_DEVICE
    assert lib.mlkem_keygen_random_dev(None, 1024, 0, None, None, None, None) == MLKEM_ERR_NO_DEVICE
    assert lib.mlkem_encaps_random_dev(None, 768, 1, p, p, p, None, None) == MLKEM_ERR_NO_DEVICE
    assert lib.mlkem_encaps_keyset_random_dev(None, None, 1, None, p, p, None, None) == MLKEM_ERR_NO_DEVICE
    ctx = C.c_void_p()
    assert lib.mlkem_ctx_create(C.byref(ctx), 0, 0) == MLKEM_ERR_NO_DEVICE
    with pytest.raises(pkg.MLKEMError) as e:
        pkg.MLKEM(768).keygen_random(4)
    assert e.value.code == MLKEM_ERR_NO_DEVICE


def test_rng_seed_reports_a_failing_getrandom(pkg, tmp_path):
    """mlkem_ctx_rng_seed(ctx, NULL) draws the root before any device work: with an interposed getrandom() that always fails (the
    technique of tests/test_abi.py::test_rng_failure_sets_ml_errno_minus_2, in a child process) it returns MLKEM_ERR_RNG with or
    without a device, while a caller-supplied seed never touches the OS source."""
    src = tmp_path / "norandom.c"
    src.write_text("#include <errno.h>\n#include <sys/types.h>\n"
                   "ssize_t getrandom(void* b, size_t n, unsigned f) { (void)b; (void)n; (void)f; errno = ENOSYS; return -1; }\n")
    so = tmp_path / "libnorandom.so"
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    child = r'''
import ctypes as C, sys
lib = C.CDLL(sys.argv[1])
lib.mlkem_ctx_rng_seed.argtypes = [C.c_void_p, C.c_void_p]
assert lib.mlkem_ctx_rng_seed(None, None) == -2, lib.mlkem_ctx_rng_seed(None, None)
seed = (C.c_uint8 * 32)()
rc = lib.mlkem_ctx_rng_seed(None, C.addressof(seed))
assert rc in (-100, -101), rc          # no OS draw: the NULL context is what is wrong (-100 without any device)
print("rng-seed-failure OK")
'''
    env = dict(os.environ, LD_PRELOAD=":".join(x for x in (str(so), os.environ.get("LD_PRELOAD", "")) if x))   # ours first, nothing dropped
    r = subprocess.run([sys.executable, "-c", child, pkg.LIB_PATH], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "rng-seed-failure OK" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def test_python_argument_checks_without_gpu(pkg):
    """keygen_random(dk=False) without return_seed and a seed of the wrong length are refused before any library call"""
    e = pkg.MLKEM.__new__(pkg.MLKEM)
    e._ctx = None
    with pytest.raises(pkg.MLKEMError) as ex:
        e.keygen_random(4, dk=False)
    assert ex.value.code == MLKEM_ERR_ARG
    import torch
    e.torch = torch
    e.lib = pkg.load_library()
    with pytest.raises(pkg.MLKEMError) as ex:
        e.rng_seed(b"short")
    assert ex.value.code == MLKEM_ERR_ARG
