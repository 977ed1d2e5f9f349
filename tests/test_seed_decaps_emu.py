"""CPU tier: decapsulation from 64-byte seed-format keys (d || z, FIPS 203 §3.3) on the host wave emulator.

tests/emu/emu_seed.cpp compiles the product's decaps_seed_run (mlkem_pipeline.hpp) -- the one-workgroup-per-item kernel
k_decaps_seed_small (mlkem_small.hpp) and the batch composition KeyGen -> staging region -> Decaps -- for the emulator.  Every
result is checked against the oracle's KeyGen followed by its Decaps, in both conformance modes, for an untouched ciphertext
(K equals Encaps' K) and a tampered one (K equals J(z || c), the implicit rejection)."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from conftest import seeds
from oracle.loader import SIZES

u8p = C.POINTER(C.c_uint8)


def p8(a):
    return a.ctypes.data_as(u8p)


@pytest.fixture(scope="module")
def emu_seed(tmp_path_factory):
    """the test-only TU, built with build_emulator's compiler line into a temporary directory"""
    emu = os.path.join(ge.ROOT, "tests", "emu")
    out = str(tmp_path_factory.mktemp("emu_seed") / "libmlkem_emu_seed.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-attributes",
                        "-o", out, os.path.join(emu, "emu_seed.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    lib.emu_seed_lds_nonzero.restype = C.c_long
    return lib


def _case(oracle, pset, fips, n, label):
    """seeds, ciphertexts (every second one tampered) and the expected keys: the oracle's KeyGen, then its Decaps"""
    oracle.set_conformance(bool(fips))
    d, z, m = seeds(label + "-d", n, pset), seeds(label + "-z", n, pset), seeds(label + "-m", n, pset)
    ek, dk = oracle.keygen(pset, d, z)
    c, K_enc = oracle.encaps(pset, ek, m)
    tampered = np.arange(n) % 2 == 1
    for i in np.nonzero(tampered)[0]:
        c[i, (37 * i) % c.shape[1]] ^= 1 << (i % 8)
    K_o, st_o = oracle.decaps(pset, dk, c)
    assert (st_o == 0).all()
    shake = hashlib.shake_256 if fips else hashlib.shake_128   # J: SHAKE128 in the reference's mode, SHAKE256 in FIPS 203 mode
    for i in range(n):
        if tampered[i]:
            assert (K_o[i] == np.frombuffer(shake(z[i].tobytes() + c[i].tobytes()).digest(32), np.uint8)).all()
            assert (K_o[i] != K_enc[i]).any()
        else:
            assert (K_o[i] == K_enc[i]).all()
    return np.ascontiguousarray(np.concatenate([d, z], axis=1)), c, K_o


def _run(lib, pset, seed, c):
    K = np.zeros((seed.shape[0], 32), np.uint8)
    assert lib.emu_decaps_seed(pset, C.c_size_t(seed.shape[0]), p8(seed), p8(c), p8(K)) == 0
    return K


@pytest.mark.parametrize("pset,fips,waves", ((512, 0, 8), (512, 1, 4), (768, 0, 8), (768, 1, 4), (1024, 0, 4), (1024, 1, 8)))
def test_emu_fused_seed_decaps_kernel(emu_seed, oracle, pset, fips, waves):
    """k_decaps_seed_small at each wave count decaps_seed_run selects (eight up to small_lat_max, four above): an
    untouched and a tampered ciphertext, bit for bit against the oracle; afterwards the kernel's secret-bearing LDS regions
    (A-hat / PRF rows / sigma / r' / m' / K' / Kbar, ek / s-hat / h, the NTT exchange, the squeezed blocks) are all zero."""
    n = 2
    emu_seed.emu_seed_conformance(fips)
    emu_seed.emu_seed_small(C.c_size_t(16), C.c_size_t(16 if waves == 8 else 0), C.c_size_t(0))
    emu_seed.emu_seed_lds_reset()
    try:
        seed, c, K_o = _case(oracle, pset, fips, n, "sd-%d" % waves)
        K = _run(emu_seed, pset, seed, c)
        assert (K == K_o).all()
        assert emu_seed.emu_seed_lds_regions() == 4
        assert emu_seed.emu_seed_lds_nonzero() == 0
    finally:
        emu_seed.emu_seed_small(C.c_size_t(0), C.c_size_t(256), C.c_size_t(0))
        emu_seed.emu_seed_conformance(0)
        oracle.set_conformance(False)


@pytest.mark.parametrize("pset,fips", ((512, 0), (768, 0), (768, 1), (1024, 0)))
def test_emu_batch_seed_decaps_chunk_loops(emu_seed, oracle, pset, fips):
    """Calls above small_max: KeyGen into the staging region, Decaps from it without the hash check.  cap = 2 and hcap = 3 for
    7 items: the staging loop runs four chunks (the last one short), and KeyGen / Decaps run their own loops inside each."""
    n = 7
    emu_seed.emu_seed_conformance(fips)
    emu_seed.emu_seed_config(C.c_size_t(2), C.c_size_t(3))
    try:
        seed, c, K_o = _case(oracle, pset, fips, n, "sb")
        K = _run(emu_seed, pset, seed, c)
        assert (K == K_o).all()
    finally:
        emu_seed.emu_seed_config(C.c_size_t(0), C.c_size_t(0))
        emu_seed.emu_seed_conformance(0)
        oracle.set_conformance(False)


def test_emu_seed_decaps_small_and_batch_agree(emu_seed, oracle):
    """The same 3 items through both paths (ML-KEM-768, reference mode): the fused kernel and the two-stage composition agree."""
    seed, c, K_o = _case(oracle, 768, 0, 3, "sx")
    K_batch = _run(emu_seed, 768, seed, c)
    emu_seed.emu_seed_small(C.c_size_t(16), C.c_size_t(0), C.c_size_t(0))
    try:
        K_small = _run(emu_seed, 768, seed, c)
    finally:
        emu_seed.emu_seed_small(C.c_size_t(0), C.c_size_t(256), C.c_size_t(0))
    assert (K_batch == K_o).all() and (K_small == K_o).all()
