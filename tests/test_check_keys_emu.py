"""CPU tier: batched key validation (mlkem_check_keys_dev) on the host wave emulator.

tests/emu/emu_check.cpp compiles the product's check_keys_run (mlkem_pipeline.hpp) -- the structural check kernel k_check_keys
(mlkem_check.hpp) with the in-kernel wave-wide hash or the lane-sliced k_hash_batch<0> pre-pass, and the seed / PCT legs through
the staging region -- for the emulator, with lowered limits.  Every status word is compared with one computed independently in
tests/keycheck_cases.py (numpy ByteDecode_12, hashlib SHA3-256, byte comparison, the oracle's KeyGen / Encaps / Decaps_internal)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from keycheck_cases import CLASSES, COMBOS, expected, check_against, make_batch, k_of, SEED

u8p = C.POINTER(C.c_uint8)


def p8(a):
    return None if a is None else a.ctypes.data_as(u8p)


@pytest.fixture(scope="module")
def emu_check(tmp_path_factory):
    """the test-only TU, built with build_emulator's compiler line into a temporary directory"""
    emu = os.path.join(ge.ROOT, "tests", "emu")
    out = str(tmp_path_factory.mktemp("emu_check") / "libmlkem_emu_check.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-attributes",
                        "-o", out, os.path.join(emu, "emu_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    lib.emu_check_last_chunk.restype = C.c_size_t
    lib.emu_check_lds_copy.restype = C.c_size_t
    return lib


def _run(lib, pset, batch, names):
    a = {x: (batch[x] if x in names else None) for x in ("ek", "dk", "seed", "m")}
    n = batch["dk"].shape[0]
    st = np.full(n, -1, np.int32)
    rc = lib.emu_check_keys(pset, C.c_size_t(n), p8(a["ek"]), p8(a["dk"]), p8(a["seed"]), p8(a["m"]),
                            st.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, rc
    return st, a


def _config(lib, cap, wide, small):
    lib.emu_check_config(C.c_size_t(cap), C.c_size_t(wide), C.c_size_t(small))


@pytest.fixture
def limits(emu_check):
    yield lambda cap, wide, small, fips=0: (_config(emu_check, cap, wide, small), emu_check.emu_check_conformance(fips))
    _config(emu_check, 0, 4096, 0)
    emu_check.emu_check_conformance(0)


STRUCTURAL = ("ek", "dk", "ek+dk")


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("fips", (0, 1))
@pytest.mark.parametrize("hash_in", (True, False), ids=("wave-hash", "lane-sliced-hash"))
def test_emu_structural_checks(emu_check, oracle, limits, pset, fips, hash_in):
    """Every corruption class through the structural check alone, in both hash forms: the in-kernel wave-wide H(dk.ek)
    (n <= wide_kem; one round of the nine classes, ek+dk and ek alone -- the emulated wave sponge is slow) and the lane-sliced
    pre-pass into scratch (wide_kem = 0; two rounds, every structural combination); cap = 4 makes several chunks."""
    n = (1 if hash_in else 2) * len(CLASSES)
    limits(4, 4096 if hash_in else 0, 0, fips)
    batch, cls = make_batch(oracle, pset, fips, n, "ks-%d" % pset)
    try:
        for combo in (("ek", "ek+dk") if hash_in else STRUCTURAL):
            names = COMBOS[combo]
            st, given = _run(emu_check, pset, batch, names)
            check_against(st, expected(oracle, pset, fips, given), cls, names)
    finally:
        oracle.set_conformance(False)


LEG_CASES = [(pset, fips, combo) for pset in (512, 768, 1024) for fips in (0, 1)
             for combo in ("ek+dk+seed", "ek+dk+m", "dk+m", "all")]


@pytest.mark.parametrize("pset,fips,combo", LEG_CASES)
def test_emu_seed_and_pct_legs(emu_check, oracle, limits, pset, fips, combo):
    """The seed and PCT legs through the batch KeyGen / Encaps / Decaps kernels and the staging region, one item of every class:
    cap = 4 (three staging rounds; ML-KEM-1024 with all four inputs needs 6432 of the 4800 bytes per item and runs rounds of 2 items).
    The staging region reads back as zero after the call."""
    n = len(CLASSES)
    limits(4, 0, 0, fips)
    batch, cls = make_batch(oracle, pset, fips, n, "kl-%d-%s" % (pset, combo))
    try:
        names = COMBOS[combo]
        st, given = _run(emu_check, pset, batch, names)
        check_against(st, expected(oracle, pset, fips, given), cls, names)
        if pset == 1024 and combo == "all":
            assert emu_check.emu_check_last_chunk() == 2
    finally:
        oracle.set_conformance(False)


@pytest.mark.parametrize("combo", ("all",))
def test_emu_small_call_legs(emu_check, oracle, limits, combo):
    """Calls of at most small_max items: the legs run the one-workgroup-per-item KeyGen / Encaps / Decaps kernels, then ONE
    k_check_keys with the in-kernel hash (ML-KEM-768, reference mode)."""
    n = len(CLASSES)
    limits(0, 4096, 16)
    batch, cls = make_batch(oracle, 768, 0, n, "kss-" + combo)
    try:
        names = COMBOS[combo]
        st, given = _run(emu_check, 768, batch, names)
        check_against(st, expected(oracle, 768, 0, given), cls, names)
    finally:
        oracle.set_conformance(False)


def _keccak_round_constants():
    """the 24 iota constants of Keccak-f[1600] from their LFSR (FIPS 202 §3.2.5)"""
    r, out = 1, []
    for _ in range(24):
        rc = 0
        for j in range(7):
            if r & 1:
                rc |= 1 << ((1 << j) - 1)
            r = ((r << 1) ^ 0x171) if r & 0x80 else (r << 1)
        out.append(rc)
    return out


@pytest.mark.parametrize("pset", (768, 1024))
def test_emu_lds_holds_no_key_bytes(emu_check, oracle, limits, pset):
    """k_check_keys' only LDS in its in-kernel-hash form is the sponge wave's round-constant table and the hash flag it hands to
    the checking wave: after a seed-checked call over valid and corrupted keys the block holds the 24 Keccak constants, the
    zero entry and a flag of 0 / 1 -- no byte of a key, the staged KeyGen output or K.  (The last item, class dk_h, sets it.)"""
    n = 5   # classes valid, ek_q, ek_4095, dkek_q, dk_h
    limits(0, 4096, 0)
    batch, cls = make_batch(oracle, pset, 0, n, "klds")
    emu_check.emu_check_lds_reset()
    try:
        st, given = _run(emu_check, pset, batch, COMBOS["ek+dk+seed"])
        check_against(st, expected(oracle, pset, 0, given), cls, COMBOS["ek+dk+seed"])
    finally:
        oracle.set_conformance(False)
    assert emu_check.emu_check_lds_regions() == 1
    buf = np.zeros(4096, np.uint8)
    got = emu_check.emu_check_lds_copy(p8(buf), C.c_size_t(buf.size))
    assert got == 25 * 8 + 4
    words = buf[:200].view("<u4").reshape(25, 2)
    rc = [int(lo) | (int(hi) << 32) for lo, hi in words]
    assert rc[:24] == _keccak_round_constants() and rc[24] == 0
    assert int(buf[200:204].view("<i4")[0]) == 1
