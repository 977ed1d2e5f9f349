"""CPU tier: prepared key sets (mlkem_keyset.hpp) on the host wave emulator.

tests/emu/emu_keyset.cpp compiles the product's import (check kernel, H table, A-hat^T sampled into the set's table), the
one-workgroup-per-item kernels k_encaps_keyset_small / k_decaps_keyset_small (both wave counts) and the indexed batch path for the
emulator, with lowered limits so that every chunk loop runs more than once with a short last chunk.  Every c / K is compared bit for
bit with the oracle's Encaps / Decaps_internal on the gathered keys; out-of-range items must come back zero with status
MLKEM_ERR_ARG; the import's status words must equal tests/keycheck_cases.py's independently computed bits.  The emulator's flag_wait
spins without bound, so a hand-over bug would hang: the module runs under a thread timeout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from conftest import seeds
from keycheck_cases import CLASSES, make_batch, expected
from oracle.loader import SIZES

pytestmark = pytest.mark.timeout(3600, method="thread")
ERR_ARG = -101
u8p, u32p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


def p8(a):
    return None if a is None else a.ctypes.data_as(u8p)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """the test-only TU, built with build_emulator's compiler line into a temporary directory"""
    out = str(tmp_path_factory.mktemp("emu_keyset") / "libmlkem_emu_keyset.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-attributes",
                        "-o", out, os.path.join(ge.ROOT, "tests", "emu", "emu_keyset.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    lib.emu_ks_lds_nonzero.restype = C.c_size_t
    lib.emu_ks_tables.restype = C.c_size_t
    yield lib
    lib.emu_ks_destroy()


@pytest.fixture
def cfg(emu):
    def set_(cap=0, hcap=0, small=0, lat=0, fips=0):
        emu.emu_ks_config(C.c_size_t(cap), C.c_size_t(hcap), C.c_size_t(small), C.c_size_t(lat))
        emu.emu_ks_conformance(fips)
    yield set_
    set_()


def create(emu, n, ek=None, dk=None, seed=None):
    """emu_ks_create of the parameter set the test put in create.pset: (return code, key_status)"""
    st = np.full(n, -1, np.int32)
    rc = emu.emu_ks_create(create.pset, C.c_size_t(n), p8(ek), p8(dk), p8(seed), st.ctypes.data_as(i32p))
    return rc, st


def run_round(emu, oracle, pset, fips, ek, dk, idx, label, decaps=True, consistent=True):
    """encaps (+ decaps of an untouched and a tampered ciphertext per item) through the set against the oracle on the gathered keys;
    consistent: ek and dk are pairs, so the untouched ciphertexts decapsulate to K"""
    n = len(idx)
    bad = idx >= ek.shape[0]
    g = np.where(bad, 0, idx)
    m = seeds(label, n, pset)
    c, K, st = np.full((n, SIZES[pset][2]), 0xAA, np.uint8), np.full((n, 32), 0xAA, np.uint8), np.full(n, 7, np.int32)
    assert emu.emu_ks_encaps(C.c_size_t(n), idx.ctypes.data_as(u32p), p8(m), p8(c), p8(K), st.ctypes.data_as(i32p)) == 0
    oracle.set_conformance(bool(fips))
    c_o, K_o = oracle.encaps(pset, np.ascontiguousarray(ek[g]), m)
    assert (st == np.where(bad, ERR_ARG, 0)).all(), st
    assert (c[~bad] == c_o[~bad]).all() and (K[~bad] == K_o[~bad]).all()
    assert not c[bad].any() and not K[bad].any()
    if not decaps:
        return
    ct = c_o.copy()
    ct[1::2, 3] ^= 0x40                     # every second item tampered: K = J(z || c)
    K2, st2 = np.full((n, 32), 0xAA, np.uint8), np.full(n, 7, np.int32)
    assert emu.emu_ks_decaps(C.c_size_t(n), idx.ctypes.data_as(u32p), p8(ct), p8(K2), st2.ctypes.data_as(i32p)) == 0
    assert (st2 == np.where(bad, ERR_ARG, 0)).all(), st2
    for i in range(n):
        if bad[i]:
            assert not K2[i].any()
        else:
            assert (K2[i] == oracle.decaps_internal(pset, dk[g[i]], ct[i])).all(), i
            if consistent:
                assert (K2[i] == K_o[i]).all() == (i % 2 == 0), i


def keys(oracle, pset, fips, n, label):
    oracle.set_conformance(bool(fips))
    d, z = seeds(label + "-d", n, pset), seeds(label + "-z", n, pset)
    ek, dk = oracle.keygen(pset, d, z)
    return ek, dk, np.ascontiguousarray(np.concatenate([d, z], axis=1))


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("fips", (0, 1))
@pytest.mark.parametrize("source", ("dk", "seed", "ek"))
def test_emu_keyset_small_kernels(emu, oracle, cfg, pset, fips, source):
    """one workgroup per item, eight waves (n <= lat) and four; repeated, out-of-range and NULL indices; the LDS reads zero after"""
    create.pset = pset
    ek, dk, seed = keys(oracle, pset, fips, 3, "kss-%d" % pset)
    cfg(small=8, lat=2, fips=fips)
    src = {"dk": dict(dk=dk), "seed": dict(seed=seed), "ek": dict(ek=ek)}[source]
    rc, st = create(emu, 3, **src)
    assert rc == 0 and not st.any()
    try:
        oracle.set_conformance(bool(fips))
        for idx, lbl in ((np.array([2, 2], np.uint32), "a"), (np.array([1, 3, 0, 0xFFFFFFFF, 2], np.uint32), "b")):
            emu.emu_ks_lds_reset()
            run_round(emu, oracle, pset, fips, ek, dk, idx, "kss-%d-%s" % (pset, lbl), decaps="ek" not in src)
            assert emu.emu_ks_lds_regions() >= 2
            assert emu.emu_ks_lds_nonzero() == 0
        # NULL key_index: key 0 for every item
        m = seeds("kss-null", 2, pset)
        oracle.set_conformance(bool(fips))
        c_o, K_o = oracle.encaps(pset, np.ascontiguousarray(ek[[0, 0]]), m)
        c, K = np.zeros_like(c_o), np.zeros_like(K_o)
        assert emu.emu_ks_encaps(C.c_size_t(2), None, p8(m), p8(c), p8(K), None) == 0
        assert (c == c_o).all() and (K == K_o).all()
    finally:
        oracle.set_conformance(False)


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("fips", (0, 1))
@pytest.mark.parametrize("source", ("dk", "seed", "ek"))
def test_emu_keyset_batch_path(emu, oracle, cfg, pset, fips, source):
    """the indexed batch kernels with cap = 2, hcap = 4: five items run two h-chunks (4 + 1) and chunks of 2 + 2, 1; the import
    of 5 keys runs its sampler chunk loop three times (2 + 2 + 1); the gathered z rows in scratch read zero after Decaps"""
    create.pset = pset
    ek, dk, seed = keys(oracle, pset, fips, 5, "ksb-%d" % pset)
    cfg(cap=2, hcap=4, small=0, fips=fips)
    src = {"dk": dict(dk=dk), "seed": dict(seed=seed), "ek": dict(ek=ek)}[source]
    rc, st = create(emu, 5, **src)
    assert rc == 0 and not st.any()
    try:
        idx = np.array([4, 0, 7, 4, 1], np.uint32)
        run_round(emu, oracle, pset, fips, ek, dk, idx, "ksb-%d" % pset, decaps="ek" not in src)
        # the tables the import stored: H(ek) of each key (hashlib) -- A-hat^T is covered by every result above
        import hashlib
        k = (ek.shape[1] - 32) // 384
        h = np.zeros((5, 32), np.uint8)
        a = np.zeros((5, k * k * 256), np.uint16)
        assert emu.emu_ks_tables(p8(h), a.ctypes.data_as(C.POINTER(C.c_uint16))) == 5
        for i in range(5):
            assert h[i].tobytes() == hashlib.sha3_256(ek[i].tobytes()).digest()
        assert (a < 3329).all()
    finally:
        oracle.set_conformance(False)


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("fips", (0, 1))
def test_emu_keyset_import_refusal(emu, oracle, cfg, pset, fips):
    """two items per corruption class: ek and dk imports are refused with exactly the expected status words; the keys that pass on
    their own (dk_z, dk_pke, ek_rho, swap among them) form a set whose results match the oracle on those keys"""
    create.pset = pset
    n = 2 * len(CLASSES)   # two "swap" items, which exchange their dks
    batch, cls = make_batch(oracle, pset, fips, n, "ksr-%d" % pset)
    cfg(cap=4, small=4, lat=0, fips=fips)
    try:
        for name in ("ek", "dk"):
            arr = batch[name]
            rc, st = create(emu, n, **{name: arr})
            want = expected(oracle, pset, fips, {name: arr})
            assert rc == -6
            assert (st == want).all(), (st, want, cls)
            good = np.nonzero(want == 0)[0]
            assert {cls[i] for i in good} >= ({"valid", "dk_z", "dk_pke", "swap"} if name == "dk" else {"valid", "ek_rho", "swap"})
            sub = np.ascontiguousarray(arr[good])
            rc, st = create(emu, len(good), **{name: sub})
            assert rc == 0 and not st.any()
            k = (batch["ek"].shape[1] - 32) // 384
            eks = np.ascontiguousarray(sub[:, 384 * k:768 * k + 32]) if name == "dk" else sub
            dks = sub if name == "dk" else None
            idx = np.arange(len(good), dtype=np.uint32)[::-1].copy()
            run_round(emu, oracle, pset, fips, eks, dks, idx, "ksr-%d-%s" % (pset, name), decaps=name == "dk", consistent=False)
    finally:
        oracle.set_conformance(False)
