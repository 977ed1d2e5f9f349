"""CPU tier: deferred implicit rejection in the lane-sliced batch Decaps, on the host wave emulator.

Above ws.wide_kem(K) items k_hash_decaps no longer computes Kbar = J(z || c) for every item: the compare kernel (encrypt2_body,
CMP_DEFER) stores K' & ~reject, appends every rejected item to the h-chunk's reject list in ws.Kbar, and k_hash_j_rejected hashes
the listed items alone into their K rows.  Every result is compared bit for bit with oracle.decaps.

n = 67 is one full wave of list entries plus 3.  emu_config(0, 0) runs one h-chunk of 67 (the list counter's atomicAdd sees all
64 lanes of k_hash_j_rejected's first wave); emu_config(5, 11) has chunks cross h-chunks and resets the list seven times."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from conftest import seeds
from oracle.loader import SIZES

u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
N = 67
GUARD = 0xA5

PATTERNS = {
    "none": [],
    "all": list(range(N)),
    "odd": list(range(1, N, 2)),          # the upper half-waves of the compare kernel
    "even": list(range(0, N, 2)),         # the lower ones
    "sparse": [0, 31, 32, 63, 64, 66],
    # with hcap = 11: h-chunk 0 fully rejected, h-chunk 1 (and every later one) with none -- a list that is not reset would replay
    "first_hchunk": list(range(11)),
}
CONFIGS = ((0, 0), (5, 11))
SETS = ((768, 0), (1024, 1))


def p8(a):
    return a.ctypes.data_as(u8p)


@pytest.fixture(scope="module")
def emu():
    lib = C.CDLL(ge.build_emulator())
    lib.emu_wide_hash(C.c_size_t(0))   # the lane-sliced form, whatever a test before this one left behind
    lib.emu_small(C.c_size_t(0))
    return lib


@pytest.fixture(scope="module")
def cases(oracle):
    """keys and honest ciphertexts per (parameter set, mode), computed once; the tests copy what they change"""
    out = {}
    for pset, fips in SETS:
        oracle.set_conformance(bool(fips))
        try:
            d, z, m = seeds("dd-d", N, pset), seeds("dd-z", N, pset), seeds("dd-m", N, pset)
            ek, dk = oracle.keygen(pset, d, z)
            c, K = oracle.encaps(pset, ek, m)
        finally:
            oracle.set_conformance(False)
        for a in (dk, c, K):
            a.setflags(write=False)
        out[pset, fips] = (dk, c, K)
    return out


def tamper(c, items):
    """one flipped bit per listed item, at a position that moves with the item"""
    ct = c.copy()
    for i in items:
        ct[i, (131 * i + 7) % ct.shape[1]] ^= 1 << (i % 8)
    return ct


def expect(oracle, pset, fips, dk, ct, items, K_enc):
    oracle.set_conformance(bool(fips))
    try:
        K_o, st_o = oracle.decaps(pset, np.ascontiguousarray(dk), ct)
    finally:
        oracle.set_conformance(False)
    rej = np.zeros(ct.shape[0], bool)
    rej[items] = True
    assert (st_o == 0).all()
    assert ((K_o == K_enc[: ct.shape[0]]).all(axis=1) == ~rej).all()   # the pattern is what the oracle rejects
    return K_o


def run(emu, fn, pset, dk, ct, with_check=True):
    """K and status of one emulated call, each with a guard row behind the n rows that must come back untouched"""
    n = ct.shape[0]
    K = np.full((n + 1, 32), GUARD, np.uint8)
    st = np.full(n + 1, 0x5A5A5A5A, np.int32)
    args = [pset, C.c_size_t(n), p8(dk), p8(ct), p8(K), st.ctypes.data_as(i32p)]
    if fn == "emu_decaps":
        args.append(1 if with_check else 0)
    assert getattr(emu, fn)(*args) == 0
    assert (K[n] == GUARD).all() and st[n] == 0x5A5A5A5A
    return K[:n], st[:n]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "cap%d-hcap%d" % c)
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("pset,fips", SETS)
def test_emu_deferred_rejection(emu, oracle, cases, pset, fips, pattern, cfg):
    dk, c, K_enc = cases[pset, fips]
    items = PATTERNS[pattern]
    ct = tamper(c, items)
    K_o = expect(oracle, pset, fips, dk, ct, items, K_enc)
    emu.emu_conformance(fips)
    emu.emu_config(C.c_size_t(cfg[0]), C.c_size_t(cfg[1]))
    try:
        K, st = run(emu, "emu_decaps", pset, np.ascontiguousarray(dk), ct)
    finally:
        emu.emu_config(C.c_size_t(0), C.c_size_t(0))
        emu.emu_conformance(0)
    assert (st == 0).all()
    bad = np.nonzero((K != K_o).any(axis=1))[0]
    assert bad.size == 0, "items that differ from the oracle: %s" % bad.tolist()


@pytest.mark.parametrize("pattern", ("sparse", "all"))
def test_emu_deferred_rejection_without_hash_check(emu, oracle, cases, pattern):
    """hash_check off: k_hash_decaps runs G alone (one role, no status words of its own)"""
    dk, c, K_enc = cases[768, 0]
    items = PATTERNS[pattern]
    ct = tamper(c, items)
    K_o = expect(oracle, 768, 0, dk, ct, items, K_enc)
    emu.emu_config(C.c_size_t(5), C.c_size_t(11))
    try:
        K, _ = run(emu, "emu_decaps", 768, np.ascontiguousarray(dk), ct, with_check=False)
    finally:
        emu.emu_config(C.c_size_t(0), C.c_size_t(0))
    assert (K == K_o).all()


@pytest.mark.parametrize("pattern", ("sparse", "all"))
def test_emu_deferred_rejection_shared_key(emu, oracle, pattern):
    """decaps_shared_run: one dk for all items (z stride 0 in k_hash_j_rejected), chunks crossing h-chunks"""
    pset, ekl = 768, SIZES[768][0]
    d, z, m = seeds("dds-d", 1, pset), seeds("dds-z", 1, pset), seeds("dds-m", N, pset)
    ek1, dk1 = oracle.keygen(pset, d, z)
    assert ek1.shape[1] == ekl
    c, K_enc = oracle.encaps(pset, np.repeat(ek1, N, axis=0), m)
    items = PATTERNS[pattern]
    ct = tamper(c, items)
    K_o = expect(oracle, pset, 0, np.repeat(dk1, N, axis=0), ct, items, K_enc)
    emu.emu_config(C.c_size_t(5), C.c_size_t(11))
    try:
        K, st = run(emu, "emu_decaps_shared", pset, dk1, ct)
    finally:
        emu.emu_config(C.c_size_t(0), C.c_size_t(0))
    assert (st == 0).all() and (K == K_o).all()


@pytest.fixture(scope="module")
def emu_ks(tmp_path_factory):
    """tests/emu/emu_keyset.cpp, built with build_emulator's compiler line into a temporary directory"""
    import os
    import subprocess
    out = str(tmp_path_factory.mktemp("emu_keyset_dd") / "libmlkem_emu_keyset.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-attributes",
                        "-o", out, os.path.join(ge.ROOT, "tests", "emu", "emu_keyset.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    yield lib
    lib.emu_ks_destroy()


@pytest.mark.parametrize("pattern", ("sparse", "all"))
def test_emu_deferred_rejection_keyset_batch(emu_ks, oracle, pattern):
    """decaps_keyset_run's batch branch (small limit 0): k_hash_j_rejected reads z from the set by index, before k_keyset_fix.
    Item 31 names a key outside the set and is rejected in both patterns: it must end as zeros and MLKEM_ERR_ARG."""
    pset, nk, n = 768, 3, 35
    d, z, m = seeds("ddk-d", nk, pset), seeds("ddk-z", nk, pset), seeds("ddk-m", n, pset)
    ek, dk = oracle.keygen(pset, d, z)
    idx = (np.arange(n) % nk).astype(np.uint32)
    idx[31] = 9
    g = np.where(idx >= nk, 0, idx)
    c, K_enc = oracle.encaps(pset, np.ascontiguousarray(ek[g]), m)
    items = [i for i in PATTERNS[pattern] if i < n]
    ct = tamper(c, items)
    K_o = expect(oracle, pset, 0, dk[g], ct, items, K_enc)
    K_o[31] = 0
    emu_ks.emu_ks_conformance(0)
    emu_ks.emu_ks_config(C.c_size_t(5), C.c_size_t(11), C.c_size_t(0), C.c_size_t(0))
    try:
        st = np.full(nk, -1, np.int32)
        assert emu_ks.emu_ks_create(pset, C.c_size_t(nk), None, p8(dk), None, st.ctypes.data_as(i32p)) == 0 and not st.any()
        K = np.full((n + 1, 32), GUARD, np.uint8)
        st = np.full(n + 1, 0x5A5A5A5A, np.int32)
        assert emu_ks.emu_ks_decaps(C.c_size_t(n), idx.ctypes.data_as(C.POINTER(C.c_uint32)), p8(ct), p8(K), st.ctypes.data_as(i32p)) == 0
    finally:
        emu_ks.emu_ks_config(C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0))
    assert (K[n] == GUARD).all() and st[n] == 0x5A5A5A5A
    assert (st[:n] == np.where(idx >= nk, -101, 0)).all()
    assert (K[:n] == K_o).all()
