"""CPU tier: batched X25519 (mlkem_x25519.hpp) and the X-Wing layer (mlkem_xwing.hpp) on the host wave emulator.

tests/emu/emu_xwing.cpp compiles the product headers for the emulator and exports the launches and run functions, plus two field
helpers.  Everything is compared with tests/x25519_py.py: Python integers for the field and the ladder, hashlib and
tests/fips203_py.py for X-Wing.  The emulator returns -2 when a staging region does not read zero after a call (both regions are
filled with a pattern before it)."""
import ctypes as C
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import x25519_py as X

pytestmark = pytest.mark.timeout(3600, method="thread")
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
P = X.P
M255 = (1 << 255) - 1


def p8(a):
    return None if a is None else a.ctypes.data_as(u8p)


def rows(values, width=32):
    """list of ints or bytes -> [n, width] uint8"""
    raw = b"".join(v.to_bytes(width, "little") if isinstance(v, int) else bytes(v) for v in values)
    return np.frombuffer(raw, np.uint8).reshape(len(values), width).copy()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """the test-only TU, built with build_emulator's compiler line into a temporary directory, but at -O1: half the compile time of
    -O2 and the same run time for these tests"""
    X.check_pinned()
    out = str(tmp_path_factory.mktemp("emu_xwing") / "libmlkem_emu_xwing.so")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-attributes",
                        "-o", out, os.path.join(ge.ROOT, "tests", "emu", "emu_xwing.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    lib.emu_xwing_config.argtypes = [C.c_size_t] * 3
    lib.emu_xwing_config.restype = None
    lib.emu_fe.argtypes = [C.c_size_t, u8p, u8p, u8p]
    lib.emu_fe.restype = None
    lib.emu_x25519.argtypes = [C.c_size_t, u8p, u8p, u8p, i32p]
    lib.emu_x25519.restype = None
    lib.emu_x25519_pair.argtypes = [C.c_size_t, u8p, u8p, u8p, u8p]
    lib.emu_x25519_pair.restype = None
    lib.emu_xwing_keygen.argtypes = [C.c_size_t, u8p, u8p]
    lib.emu_xwing_encaps.argtypes = [C.c_size_t, u8p, u8p, u8p, C.c_uint64, u8p, u8p, i32p]
    lib.emu_xwing_decaps.argtypes = [C.c_size_t, u8p, u8p, u8p, u8p]
    lib.emu_xwing_derive_sk.argtypes = [C.c_size_t, u8p, C.c_uint64, u8p]
    lib.emu_xwing_derive_sk.restype = None
    return lib


@pytest.fixture
def cfg(emu):
    def set_(cap=0, small=0, wide=0):
        emu.emu_xwing_config(cap, small, wide)
    yield set_
    set_()


# ---- field ------------------------------------------------------------------------------------------------------------------
def fe_encode(emu, values):
    a = rows(values)
    out = np.full_like(a, 0xAA)
    emu.emu_fe(len(values), p8(a), None, p8(out))
    return [int.from_bytes(bytes(r), "little") for r in out]


def fe_mul(emu, xs, ys):
    a, b = rows(xs), rows(ys)
    out = np.full_like(a, 0xAA)
    emu.emu_fe(len(xs), p8(a), p8(b), p8(out))
    return [int.from_bytes(bytes(r), "little") for r in out]


def test_field_encode_is_canonical(emu):
    """decode -> encode of the 255-bit inputs around 0 and p, and with bit 255 set (ignored)"""
    vals = [0, 1, 18, 19, P - 1, P, P + 1, M255]
    assert fe_encode(emu, vals) == [v % P for v in vals]
    assert fe_encode(emu, [v | (1 << 255) for v in vals]) == [v % P for v in vals]


def test_field_products_at_the_limb_bounds(emu):
    """every limb at its maximum (2^255 - 1), p - 1, and single saturated limbs against each other"""
    edge = [M255, P - 1, P, 1, 0, 19, (1 << 26) - 1, ((1 << 25) - 1) << 26, ((1 << 25) - 1) << 230, ((1 << 26) - 1) << 204,
            sum(((1 << 26) - 1) << o for o in (0, 51, 102, 153, 204)), sum(((1 << 25) - 1) << o for o in (26, 77, 128, 179, 230))]
    xs = [x for x in edge for _ in edge]
    ys = [y for _ in edge for y in edge]
    assert fe_mul(emu, xs, ys) == [x % P * (y % P) % P for x, y in zip(xs, ys)]


def test_field_products_random(emu):
    rnd = random.Random(25519)
    xs = [rnd.getrandbits(255) for _ in range(10000)]
    ys = [rnd.getrandbits(255) for _ in range(10000)]
    assert fe_mul(emu, xs, ys) == [x * y % P for x, y in zip(xs, ys)]


# ---- scalar multiplication ----------------------------------------------------------------------------------------------------
def x25519(emu, k, u, status=True):
    n = k.shape[0]
    out = np.full((n, 32), 0xAA, np.uint8)
    st = np.full(n, 7, np.int32) if status else None
    emu.emu_x25519(n, p8(k), p8(u), p8(out), None if st is None else st.ctypes.data_as(i32p))
    return out, st


@pytest.mark.parametrize("n", (1, 64, 65))
def test_x25519_random(emu, n):
    rng = np.random.default_rng(n)
    k, u = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)
    out, st = x25519(emu, k, u)
    assert [bytes(r) for r in out] == [X.x25519(bytes(a), bytes(b)) for a, b in zip(k, u)]
    assert not st.any()
    base, st = x25519(emu, k, None)
    assert [bytes(r) for r in base] == [X.x25519(bytes(a), X.BASE) for a in k]
    assert not st.any()
    # the pair launch of an Encaps item: both multiplications of one scalar
    b2, o2 = np.full((n, 32), 0xAA, np.uint8), np.full((n, 32), 0xAA, np.uint8)
    emu.emu_x25519_pair(n, p8(k), p8(b2), p8(u), p8(o2))
    assert (b2 == base).all() and (o2 == out).all()


def test_x25519_rfc7748_vectors(emu):
    h = bytes.fromhex
    k = rows([h("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4"), X.BASE])
    u = rows([h("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c"), X.BASE])
    out, _ = x25519(emu, k, u)
    assert bytes(out[0]).hex() == "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"
    assert bytes(out[1]).hex() == "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"


def test_x25519_edge_inputs(emu):
    """scalars all-zero and all-0xFF; bit 255 of u ignored; u = 2^255 - 10 = 9 mod p; the low-order inputs give zero and status -7"""
    rnd = random.Random(7748)
    scal = [bytes(32), bytes([0xFF] * 32), bytes(rnd.getrandbits(8) for _ in range(32))]
    us = [9, 9 | (1 << 255), (1 << 255) - 10, rnd.getrandbits(255), M255, P - 2] + list(X.LOW_ORDER_U) + [u | (1 << 255) for u in X.LOW_ORDER_U]
    k = rows([s for s in scal for _ in us])
    u = rows([v for _ in scal for v in us])
    out, st = x25519(emu, k, u)
    want = [X.x25519(bytes(a), bytes(b)) for a, b in zip(k, u)]
    assert [bytes(r) for r in out] == want
    per = len(us)
    for s in range(len(scal)):
        o = out[s * per:(s + 1) * per]
        assert (o[0] == o[1]).all() and (o[0] == o[2]).all()
        assert not o[6:].any() and o[:6].any(axis=1).all()
        assert list(st[s * per:(s + 1) * per]) == [0] * 6 + [-7] * 10


# ---- X-Wing -----------------------------------------------------------------------------------------------------------------------
def keygen(emu, sk):
    n = sk.shape[0]
    pk = np.full((n, 1216), 0xAA, np.uint8)
    assert emu.emu_xwing_keygen(n, p8(sk), p8(pk)) == 0
    return pk


def encaps(emu, pk, eseed=None, root=None, pos=0):
    n = pk.shape[0]
    ct, ss, st = np.full((n, 1120), 0xAA, np.uint8), np.full((n, 32), 0xAA, np.uint8), np.full(n, 7, np.int32)
    r = None if root is None else np.frombuffer(root, np.uint8).copy()
    assert emu.emu_xwing_encaps(n, p8(pk), p8(eseed), p8(r), pos, p8(ct), p8(ss), st.ctypes.data_as(i32p)) == 0
    return ct, ss, st


def decaps(emu, sk, ct, pk=None):
    n = sk.shape[0]
    ss = np.full((n, 32), 0xAA, np.uint8)
    assert emu.emu_xwing_decaps(n, p8(sk), p8(ct), p8(pk), p8(ss)) == 0
    return ss


@pytest.fixture(scope="module")
def restated():
    """65 items of the full restatement, computed once: sk, eseed -> pk, ct, ss"""
    rng = np.random.default_rng(1216)
    sk, eseed = rng.integers(0, 256, (65, 32), dtype=np.uint8), rng.integers(0, 256, (65, 64), dtype=np.uint8)
    pk = rows([X.xwing_keygen(bytes(s)) for s in sk], 1216)
    enc = [X.xwing_encaps(bytes(p), bytes(e)) for p, e in zip(pk, eseed)]
    ct, ss = rows([c for c, _ in enc], 1120), rows([s for _, s in enc])
    for v in (sk, eseed, pk, ct, ss):
        v.setflags(write=False)
    return sk, eseed, pk, ct, ss


# (cap, small, n): one slice with the batch ML-KEM kernels; slices of 2 items (2 + 1, and 32 full slices + 1); slices of 2 items whose
# last, one-item slice goes through the one-workgroup-per-item kernels
SHAPES = ((0, 0, 1), (0, 0, 3), (0, 0, 65), (2, 0, 3), (2, 0, 65), (2, 1, 3))


@pytest.mark.parametrize("cap,small,n", SHAPES)
def test_xwing_against_the_restatement(emu, cfg, restated, cap, small, n):
    """KeyGen, Encaps and Decaps (with and without pk) equal the restatement; Decaps(Encaps) round-trips; the staging regions read
    zero after every call (the emulator's own check: a nonzero return)"""
    sk, eseed, pk_w, ct_w, ss_w = (np.ascontiguousarray(v[:n]) for v in restated)
    cfg(cap=cap, small=small)
    pk = keygen(emu, sk)
    assert (pk == pk_w).all()
    ct, ss, st = encaps(emu, pk, eseed)
    assert (ct == ct_w).all() and (ss == ss_w).all() and not st.any()
    assert (decaps(emu, sk, ct) == ss_w).all()
    assert (decaps(emu, sk, ct, pk) == ss_w).all()
    assert [bytes(r) for r in ss_w[:2]] == [X.xwing_decaps(bytes(s), bytes(c)) for s, c in zip(sk[:2], ct_w[:2])]


def test_xwing_rejection_and_status(emu, cfg, restated):
    """a flipped byte in ct_M gives the restatement's implicit-rejection secret, one in ct_X the restatement's secret (neither the
    sender's); a pk_M coefficient >= q gives status -4 on that item alone"""
    sk, eseed, pk, ct, ss = (np.ascontiguousarray(v[:3]) for v in restated)
    cfg(cap=2)
    bad = ct.copy()
    bad[0, 5] ^= 1
    bad[2, 1088 + 7] ^= 0x10
    got = decaps(emu, sk, bad)
    assert [bytes(r) for r in got] == [X.xwing_decaps(bytes(s), bytes(c)) for s, c in zip(sk, bad)]
    assert (got[0] != ss[0]).any() and (got[2] != ss[2]).any() and (got[1] == ss[1]).all()
    pkb = pk.copy()
    pkb[1, 0], pkb[1, 1] = 0xFF, pkb[1, 1] | 0x0F   # coefficient 0 of item 1 = 0xFFF
    _, _, st = encaps(emu, pkb, eseed)
    assert list(st) == [0, -4, 0]


@pytest.mark.parametrize("wide", (0, 4))
def test_xwing_random_domains(emu, cfg, restated, wide):
    """domains 0x03 / 0x04 of the generator: sk = block[:32], eseed = block[:64] at consecutive positions, in both derivation forms and
    through the sliced random Encaps"""
    root, pos, n = hashlib.sha256(b"xwing-emu-root").digest(), (1 << 32) - 2, 3

    def block(dom, i, nbytes):
        return hashlib.shake_256(root + bytes([dom]) + ((pos + i) & ((1 << 64) - 1)).to_bytes(8, "little")).digest(nbytes)

    cfg(cap=2, wide=wide)
    r = np.frombuffer(root, np.uint8).copy()
    sk = np.full((n, 32), 0xAA, np.uint8)
    emu.emu_xwing_derive_sk(n, p8(r), pos, p8(sk))
    assert [bytes(s) for s in sk] == [block(3, i, 32) for i in range(n)]
    pk = np.ascontiguousarray(restated[2][:n])
    es = rows([block(4, i, 64) for i in range(n)], 64)
    ct_s, ss_s, _ = encaps(emu, pk, es)
    ct_r, ss_r, st = encaps(emu, pk, None, root=root, pos=pos)
    assert (ct_r == ct_s).all() and (ss_r == ss_s).all() and not st.any()
