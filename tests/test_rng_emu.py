"""CPU tier: device-side seed derivation (mlkem_rng.hpp) on the host wave emulator.

tests/emu/emu_rng.cpp compiles both derivation forms (k_rng_derive: one item per lane; k_rng_derive_w: one sponge per wavefront) and
the sliced random KeyGen / Encaps sequencing for the emulator.  The derivation is restated here with hashlib:
    block(root, dom, pos) = SHAKE256(root || dom || LE64(pos)) ; KeyGen: d || z = block[:64] (dom 1) ; Encaps: m = block[:32] (dom 2)
and, given those seeds, every ek / dk / c / K is compared bit for bit with the oracle's KeyGen / Encaps on them, in both conformance
modes, at sizes either side of every slice and form switch.  The emulator returns -2 when the derived-seed region or the dk staging
region does not read zero after a call (both are filled with a pattern before it)."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle.loader import SIZES

pytestmark = pytest.mark.timeout(3600, method="thread")
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
DOM_KEYGEN, DOM_ENCAPS = 1, 2
M64 = (1 << 64) - 1
ROOTS = [bytes(32), bytes(range(32)), bytes([0xFF] * 32), hashlib.sha256(b"rng-emu-root").digest()]


def p8(a):
    return None if a is None else a.ctypes.data_as(u8p)


def block(root, dom, pos, nbytes=64):
    return hashlib.shake_256(root + bytes([dom]) + (pos & M64).to_bytes(8, "little")).digest(nbytes)


def blocks(root, dom, pos, n, nbytes):
    return np.frombuffer(b"".join(block(root, dom, pos + i, nbytes) for i in range(n)), np.uint8).reshape(n, nbytes).copy()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """the test-only TU, built with build_emulator's compiler line into a temporary directory"""
    out = str(tmp_path_factory.mktemp("emu_rng") / "libmlkem_emu_rng.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-attributes",
                        "-o", out, os.path.join(ge.ROOT, "tests", "emu", "emu_rng.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    lib.emu_rng_derive.restype = None
    lib.emu_rng_derive.argtypes = [C.c_int, C.c_int, C.c_size_t, u8p, C.c_uint64, u8p, u8p, u8p]
    lib.emu_rng_keygen.argtypes = [C.c_int, C.c_size_t, u8p, C.c_uint64, u8p, u8p, u8p]
    lib.emu_rng_encaps.argtypes = [C.c_int, C.c_size_t, u8p, C.c_uint64, u8p, u8p, u8p, i32p]
    lib.emu_rng_config.argtypes = [C.c_size_t] * 5
    return lib


@pytest.fixture
def cfg(emu):
    def set_(cap=0, hcap=0, small=0, lat=256, wide=0, fips=0):
        emu.emu_rng_config(cap, hcap, small, lat, wide)
        emu.emu_rng_conformance(fips)
    yield set_
    set_()


def derive(emu, form, dom, root, pos, n, with_seed_out=True):
    """the bare derivation: (d or m rows, z rows, seed_out rows)"""
    r = np.frombuffer(root, np.uint8).copy()
    o0 = np.full((n, 32), 0xAA, np.uint8)
    o1 = np.full((n, 32), 0xAA, np.uint8) if dom == DOM_KEYGEN else None
    so = np.full((n, 64), 0xAA, np.uint8) if dom == DOM_KEYGEN and with_seed_out else None
    emu.emu_rng_derive(form, int(dom == DOM_KEYGEN), n, p8(r), pos & M64, p8(o0), p8(o1), p8(so))
    return o0, o1, so


# base positions: 0, the values around 2^32 and 2^24 / 2^56 (the word boundaries of the block's position bytes), and the last few
# positions before the counter wraps (a run that starts at 2^64 - 5 continues at 0)
BASES = [0, (1 << 24) - 3, (1 << 32) - 7, (1 << 32), (1 << 56) - 2, (1 << 63) + 12345, (1 << 64) - 5]


@pytest.mark.parametrize("form,count", ((0, 70), (1, 12)))
def test_derivation_forms_equal_hashlib(emu, form, count):
    """Both forms, both domains, four roots, seven base positions: `count` consecutive positions each (the lane-sliced form runs two
    wavefronts with a short second one) -- 2 x 4 x 7 x 70 = 3920 positions lane-sliced, 2 x 4 x 7 x 12 = 672 wave-wide."""
    checked = 0
    for root in ROOTS:
        for base in BASES:
            want = blocks(root, DOM_KEYGEN, base, count, 64)
            d, z, so = derive(emu, form, DOM_KEYGEN, root, base, count)
            assert (so == want).all(), (form, base)
            assert (d == want[:, :32]).all() and (z == want[:, 32:]).all(), (form, base)
            m, _, _ = derive(emu, form, DOM_ENCAPS, root, base, count)
            assert (m == blocks(root, DOM_ENCAPS, base, count, 32)).all(), (form, base)
            checked += 2 * count
    assert checked >= (1000 if form == 0 else 600)


def test_wave_form_reaches_a_thousand_positions(emu):
    """the one-sponge-per-wavefront form over 1000 consecutive positions across 2^32 (with the 672 above: more than 1000 for this
    form on its own), and without seed_out"""
    root, base, n = ROOTS[3], (1 << 32) - 500, 1000
    want = blocks(root, DOM_KEYGEN, base, n, 64)
    d, z, _ = derive(emu, 1, DOM_KEYGEN, root, base, n, with_seed_out=False)
    assert (d == want[:, :32]).all() and (z == want[:, 32:]).all()


def test_domains_and_roots_separate(emu):
    """sanity of the construction: the KeyGen and Encaps blocks of one position differ, and so do two roots"""
    d, _, _ = derive(emu, 0, DOM_KEYGEN, ROOTS[1], 9, 1)
    m, _, _ = derive(emu, 0, DOM_ENCAPS, ROOTS[1], 9, 1)
    d2, _, _ = derive(emu, 0, DOM_KEYGEN, ROOTS[3], 9, 1)
    assert (d != m).any() and (d != d2).any()


def keygen(emu, pset, root, pos, n, dk=True, seed=True):
    r = np.frombuffer(root, np.uint8).copy()
    ek = np.full((n, SIZES[pset][0]), 0xAA, np.uint8)
    dk_a = np.full((n, SIZES[pset][1]), 0xAA, np.uint8) if dk else None
    so = np.full((n, 64), 0xAA, np.uint8) if seed else None
    assert emu.emu_rng_keygen(pset, n, p8(r), pos & M64, p8(ek), p8(dk_a), p8(so)) == 0
    return ek, dk_a, so


def encaps(emu, pset, root, pos, ek):
    n = ek.shape[0]
    r = np.frombuffer(root, np.uint8).copy()
    c, K, st = np.full((n, SIZES[pset][2]), 0xAA, np.uint8), np.full((n, 32), 0xAA, np.uint8), np.full(n, 7, np.int32)
    assert emu.emu_rng_encaps(pset, n, p8(r), pos & M64, p8(ek), p8(c), p8(K), st.ctypes.data_as(i32p)) == 0
    return c, K, st


# (cap, hcap, small, lat, wide, n): n either side of the slice size (cap), of small_max and of the derivation-form switch
#   5 items, cap 2: slices 2 + 2 + 1, lane-sliced derivation, batch KeyGen / Encaps
#   3 items, cap 2, wide 1: slices 2 (lane-sliced) + 1 (wave-wide): the form switch inside one call
#   2 items, cap 2: exactly one slice ; 1 item: one short slice, wave-wide, the one-workgroup-per-item kernels (small 1)
SHAPES = ((2, 4, 0, 0, 0, 5), (2, 2, 0, 0, 1, 3), (2, 2, 0, 0, 2, 2), (2, 2, 1, 1, 1, 1))


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("fips", (0, 1))
def test_emu_random_keygen(emu, oracle, cfg, pset, fips):
    """seed_out equals the hashlib seeds, (ek, dk) the oracle's KeyGen on them, the dk = NULL mode returns the same ek and seeds; the
    regions read zero after every call (the emulator's own check)"""
    root, pos = ROOTS[1], (1 << 32) - 2
    try:
        for cap, hcap, small, lat, wide, n in SHAPES:
            cfg(cap=cap, hcap=hcap, small=small, lat=lat, wide=wide, fips=fips)
            want = blocks(root, DOM_KEYGEN, pos, n, 64)
            oracle.set_conformance(bool(fips))
            ek_o, dk_o = oracle.keygen(pset, np.ascontiguousarray(want[:, :32]), np.ascontiguousarray(want[:, 32:]))
            ek, dk, so = keygen(emu, pset, root, pos, n)
            assert (so == want).all(), n
            assert (ek == ek_o).all() and (dk == dk_o).all(), n
            ek2, _, so2 = keygen(emu, pset, root, pos, n, dk=False)
            assert (ek2 == ek_o).all() and (so2 == want).all(), n
            ek3, dk3, _ = keygen(emu, pset, root, pos, n, seed=False)
            assert (ek3 == ek_o).all() and (dk3 == dk_o).all(), n
    finally:
        oracle.set_conformance(False)


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("fips", (0, 1))
def test_emu_random_encaps(emu, oracle, cfg, pset, fips):
    """c, K equal the oracle's Encaps on the hashlib m; status is zero for valid keys in both modes"""
    root, pos = ROOTS[3], (1 << 64) - 2   # the counter wraps inside the call
    try:
        oracle.set_conformance(bool(fips))
        seed = blocks(ROOTS[2], DOM_KEYGEN, 0, 5, 64)
        ek_all, _ = oracle.keygen(pset, np.ascontiguousarray(seed[:, :32]), np.ascontiguousarray(seed[:, 32:]))
        for cap, hcap, small, lat, wide, n in SHAPES:
            cfg(cap=cap, hcap=hcap, small=small, lat=lat, wide=wide, fips=fips)
            ek = np.ascontiguousarray(ek_all[:n])
            m = blocks(root, DOM_ENCAPS, pos, n, 32)
            oracle.set_conformance(bool(fips))
            c_o, K_o = oracle.encaps(pset, ek, m)
            c, K, st = encaps(emu, pset, root, pos, ek)
            assert (c == c_o).all() and (K == K_o).all(), n
            assert not st.any()
    finally:
        oracle.set_conformance(False)


@pytest.mark.parametrize("fips", (0, 1))
def test_emu_split_invariance(emu, oracle, cfg, fips):
    """calls of 5 + 3 items give the items of one call of 8 (ML-KEM-768; cap 2: every call is sliced, the last slice of the 5 short)"""
    pset, root, pos = 768, ROOTS[1], 40
    try:
        cfg(cap=2, hcap=4, fips=fips)
        ek8, dk8, so8 = keygen(emu, pset, root, pos, 8)
        ek5, dk5, so5 = keygen(emu, pset, root, pos, 5)
        ek3, dk3, so3 = keygen(emu, pset, root, pos + 5, 3)
        assert (np.concatenate([ek5, ek3]) == ek8).all() and (np.concatenate([dk5, dk3]) == dk8).all()
        assert (np.concatenate([so5, so3]) == so8).all()
        c8, K8, _ = encaps(emu, pset, root, pos, ek8)
        c5, K5, _ = encaps(emu, pset, root, pos, np.ascontiguousarray(ek8[:5]))
        c3, K3, _ = encaps(emu, pset, root, pos + 5, np.ascontiguousarray(ek8[5:]))
        assert (np.concatenate([c5, c3]) == c8).all() and (np.concatenate([K5, K3]) == K8).all()
    finally:
        oracle.set_conformance(False)


def test_emu_fips_modulus_status(emu, oracle, cfg):
    """FIPS 203 mode: an ek with a coefficient >= q reports MLKEM_ERR_MODULUS for its item through the sliced call, like the seeded one"""
    pset, root = 768, ROOTS[1]
    try:
        oracle.set_conformance(True)
        seed = blocks(ROOTS[2], DOM_KEYGEN, 7, 3, 64)
        ek, _ = oracle.keygen(pset, np.ascontiguousarray(seed[:, :32]), np.ascontiguousarray(seed[:, 32:]))
        ek[2, 0], ek[2, 1] = 0xFF, ek[2, 1] | 0x0F          # coefficient 0 of item 2 = 0xFFF
        cfg(cap=2, hcap=2, fips=1)
        _, _, st = encaps(emu, pset, root, 0, ek)
        assert list(st) == [0, 0, -4]
        cfg(cap=2, hcap=2, fips=0)
        _, _, st = encaps(emu, pset, root, 0, ek)
        assert not st.any()
    finally:
        oracle.set_conformance(False)
