"""CPU tier: SHA-3 / SHAKE over messages of unequal length (mlkem_sha3r.hpp) on the host wave emulator.

tests/emu/emu_sha3r.cpp compiles both kernel forms from the product header -- k_sha3_ragged (one sponge per lane, form 0) and
k_sha3_ragged_w (one sponge per wavefront, form 1) -- and every call here forces one of them.  The expected value is always hashlib.
The emulator entry point records every message load the kernels issue and returns -3 when one is unaligned, wider than 16 bytes, or
holds no byte of the item's own head or body; -101 is the argument error of the C-ABI (the check is the one the library runs).
After every call the LDS the kernels report (the wave-wide form's round-constant table, cleared before the wave exits; the
lane-sliced form has none) must read zero.  Every call writes into rows of out_stride = outlen rounded up to 4, plus 12, pre-filled with a pattern: the gap must survive."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.timeout(3600, method="thread")
ERR_ARG = -101
# name -> (alg code, rate, digest length; 0 = any), hashlib constructor
ALGS = {"sha3_224": (0, 144, 28, hashlib.sha3_224), "sha3_256": (1, 136, 32, hashlib.sha3_256), "sha3_384": (2, 104, 48, hashlib.sha3_384),
        "sha3_512": (3, 72, 64, hashlib.sha3_512), "shake128": (4, 168, 0, hashlib.shake_128), "shake256": (5, 136, 0, hashlib.shake_256)}
FORMS = (0, 1)
PATTERN = 0xA5


def lengths(R):
    return [0, 1, 7, 8, 9, R - 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 3 * R + 5]


def want(alg, msg, outlen):
    h = ALGS[alg][3](msg)
    return h.digest(outlen) if ALGS[alg][2] == 0 else h.digest()


def aligned(nbytes, align=16, fill=None):
    """a uint8 array of nbytes whose first byte sits at an address that is 0 mod `align`"""
    raw = np.zeros(nbytes + align, np.uint8)
    skip = (-raw.ctypes.data) % align
    a = raw[skip:skip + nbytes]
    if fill is not None:
        a[:] = fill
    return a


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """the test-only TU, built with the compiler line of tests/test_rng_emu.py into a temporary directory"""
    out = str(tmp_path_factory.mktemp("emu_sha3r") / "libmlkem_emu_sha3r.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-attributes",
                        "-o", out, os.path.join(ge.ROOT, "tests", "emu", "emu_sha3r.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    vp, sz = C.c_void_p, C.c_size_t
    lib.emu_sha3r.argtypes = [C.c_int, C.c_int, sz, vp, C.c_uint, sz, vp, sz, vp, vp, vp, C.c_uint, sz, vp]
    lib.emu_sha3r_loads.restype = sz
    lib.emu_sha3r_lds_nonzero.restype = C.c_long
    return lib


def call(emu, form, alg, body_ptr, body_bytes, offs, lens, head=None, outlen=None, status=True, expect=0):
    """one emulator call -> (out rows [n, outlen], gap intact, status or None); asserts the return code and the LDS probe"""
    code, _, digest, _ = ALGS[alg]
    outlen = outlen or digest
    n = len(offs)
    off = np.array(offs, np.uint64)
    ln = np.array(lens, np.uint32)
    stride = (outlen + 3) // 4 * 4 + 12
    out = aligned(max(n, 1) * stride, fill=PATTERN)[:n * stride].reshape(n, stride)
    st = np.full(n, 7, np.int32) if status else None
    hp, hl, hs = (None, 0, 0) if head is None else (head.ctypes.data, head.shape[1], head.strides[0])
    rc = emu.emu_sha3r(form, code, n, hp, hl, hs, body_ptr, body_bytes, off.ctypes.data, ln.ctypes.data, out.ctypes.data, outlen, stride,
                       None if st is None else st.ctypes.data)
    assert rc == expect, (rc, form, alg)
    assert emu.emu_sha3r_lds_nonzero() == 0
    if form == 1 and rc == 0 and any(o <= body_bytes and l <= body_bytes - o for o, l in zip(offs, lens)):
        assert emu.emu_sha3r_lds_regions() == 1      # the wave-wide form's round-constant table was read back, not nothing
    return out[:, :outlen], bool((out[:, outlen:] == PATTERN).all()), st


def check(emu, form, alg, body, offs, lens, head=None, outlen=None, status=True):
    """a call in which every item is in bounds: every row equals hashlib over head[i] + body[off:off + len], the gap is intact"""
    code, _, digest, _ = ALGS[alg]
    outlen = outlen or digest
    out, gap_ok, st = call(emu, form, alg, body.ctypes.data if body.size else None, body.size, offs, lens, head, outlen, status)
    assert gap_ok
    for i, (o, l) in enumerate(zip(offs, lens)):
        msg = (head[i].tobytes() if head is not None else b"") + body[o:o + l].tobytes()
        assert out[i].tobytes() == want(alg, msg, outlen), (form, alg, i, o, l, 0 if head is None else head.shape[1])
    if st is not None:
        assert not st.any()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("alg", sorted(ALGS))
def test_length_by_alignment_matrix(emu, alg, form):
    """the 13 lengths around the rate at each of the 16 body start alignments mod 16: 208 messages in one call"""
    R = ALGS[alg][1]
    rng = np.random.default_rng(R + form)
    body = aligned(208 * (3 * R + 5 + 32))
    body[:] = rng.integers(0, 256, body.size, dtype=np.uint8)
    offs, lens, pos = [], [], 0
    for L in lengths(R):
        for a in range(16):
            pos += (a - pos) % 16           # address of the first byte = a mod 16
            offs.append(pos)
            lens.append(L)
            pos += L
    check(emu, form, alg, body, offs, lens, outlen=None if ALGS[alg][2] else 32)
    assert emu.emu_sha3r_loads() > 0


@pytest.mark.parametrize("form,algs", ((0, sorted(ALGS)), (1, ("sha3_512", "shake256"))))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_batch_sizes(emu, n, form, algs):
    """n either side of a wavefront, random lengths in [0, R + 40] packed back to back (every start alignment occurs)"""
    for alg in algs:
        R = ALGS[alg][1]
        rng = np.random.default_rng(1000 * n + R)
        lens = [int(x) for x in rng.integers(0, R + 41, n)]
        offs = [int(x) for x in np.cumsum([3] + lens[:-1])]
        body = aligned(3 + sum(lens) + 1)
        body[:] = rng.integers(0, 256, body.size, dtype=np.uint8)
        check(emu, form, alg, body, offs, lens, outlen=None if ALGS[alg][2] else 40)


@pytest.mark.parametrize("alg", ("sha3_256", "shake128"))
def test_one_long_lane_among_empty_ones_and_the_converse(emu, alg):
    """lane 17 absorbs 5 blocks while every other lane of its wave has an empty message, and one empty lane among long ones: a lane
    that is done keeps its output through the permutations the wave still runs"""
    R = ALGS[alg][1]
    rng = np.random.default_rng(17)
    body = aligned(64 * (4 * R + 3) + 8)
    body[:] = rng.integers(0, 256, body.size, dtype=np.uint8)
    long_len = 4 * R + 3                                     # total / R + 1 = 5 blocks
    lens = [long_len if i == 17 else 0 for i in range(64)]
    offs = [5 if i == 17 else i for i in range(64)]
    for form in FORMS:
        check(emu, form, alg, body, offs, lens, outlen=None if ALGS[alg][2] else 2 * R + 5)
    lens = [0 if i == 17 else long_len - (i % 3) for i in range(64)]
    offs = [i * (4 * R + 3) for i in range(64)]
    check(emu, 0, alg, body, offs, lens, outlen=None if ALGS[alg][2] else 2 * R + 5)


@pytest.mark.parametrize("form", FORMS)
def test_offsets_descending_overlapping_repeated(emu, form):
    rng = np.random.default_rng(3)
    body = aligned(700)
    body[:] = rng.integers(0, 256, body.size, dtype=np.uint8)
    offs = [600, 450, 450, 300, 301, 302, 0, 0, 699, 700, 137]
    lens = [100, 200, 200, 250, 250, 9, 700, 0, 1, 0, 136]
    for alg in ("sha3_256", "sha3_384", "shake256"):
        check(emu, form, alg, body, offs, lens, outlen=None if ALGS[alg][2] else 64)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("alg", sorted(ALGS))
def test_heads(emu, alg, form):
    """head_len in {0, 32, 64, R - 8, R, R + 8} with empty and non-empty bodies (a head ending on a block boundary, a body starting
    mid-block), the head rows taken from a wider array (row stride != head_len)"""
    R = ALGS[alg][1]
    rng = np.random.default_rng(R)
    body_lens = [0, 5, R - 1, R + 1]
    body = aligned(sum(body_lens) + 16)
    body[:] = rng.integers(0, 256, body.size, dtype=np.uint8)
    offs = [int(x) for x in np.cumsum([1] + body_lens[:-1])]
    for hl in (0, 32, 64, R - 8, R, R + 8):
        wide = aligned(len(body_lens) * (hl + 24)).reshape(len(body_lens), hl + 24)
        wide[:] = rng.integers(0, 256, wide.shape, dtype=np.uint8)
        head = wide[:, :hl] if hl else None
        check(emu, form, alg, body, offs, body_lens, head=head, outlen=None if ALGS[alg][2] else 48)
    # a head on its own: no body buffer at all
    head = aligned(3 * 64).reshape(3, 64)
    head[:] = rng.integers(0, 256, head.shape, dtype=np.uint8)
    check(emu, form, alg, np.zeros(0, np.uint8), [0, 0, 0], [0, 0, 0], head=head, outlen=None if ALGS[alg][2] else 48)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("alg", ("shake128", "shake256"))
def test_shake_output_lengths(emu, alg, form):
    R = ALGS[alg][1]
    rng = np.random.default_rng(R + 7)
    lens = [0, R - 1, 2 * R + 1]
    body = aligned(sum(lens) + 2)
    body[:] = rng.integers(0, 256, body.size, dtype=np.uint8)
    offs = [2, 2, 2 + R - 1]
    for outlen in (1, 3, 32, R - 1, R, R + 1, 2 * R + 5):
        check(emu, form, alg, body, offs, lens, outlen=outlen, status=outlen % 2 == 0)


@pytest.mark.parametrize("form", FORMS)
def test_out_of_bounds_items(emu, form):
    """one and several out-of-bounds items amid valid ones (the sum must not wrap at 2^64): zero rows, status -101, neighbours right;
    with and without a status array"""
    rng = np.random.default_rng(5)
    body = aligned(300)
    body[:] = rng.integers(0, 256, body.size, dtype=np.uint8)
    M64 = (1 << 64) - 1
    cases = (([0, 290, 100], [10, 11, 20], {1}),
             ([M64, 0, 301, 299, 300, 200, M64 - 5, 7], [1, 300, 0, 2, 0, 100, 6, 293], {0, 2, 3, 6}),
             ([M64] * 3, [0xFFFFFFFF, 2, 0], {0, 1, 2}))
    for alg in ("sha3_256", "shake128"):
        outlen = ALGS[alg][2] or 200
        for offs, lens, bad in cases:
            for status in (True, False):
                out, gap_ok, st = call(emu, form, alg, body.ctypes.data, body.size, offs, lens, outlen=outlen, status=status)
                assert gap_ok
                for i, (o, l) in enumerate(zip(offs, lens)):
                    if i in bad:
                        assert not out[i].any(), (alg, i)
                    else:
                        assert out[i].tobytes() == want(alg, body[o:o + l].tobytes(), outlen), (alg, i)
                if status:
                    assert list(st) == [ERR_ARG if i in bad else 0 for i in range(len(offs))]
    # a message of 2^31 bytes or more is refused per item like an out-of-bounds one (body_bytes says the buffer is that large; no
    # byte of it is read)
    head = aligned(64).reshape(1, 64)
    out, gap_ok, st = call(emu, form, "sha3_256", body.ctypes.data, 1 << 32, [0], [(1 << 31) - 64], head=head)
    assert gap_ok and not out.any() and list(st) == [ERR_ARG]
    assert emu.emu_sha3r_loads() == 0


@pytest.mark.parametrize("form", FORMS)
def test_bodies_at_both_ends_of_an_allocation(emu, form):
    """the body's first byte is the first byte of a malloc'ed buffer and its last byte the last byte of one, at buffer sizes that
    leave the end at every position of an aligned qword; items that end (and begin) exactly there"""
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    libc.malloc.argtypes = [C.c_size_t]
    libc.free.argtypes = [C.c_void_p]
    rng = np.random.default_rng(11)
    for size in (1, 7, 8, 9, 137, 271, 300, 413):
        p = libc.malloc(size)
        assert p
        try:
            data = rng.integers(0, 256, size, dtype=np.uint8)
            C.memmove(p, data.ctypes.data, size)
            tails = sorted({1, min(size, 5), min(size, 8), min(size, 136), size})
            offs = [0] + [size - t for t in tails] + [size]
            lens = [size] + tails + [0]
            for alg in ("sha3_256", "shake128"):
                outlen = ALGS[alg][2] or 32
                out, gap_ok, st = call(emu, form, alg, p, size, offs, lens, outlen=outlen)
                assert gap_ok and not st.any()
                for i, (o, l) in enumerate(zip(offs, lens)):
                    assert out[i].tobytes() == want(alg, data[o:o + l].tobytes(), outlen), (size, alg, i)
        finally:
            libc.free(p)


def test_zero_items_and_argument_errors(emu):
    body = aligned(64)
    for form in FORMS:
        out, gap_ok, st = call(emu, form, "sha3_256", body.ctypes.data, 64, [], [])          # n = 0: a no-op
        assert out.shape[0] == 0
        assert emu.emu_sha3r(form, 1, 0, None, 0, 0, None, 0, None, None, None, 32, 32, None) == 0
    code = ALGS["sha3_256"][0]
    off, ln = np.zeros(1, np.uint64), np.full(1, 8, np.uint32)
    out = aligned(64, fill=PATTERN)
    head = aligned(64)
    args = lambda **kw: [kw.get(k, d) for k, d in (("form", 0), ("alg", code), ("n", 1), ("head", None), ("head_len", 0), ("head_stride", 0),
                                                    ("body", body.ctypes.data), ("body_bytes", 64), ("off", off.ctypes.data), ("len", ln.ctypes.data),
                                                    ("out", out.ctypes.data), ("outlen", 32), ("out_stride", 32), ("status", None))]
    assert emu.emu_sha3r(*args()) == 0
    out[:] = PATTERN
    bad = (dict(alg=6), dict(alg=-1), dict(outlen=31), dict(outlen=0), dict(alg=4, outlen=0), dict(alg=5, outlen=65537),
           dict(out=None), dict(off=None), dict(len=None), dict(body=None), dict(out=out.ctypes.data + 8), dict(out_stride=34),
           dict(out_stride=28), dict(off=off.ctypes.data + 4), dict(len=ln.ctypes.data + 2),
           dict(head=head.ctypes.data, head_len=12, head_stride=16), dict(head=head.ctypes.data + 4, head_len=8, head_stride=8),
           dict(head=head.ctypes.data, head_len=16, head_stride=8), dict(head=head.ctypes.data, head_len=8, head_stride=12))
    for kw in bad:
        assert emu.emu_sha3r(*args(**kw)) == ERR_ARG, kw
    assert (out == PATTERN).all()
