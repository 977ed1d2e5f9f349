"""CPU tier: SP 800-185 cSHAKE / KMAC over messages of unequal length (mlkem_kmac.hpp) on the host wave emulator.

tests/emu/emu_kmac.cpp compiles the three kernels from the product header -- k_kmac_prefix, k_kmac_ragged (one sponge per lane,
form 0) and k_kmac_ragged_w (one sponge per wavefront, form 1) -- sequenced by the product's kmac_launch; every call here forces one
form.  The expected value is always the independent restatement tests/sp800185_py.py (pinned against hashlib and the NIST samples in
tests/test_kmac_abi.py and once more here).  The emulator entry points record every message and key load the kernels issue and
return -3 when one is not a naturally aligned 8-byte load holding a byte of the item's own key, head or body (of the shared key for
the prefix kernel); -101 is the argument error of the C-ABI (the check is the one the library runs).  After every call the LDS the
kernels report must read zero, after a shared-key call the midstate region too.  Every call writes into rows of out_stride = outlen
rounded up to 4, plus 12, pre-filled with a pattern: the gap must survive."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import sp800185_py as sp

pytestmark = pytest.mark.timeout(3600, method="thread")
ERR_ARG = -101
FORMS = (0, 1)
BITS = (128, 256)
PATTERN = 0xA5


def aligned(nbytes, align=16, fill=None):
    """a uint8 array of nbytes whose first byte sits at an address that is 0 mod `align`"""
    raw = np.zeros(nbytes + align, np.uint8)
    skip = (-raw.ctypes.data) % align
    a = raw[skip:skip + nbytes]
    if fill is not None:
        a[:] = fill
    return a


def rand(rng, *shape):
    a = aligned(int(np.prod(shape))).reshape(shape)
    a[...] = rng.integers(0, 256, shape, dtype=np.uint8)
    return a


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """the test-only TU, built with the compiler line of tests/test_sha3r_emu.py into a temporary directory"""
    sp.check_pinned()
    out = str(tmp_path_factory.mktemp("emu_kmac") / "libmlkem_emu_kmac.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-Wno-attributes",
                        "-o", out, os.path.join(ge.ROOT, "tests", "emu", "emu_kmac.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    lib.emu_cshake.argtypes = [C.c_int, C.c_int, sz, vp, u, vp, u, vp, u, vp, u, sz, vp, sz, vp, vp, vp, u, sz, vp]
    lib.emu_kmac.argtypes = [C.c_int, C.c_int, sz, vp, u, sz, vp, u, vp, u, vp, u, sz, vp, sz, vp, vp, vp, u, sz, vp]
    lib.emu_kmac_loads.restype = sz
    lib.emu_kmac_lds_nonzero.restype = C.c_long
    lib.emu_kmac_mid_nonzero.restype = C.c_long
    return lib


def call(emu, form, bits, body, offs, lens, *, outlen, key=None, fname=b"", custom=b"", lead=b"", head=None, xof=False, status=True,
         expect=0, body_bytes=None):
    """one emulator call -> (out rows [n, outlen], gap intact, status or None).  key: None = cSHAKE; a 2-D array (view) = per-item
    keys used in place; a 1-D array = one shared key.  Asserts the return code, the LDS probe and the midstate rule."""
    n = len(offs)
    off, ln = np.array(offs, np.uint64), np.array(lens, np.uint32)
    stride = (outlen + 3) // 4 * 4 + 12
    out = aligned(max(n, 1) * stride, fill=PATTERN)[:n * stride].reshape(n, stride)
    st = np.full(n, 7, np.int32) if status else None
    hp, hl, hs = (None, 0, 0) if head is None else (head.ctypes.data, head.shape[1], head.strides[0])
    bp = body.ctypes.data if body is not None and body.size else None
    bb = (body.size if body is not None else 0) if body_bytes is None else body_bytes
    tail = (bytes(lead), len(lead), hp, hl, hs, bp, bb, off.ctypes.data, ln.ctypes.data, out.ctypes.data, outlen, stride,
            None if st is None else st.ctypes.data)
    if key is None:
        rc = emu.emu_cshake(form, bits, n, bytes(fname), len(fname), bytes(custom), len(custom), *tail)
    else:
        kp, kl, ks = (key.ctypes.data if key.size else None, key.size, 0) if key.ndim == 1 else (key.ctypes.data, key.shape[1], key.strides[0])
        rc = emu.emu_kmac(form, (bits == 256) + 2 * bool(xof), n, kp, kl, ks, bytes(custom), len(custom), *tail)
    assert rc == expect, (rc, form, bits)
    assert emu.emu_kmac_lds_nonzero() == 0
    if key is not None and key.ndim == 1 and rc == 0:
        assert emu.emu_kmac_mid_nonzero() == 0           # key-equivalent: zeroed behind the call's last kernel
    return out[:, :outlen], bool((out[:, outlen:] == PATTERN).all()), st


def want(bits, X, outlen, key=None, fname=b"", custom=b"", xof=False):
    if key is None:
        return sp.cshake(bits, X, outlen, fname, custom)
    return sp.kmac(bits, key, X, outlen, custom, xof)


def check(emu, form, bits, body, offs, lens, *, outlen, key=None, fname=b"", custom=b"", lead=b"", head=None, xof=False, status=True):
    """a call in which every item is in bounds: every row equals the restatement over lead + head[i] + body[off:off + len]"""
    out, gap_ok, st = call(emu, form, bits, body, offs, lens, outlen=outlen, key=key, fname=fname, custom=custom, lead=lead, head=head,
                           xof=xof, status=status)
    assert gap_ok
    for i, (o, l) in enumerate(zip(offs, lens)):
        X = bytes(lead) + (head[i].tobytes() if head is not None else b"") + body[o:o + l].tobytes()
        k = None if key is None else (key.tobytes() if key.ndim == 1 else key[i].tobytes())
        assert out[i].tobytes() == want(bits, X, outlen, k, fname, custom, xof), (form, bits, i, o, l, len(lead))
    if st is not None:
        assert not st.any()


def take(idx, offs, lens, *rows):
    """items idx of a call: offsets, lengths and (16-byte aligned copies of) the given per-item rows.  The wave-wide form costs the
    emulator 64 threads and ~14 barriers per round for ONE item, so its calls take the items that differ, not every combination."""
    out = [[offs[i] for i in idx], [lens[i] for i in idx]]
    for r in rows:
        c = aligned(len(idx) * r.shape[1]).reshape(len(idx), r.shape[1])
        c[:] = r[list(idx)]
        out.append(c)
    return out


def spread(lens, first=0):
    """offsets that put message i at an address that is first + i mod 8 (the body buffer is 16-byte aligned)"""
    offs, pos = [], 0
    for i, l in enumerate(lens):
        pos += (first + i - pos) % 8
        offs.append(pos)
        pos += l
    return offs, pos


@pytest.mark.parametrize("form", FORMS)
def test_nist_samples(emu, form):
    """the sample values of SP 800-185 through the kernels: X as the body, K as a per-item key row and as the shared key"""
    body = aligned(208)
    body[:200] = np.arange(200, dtype=np.uint8)
    for fn, args, hexval in sp.SAMPLES:
        bits = args[0]
        xlen, outlen = (len(args[1]), args[2]) if fn is sp.cshake else (len(args[2]), args[3])
        if fn is sp.cshake:
            out, _, _ = call(emu, form, bits, body, [0], [xlen], outlen=outlen, fname=args[3], custom=args[4])
            assert out[0].tobytes().hex().upper() == hexval
            continue
        key = aligned(32).reshape(1, 32)
        key[0] = np.frombuffer(sp.K_SAMPLE, np.uint8)
        for k in (key, key[0]):
            out, _, _ = call(emu, form, bits, body, [0], [xlen], outlen=outlen, key=k, custom=args[4], xof=len(args) > 5)
            assert out[0].tobytes().hex().upper() == hexval, (bits, xlen, k.ndim)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bits", BITS)
def test_tail_around_block_boundaries(emu, bits, form):
    """totals lead + head + body = b R + r for r = R - 6 .. R + 1 and b = 0, 1, 2 full blocks before: the (up to 5-byte) tail
    right_encode(L) || 04 lies inside a block, ends exactly at its end, and straddles the boundary; bodies at every address mod 8"""
    R = sp.rate_of(bits)
    rng = np.random.default_rng(R + form)
    totals = [b * R + r for b in range(3) for r in range(R - 6, R + 2)]
    head = rand(rng, len(totals), 32)
    keys = rand(rng, len(totals), 32)
    lens = [t - 36 for t in totals]
    offs, size = spread(lens)
    body = rand(rng, size)
    lead = b"\x00\x00\x00\x01"
    check(emu, form, bits, body, offs, lens, outlen=32, key=keys, custom=b"KDF", lead=lead, head=head)             # 4-byte tail
    # the other tail widths: every total in the lane-sliced form; in the wave-wide form the totals around the first boundary
    o, l, k, h = take(range(len(lens)) if form == 0 else range(8), offs, lens, keys, head)
    check(emu, form, bits, body, o, l, outlen=32, key=k[0], custom=b"KDF", lead=lead, head=h, xof=True)            # 3 bytes: 00 01 04
    check(emu, form, bits, body, o, l, outlen=40, custom=b"S", lead=lead, head=h)                                  # cSHAKE: 1 byte
    # L = 2^16 bits: the 5-byte tail 01 00 00 03 04 (61 squeezed blocks per item: in the wave-wide form the two items whose tail
    # ends exactly with the first block and straddles its end by four bytes)
    o5, l5, k5, h5 = take(range(len(lens)) if form == 0 else (1, 5), offs, lens, keys, head)
    check(emu, form, bits, body, o5, l5, outlen=8192, key=k5, lead=lead, head=h5, status=False)
    # without lead and head the totals are the body lengths
    o, l, k = take(range(len(totals)) if form == 0 else range(8, 16), *spread(totals, first=3)[:1], totals, keys)
    body = rand(rng, spread(totals, first=3)[1])
    check(emu, form, bits, body, o, l, outlen=32, key=k, custom=b"x")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bits", BITS)
def test_lead_head_and_body_alignment(emu, bits, form):
    """lead_len 0, 4, 8 (and 1, 7) with and without a head of 32 bytes, bodies of length 0, 1, 9 and R - 1 at addresses 0..7 mod 8"""
    R = sp.rate_of(bits)
    rng = np.random.default_rng(R + 10 * form)
    lens = [l for l in (0, 1, 9, R - 1) for _ in range(8)]
    offs, size = spread(lens)
    body = rand(rng, size)
    wide = rand(rng, len(lens), 40)
    keys = rand(rng, len(lens), 32)
    for lead_len in (0, 4, 8, 1, 7):
        lead = bytes(range(0xF1, 0xF1 + lead_len))
        for head in (None, wide[:, :32]):
            if form == 0:
                check(emu, form, bits, body, offs, lens, outlen=32, key=keys, custom=b"c", lead=lead, head=head)
                check(emu, form, bits, body, offs, lens, outlen=32, custom=b"c", lead=lead, head=head)
            elif lead_len in (0, 4, 8):
                # the wave-wide form: eight items, one per address mod 8, the four lengths twice; KMAC with the head, cSHAKE without
                idx = [i + 8 * (i % 4) for i in range(8)]
                o, l, k = take(idx, offs, lens, keys)
                if head is None:
                    check(emu, form, bits, body, o, l, outlen=32, custom=b"c", lead=lead)
                else:
                    check(emu, form, bits, body, o, l, outlen=32, key=k, custom=b"c", lead=lead, head=take(idx, offs, lens, head)[2])
    # a lead and a head on their own: no body buffer at all
    check(emu, form, bits, np.zeros(0, np.uint8), [0, 0], [0, 0], outlen=32, key=keys[:2], lead=b"\x01\x02\x03\x04", head=wide[:2, :32])
    check(emu, form, bits, np.zeros(0, np.uint8), [0], [0], outlen=32, key=keys[:1])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bits", BITS)
def test_per_item_keys(emu, bits, form):
    """key_len 8, 24 (4-byte header), 32, 64, 128 (5-byte header), the rows a strided view of a wider array"""
    R = sp.rate_of(bits)
    rng = np.random.default_rng(R + 20 * form)
    lens = [0, 5, 64, R - 4, R + 9]
    offs, size = spread(lens, first=5)
    body = rand(rng, size)
    wide = rand(rng, len(lens), 136)
    if form == 1:
        offs, lens, wide = offs[1:4], lens[1:4], wide[1:4]
    for kl in (8, 24, 32, 64, 128):
        check(emu, form, bits, body, offs, lens, outlen=32, key=wide[:, :kl], custom=b"My Tagged Application")
        if form == 0 or kl in (24, 128):
            check(emu, form, bits, body, offs, lens, outlen=32, key=wide[:, 8:8 + kl], lead=b"\x00\x00\x00\x01", xof=True)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bits", BITS)
def test_shared_keys(emu, bits, form):
    """one key of 0, 1, 32, 132, 164 and 200 bytes (two key blocks at R = 136) for all items, at an aligned and an odd address"""
    R = sp.rate_of(bits)
    rng = np.random.default_rng(R + 30 * form)
    lens = [0, 3, 64, R + 1]
    offs, size = spread(lens, first=1)
    body = rand(rng, size)
    store = rand(rng, 540)
    if form == 1:
        offs, lens = offs[2:], lens[2:]
    for j, kl in enumerate((0, 1, 32, 132, 164, 200, 512)):
        for at in ((0, 3) if form == 0 else (3 * (j % 2),)):
            check(emu, form, bits, body, offs, lens, outlen=48, key=store[at:at + kl], custom=b"KDF", lead=b"\x00\x00\x00\x01")
    zero = aligned(164)
    check(emu, form, bits, body, offs, lens, outlen=32, key=zero[:164 if bits == 128 else 132], custom=b"KDF")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bits", BITS)
def test_function_name_and_customisation(emu, bits, form):
    """S of 0, 1, 40 and 256 bytes, N = "" and 32 bytes: one to three prefix blocks; N = S = "" is SHAKE (hashlib)"""
    R = sp.rate_of(bits)
    rng = np.random.default_rng(R + 40 * form)
    lens = [0, 7, R - 1, R]
    offs, size = spread(lens, first=2)
    body = rand(rng, size)
    key = rand(rng, len(lens), 32)
    if form == 1:
        offs, lens, key = offs[2:], lens[2:], take((2, 3), offs, lens, key)[2]
    for S in (b"", b"s", bytes(range(40)), bytes(i & 0xFF for i in range(256))):
        for N in (b"", bytes(range(100, 132))):
            check(emu, form, bits, body, offs, lens, outlen=32, fname=N, custom=S)
        check(emu, form, bits, body, offs, lens, outlen=32, key=key, custom=S)
    out, gap_ok, _ = call(emu, form, bits, body, offs, lens, outlen=50, lead=b"ab")
    shake = hashlib.shake_128 if bits == 128 else hashlib.shake_256
    for i, (o, l) in enumerate(zip(offs, lens)):
        assert out[i].tobytes() == shake(b"ab" + body[o:o + l].tobytes()).digest(50), i
    assert gap_ok


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bits", BITS)
def test_output_lengths(emu, bits, form):
    R = sp.rate_of(bits)
    rng = np.random.default_rng(R + 50 * form)
    lens = [0, R - 1, 2 * R + 1]
    offs, size = spread(lens, first=6)
    body = rand(rng, size)
    key = rand(rng, len(lens), 32)
    if form == 1:
        offs, lens, key = offs[:2], lens[:2], take((0, 1), offs, lens, key)[2]
    for outlen in (1, 32, R, R + 1, 2 * R + 3):
        for xof in (False, True):
            check(emu, form, bits, body, offs, lens, outlen=outlen, key=key, custom=b"o", xof=xof, status=outlen % 2 == 0)
        if form == 0 or outlen in (1, 2 * R + 3):
            check(emu, form, bits, body, offs, lens, outlen=outlen, custom=b"o")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n", (1, 64, 130))
def test_lane_sliced_batches_of_mixed_lengths(emu, n, bits):
    """1, 64 and 130 items in the lane-sliced form, lengths in [0, 2 R + 40] mixed within a wave: short lanes finish (and keep
    their output) while long ones run"""
    R = sp.rate_of(bits)
    rng = np.random.default_rng(1000 * n + R)
    lens = [int(x) for x in rng.integers(0, 2 * R + 41, n)]
    lens[0] = 0
    offs = [int(x) for x in np.cumsum([3] + lens[:-1])]
    body = rand(rng, 3 + sum(lens) + 1)
    keys = rand(rng, n, 32)
    check(emu, 0, bits, body, offs, lens, outlen=R + 5, key=keys, custom=b"KDF", lead=b"\x00\x00\x00\x01", head=rand(rng, n, 32))
    assert emu.emu_kmac_loads() > 0
    check(emu, 0, bits, body, offs, lens, outlen=32, key=keys[0], custom=b"KDF")
    check(emu, 0, bits, body, offs, lens, outlen=32, fname=b"N", custom=b"S", lead=b"\x09")


@pytest.mark.parametrize("form", FORMS)
def test_offsets_descending_overlapping_repeated(emu, form):
    rng = np.random.default_rng(3)
    body = rand(rng, 700)
    offs = [600, 450, 450, 300, 301, 302, 0, 0, 699, 700, 137]
    lens = [100, 200, 200, 250, 250, 9, 700, 0, 1, 0, 136]
    keys = rand(rng, len(offs), 32)
    for bits in (BITS if form == 0 else (256,)):
        check(emu, form, bits, body, offs, lens, outlen=64, key=keys, lead=b"\x00\x00\x00\x01")


@pytest.mark.parametrize("form", FORMS)
def test_out_of_bounds_items(emu, form):
    """bad items (offset outside, off + len wrapping at 2^64) between good ones: zero rows, status -101, neighbours right; with and
    without a status array; a message of 2^31 bytes or more is refused per item and reads nothing"""
    rng = np.random.default_rng(5)
    body = rand(rng, 300)
    M64 = (1 << 64) - 1
    offs, lens, bad = [M64, 0, 301, 299, 300, 200, M64 - 5, 7], [1, 300, 0, 2, 0, 100, 6, 293], {0, 2, 3, 6}
    keys = rand(rng, len(offs), 32)
    for bits in (BITS if form == 0 else (256,)):
        for key in (keys, keys[0], None):
            for status in ((True, False) if key is keys else (True,)):
                outlen = 200 if form == 0 else 40
                out, gap_ok, st = call(emu, form, bits, body, offs, lens, outlen=outlen, key=key, custom=b"b", lead=b"\x07", status=status)
                assert gap_ok
                for i, (o, l) in enumerate(zip(offs, lens)):
                    if i in bad:
                        assert not out[i].any(), (bits, i)
                    else:
                        k = None if key is None else (key.tobytes() if key.ndim == 1 else key[i].tobytes())
                        assert out[i].tobytes() == want(bits, b"\x07" + body[o:o + l].tobytes(), outlen, k, b"", b"b"), (bits, i)
                if status:
                    assert list(st) == [ERR_ARG if i in bad else 0 for i in range(len(offs))]
    head = aligned(64).reshape(1, 64)
    out, gap_ok, st = call(emu, form, 256, body, [0], [(1 << 31) - 64 - 4], outlen=32, key=keys[:1], lead=b"\x00\x00\x00\x01", head=head,
                           body_bytes=1 << 32)
    assert gap_ok and not out.any() and list(st) == [ERR_ARG]
    assert emu.emu_kmac_loads() == 0


def test_zero_items_and_argument_errors(emu):
    body = aligned(64)
    key = aligned(2 * 40).reshape(2, 40)
    for form in FORMS:
        out, _, _ = call(emu, form, 256, body, [], [], outlen=32, key=key[:0, :32])        # n = 0: a no-op
        assert out.shape[0] == 0
    off, ln = np.zeros(1, np.uint64), np.full(1, 8, np.uint32)
    out = aligned(64, fill=PATTERN)
    head = aligned(64)
    S = b"custom"
    base = dict(form=0, alg=1, n=1, key=key.ctypes.data, key_len=32, key_stride=40, custom=S, custom_len=len(S), lead=b"\x01\x02", lead_len=2,
                head=None, head_len=0, head_stride=0, body=body.ctypes.data, body_bytes=64, off=off.ctypes.data, len=ln.ctypes.data,
                out=out.ctypes.data, outlen=32, out_stride=32, status=None)
    order = list(base)
    assert emu.emu_kmac(*[base[k] for k in order]) == 0
    out[:] = PATTERN
    bad = (dict(alg=4), dict(alg=-1), dict(outlen=0), dict(outlen=65537, out_stride=65540), dict(key_len=0), dict(key_len=12), dict(key_len=136, key_stride=136),
           dict(key_len=40, key_stride=32), dict(key_stride=36), dict(key=key.ctypes.data + 4), dict(key=None), dict(key_stride=0, key_len=513),
           dict(key_stride=0, key=None), dict(custom_len=257), dict(custom=None), dict(lead_len=9), dict(lead=None),
           dict(out=None), dict(off=None), dict(len=None), dict(body=None), dict(out=out.ctypes.data + 8), dict(out_stride=34),
           dict(out_stride=28), dict(off=off.ctypes.data + 4), dict(len=ln.ctypes.data + 2),
           dict(head=head.ctypes.data, head_len=12, head_stride=16), dict(head=head.ctypes.data + 4, head_len=8, head_stride=8),
           dict(head=head.ctypes.data, head_len=16, head_stride=8), dict(head=head.ctypes.data, head_len=8, head_stride=12))
    for kw in bad:
        assert emu.emu_kmac(*[dict(base, **kw)[k] for k in order]) == ERR_ARG, kw
    cbase = dict(form=0, bits=128, n=1, fname=b"N", fname_len=1, custom=S, custom_len=len(S), lead=b"", lead_len=0, head=None, head_len=0,
                 head_stride=0, body=body.ctypes.data, body_bytes=64, off=off.ctypes.data, len=ln.ctypes.data, out=out.ctypes.data, outlen=32,
                 out_stride=32, status=None)
    corder = list(cbase)
    for kw in (dict(bits=192), dict(bits=0), dict(fname_len=33), dict(fname=None), dict(custom_len=257), dict(outlen=0), dict(out=None),
               dict(lead_len=9, lead=bytes(9))):
        assert emu.emu_cshake(*[dict(cbase, **kw)[k] for k in corder]) == ERR_ARG, kw
    assert (out == PATTERN).all()
    assert emu.emu_cshake(*[cbase[k] for k in corder]) == 0
    assert out[:32].tobytes() == sp.cshake(128, bytes(8), 32, b"N", S)
