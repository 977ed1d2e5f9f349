"""GPU tier (-m gpu): SP 800-185 cSHAKE / KMAC over device-resident messages of unequal length -- mlkem_cshake_dev / mlkem_kmac_dev
through MLKEM.cshake / MLKEM.kmac / MLKEM.kdf_onestep, the host-pointer calls, and a captured graph.  The expected value is always
the restatement tests/sp800185_py.py (pinned against hashlib and the NIST samples by tests/test_kmac_abi.py), computed once per case
and shared by the two engines: the default one, which takes the wave-wide form at these sizes, and one created with
MLKEM_SHA3_WIDE_ITEMS=0, which takes the lane-sliced form.  The matrix is the CPU tier's (tests/test_kmac_emu.py), n <= 200 per call."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import sp800185_py as sp

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
ERR_ARG = -101
BITS = (128, 256)
_WANT = {}


def want(bits, X, outlen, key=None, fname=b"", custom=b"", xof=False):
    k = (bits, X, outlen, key, fname, custom, xof)
    if k not in _WANT:
        _WANT[k] = sp.cshake(bits, X, outlen, fname, custom) if key is None else sp.kmac(bits, key, X, outlen, custom, xof)
    return _WANT[k]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"
    return torch


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    p = ge.load_package()
    p.load_library()
    return p


@pytest.fixture(scope="module")
def engines(pkg, torch):
    """(default engine, engine that always runs the lane-sliced form)"""
    default = pkg.MLKEM(768, device=0, chunk_items=1024)
    old = os.environ.get("MLKEM_SHA3_WIDE_ITEMS")
    os.environ["MLKEM_SHA3_WIDE_ITEMS"] = "0"
    try:
        lanes = pkg.MLKEM(768, device=0, chunk_items=1024)
    finally:
        if old is None:
            del os.environ["MLKEM_SHA3_WIDE_ITEMS"]
        else:
            os.environ["MLKEM_SHA3_WIDE_ITEMS"] = old
    assert default.sha3_wide_max >= 200 and lanes.sha3_wide_max == 0
    yield default, lanes
    default.close()
    lanes.close()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def spread(lens, first=0):
    """offsets that put message i at an address that is first + i mod 8 (torch allocations are 256-byte aligned)"""
    offs, pos = [], 0
    for i, l in enumerate(lens):
        pos += (first + i - pos) % 8
        offs.append(pos)
        pos += l
    return offs, pos


def run(torch, eng, bits, body, offs, lens, *, outlen, key=None, key_view=None, fname=b"", custom=b"", lead=b"", head=None, head_view=None,
        xof=False, bad=()):
    """MLKEM.cshake (key None) / MLKEM.kmac on an in-place body tensor; every row against the restatement (zero row and status -101 for
    the items in `bad`).  key / head: host arrays (2-D: per item; key 1-D: shared); key_view / head_view: the device tensors to pass
    instead of fresh copies of them."""
    bt = dev(torch, body)
    ot, lt = dev(torch, np.array(offs, np.uint64).view(np.int64)), dev(torch, np.array(lens, np.uint32).view(np.int32))
    ht = head_view if head_view is not None else (None if head is None else dev(torch, head))
    if key is None:
        out, st = eng.cshake(bits, bt, ot, lt, head=ht, lead=lead, outlen=outlen, function_name=fname, custom=custom, return_status=True)
    else:
        kt = key_view if key_view is not None else dev(torch, key)
        out, st = eng.kmac(bits, kt, bt, ot, lt, head=ht, lead=lead, outlen=outlen, custom=custom, xof=xof, return_status=True)
    torch.cuda.synchronize()
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert out.shape == (len(offs), outlen)
    for i, (o, l) in enumerate(zip(offs, lens)):
        if i in bad:
            assert not out[i].any() and st[i] == ERR_ARG, i
            continue
        X = bytes(lead) + (head[i].tobytes() if head is not None else b"") + body[o:o + l].tobytes()
        k = None if key is None else (key.tobytes() if key.ndim == 1 else key[i].tobytes())
        assert out[i].tobytes() == want(bits, X, outlen, k, fname, custom, xof), (bits, i, o, l, len(lead), outlen)
        assert st[i] == 0


@pytest.mark.parametrize("lane_form", (False, True))
@pytest.mark.parametrize("bits", BITS)
def test_tail_lead_and_alignment(torch, engines, bits, lane_form):
    """totals on either side of each block boundary (the tail inside, ending at, and straddling it) in the KDF's shape; lead_len 0, 4, 8
    with and without a head, bodies of length 0 and R - 1 at every address mod 8"""
    eng = engines[1] if lane_form else engines[0]
    R = sp.rate_of(bits)
    rng = np.random.default_rng(R)
    totals = [b * R + r for b in range(3) for r in range(R - 6, R + 2)]
    n = len(totals)
    head, keys = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)
    lens = [t - 36 for t in totals]
    offs, size = spread(lens)
    body = rng.integers(0, 256, size, dtype=np.uint8)              # the last message ends at the tensor's last byte
    lead = b"\x00\x00\x00\x01"
    run(torch, eng, bits, body, offs, lens, outlen=32, key=keys, custom=b"KDF", lead=lead, head=head)
    run(torch, eng, bits, body, offs, lens, outlen=32, key=keys[0], custom=b"KDF", lead=lead, head=head, xof=True)
    run(torch, eng, bits, body, offs[:8], lens[:8], outlen=8192, key=keys[:8], lead=lead, head=head[:8])           # the 5-byte tail
    run(torch, eng, bits, body, offs, lens, outlen=40, custom=b"S", lead=lead, head=head)
    lens = [l for l in (0, R - 1) for _ in range(8)]
    offs, size = spread(lens)
    body = rng.integers(0, 256, size, dtype=np.uint8)
    head, keys = rng.integers(0, 256, (16, 32), dtype=np.uint8), rng.integers(0, 256, (16, 32), dtype=np.uint8)
    for lead_len in (0, 4, 8):
        lead = bytes(range(0xF1, 0xF1 + lead_len))
        run(torch, eng, bits, body, offs, lens, outlen=32, key=keys, custom=b"c", lead=lead)
        run(torch, eng, bits, body, offs, lens, outlen=32, key=keys, custom=b"c", lead=lead, head=head)
        run(torch, eng, bits, body, offs, lens, outlen=32, custom=b"c", lead=lead, head=head)


@pytest.mark.parametrize("lane_form", (False, True))
@pytest.mark.parametrize("bits", BITS)
def test_keys_strings_and_output_lengths(torch, engines, bits, lane_form):
    eng = engines[1] if lane_form else engines[0]
    R = sp.rate_of(bits)
    rng = np.random.default_rng(R + 1)
    lens = [0, 5, R + 9]
    offs, size = spread(lens, first=5)
    body = rng.integers(0, 256, size, dtype=np.uint8)
    wide = rng.integers(0, 256, (3, 136), dtype=np.uint8)
    wt = dev(torch, wide)
    for kl in (8, 24, 32, 64, 128):                               # both header widths, the rows a strided view
        run(torch, eng, bits, body, offs, lens, outlen=32, key=wide[:, :kl], key_view=wt[:, :kl], custom=b"My Tagged Application")
    store = rng.integers(0, 256, 540, dtype=np.uint8)
    stt = dev(torch, store)
    for kl, at in ((0, 0), (1, 3), (32, 0), (132, 3), (164, 0), (200, 3)):      # shared keys; 200 bytes: two key blocks at R = 136
        run(torch, eng, bits, body, offs, lens, outlen=48, key=store[at:at + kl], key_view=stt[at:at + kl], custom=b"KDF", lead=b"\x00\x00\x00\x01")
    keys = wide[:, :32].copy()
    for S in (b"", b"s", bytes(range(40)), bytes(i & 0xFF for i in range(256))):       # one to three prefix blocks
        for N in (b"", bytes(range(100, 132))):
            run(torch, eng, bits, body, offs, lens, outlen=32, fname=N, custom=S)
    shake = hashlib.shake_128 if bits == 128 else hashlib.shake_256
    out = eng.cshake(bits, [b"", b"abc", bytes(R)], outlen=50, lead=b"ab").cpu().numpy()       # N = S = "": SHAKE
    for i, m in enumerate((b"", b"abc", bytes(R))):
        assert out[i].tobytes() == shake(b"ab" + m).digest(50), i
    for outlen in (1, 32, R, R + 1, 2 * R + 3):
        for xof in (False, True):
            run(torch, eng, bits, body, offs, lens, outlen=outlen, key=keys, custom=b"o", xof=xof)


@pytest.mark.parametrize("n", (1, 64, 130))
def test_mixed_lengths_in_both_forms(torch, engines, n):
    """1, 64 and 130 items with lengths mixed within a wavefront of the lane-sliced form"""
    rng = np.random.default_rng(1000 * n)
    lens = [int(x) for x in rng.integers(0, 2 * 136 + 41, n)]
    lens[0] = 0
    offs = [int(x) for x in np.cumsum([3] + lens[:-1])]
    body = rng.integers(0, 256, 3 + sum(lens), dtype=np.uint8)
    keys, head = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for eng in engines:
        run(torch, eng, 256, body, offs, lens, outlen=141, key=keys, custom=b"KDF", lead=b"\x00\x00\x00\x01", head=head)


def test_out_of_bounds_items(torch, engines):
    rng = np.random.default_rng(5)
    body = rng.integers(0, 256, 300, dtype=np.uint8)
    M64 = (1 << 64) - 1
    offs, lens, bad = [M64, 0, 301, 299, 300, 200, M64 - 5, 7], [1, 300, 0, 2, 0, 100, 6, 293], {0, 2, 3, 6}
    keys = rng.integers(0, 256, (len(offs), 32), dtype=np.uint8)
    for eng in engines:
        for key in (keys, keys[0], None):
            run(torch, eng, 256, body, offs, lens, outlen=200, key=key, custom=b"b", lead=b"\x07", bad=bad)


@pytest.mark.parametrize("bits", BITS)
def test_kdf_onestep_on_the_k_of_a_live_encaps(pkg, torch, engines, bits):
    """Encaps -> kdf_onestep on the device: K of encaps_random (seeded root) is the head, in place; default and explicit salt"""
    for eng in engines:
        eng.rng_seed(bytes(range(32)))
        n = 5
        ek, _ = eng.keygen_random(n)
        _, K = eng.encaps_random(ek)
        infos = [b"", b"session 1", bytes(range(100)), b"x" * 137, b"alg-id || party-u || party-v"]
        out = eng.kdf_onestep(K, infos, 64, bits=bits).cpu().numpy()
        salt = bytes(range(48))
        out2 = eng.kdf_onestep(K, infos, 32, bits=bits, salt=salt).cpu().numpy()
        Kh = K.cpu().numpy()
        for i in range(n):
            assert out[i].tobytes() == sp.kdf_onestep(bits, Kh[i].tobytes(), infos[i], 64), i
            assert out2[i].tobytes() == sp.kdf_onestep(bits, Kh[i].tobytes(), infos[i], 32, salt), i


def test_strided_k_view_is_used_in_place(pkg, torch, engines):
    """K rows that are a view with a row stride go to the library as they are -- the view's own address and stride, no copy -- as the
    key of MLKEM.kmac and as the head of MLKEM.kdf_onestep"""
    eng = engines[0]
    rng = np.random.default_rng(8)
    wide = rng.integers(0, 256, (6, 64), dtype=np.uint8)
    wt = dev(torch, wide)
    K = wt[:, 16:48]
    assert K.stride(0) == 64 and not K.is_contiguous()
    seen = []
    real = eng.lib.mlkem_kmac_dev

    def spy(*a):
        seen.append(a)
        return real(*a)
    eng.lib.mlkem_kmac_dev = spy
    try:
        msgs = [bytes([i]) * (3 * i) for i in range(6)]
        out = eng.kmac(256, K, msgs, outlen=32, custom=b"v").cpu().numpy()
        out2 = eng.kdf_onestep(K, msgs, 32).cpu().numpy()
    finally:
        eng.lib.mlkem_kmac_dev = real
    assert seen[0][3:6] == (K.data_ptr(), 32, 64)                      # key, key_len, key_stride
    assert seen[1][10:13] == (K.data_ptr(), 32, 64)                    # head, head_len, head_stride
    for i in range(6):
        assert out[i].tobytes() == sp.kmac(256, wide[i, 16:48].tobytes(), msgs[i], 32, b"v"), i
        assert out2[i].tobytes() == sp.kdf_onestep(256, wide[i, 16:48].tobytes(), msgs[i], 32), i
    assert (wt.cpu().numpy() == wide).all()


def test_host_pointer_calls(pkg, torch, engines):
    """mlkem_cshake and mlkem_kmac on numpy arrays: unaligned rows of 33 bytes whose last byte is left alone, an out-of-bounds item"""
    lib = pkg.load_library()
    rng = np.random.default_rng(9)
    lens = [int(x) for x in rng.integers(0, 300, 20)] + [0, 5]
    offs = [int(x) for x in np.cumsum([3] + lens[:-1])]
    body = rng.integers(0, 256, 3 + sum(lens), dtype=np.uint8)
    offs[-1] = body.size - 2                                          # out of bounds
    n = len(lens)
    head = rng.integers(0, 256, (n, 40), dtype=np.uint8)              # head_len 32 out of rows of 40
    keys = rng.integers(0, 256, (n, 33), dtype=np.uint8)[:, 1:]       # key rows at odd host addresses
    off, ln = np.array(offs, np.uint64), np.array(lens, np.uint32)
    lead, S = b"\x00\x00\x00\x01", b"host"
    for kind in ("kmac", "shared", "cshake"):
        out = np.full((n, 33), 0xA5, np.uint8)
        st = np.full(n, 7, np.int32)
        tail = (lead, 4, head.ctypes.data, 32, 40, body.ctypes.data, body.size, off.ctypes.data, ln.ctypes.data, out.ctypes.data, 32, 33,
                st.ctypes.data)
        if kind == "kmac":
            rc = lib.mlkem_kmac(1, n, keys.ctypes.data, 32, keys.strides[0], S, 4, *tail)
        elif kind == "shared":
            rc = lib.mlkem_kmac(2, n, keys.ctypes.data, 21, 0, S, 4, *tail)
        else:
            rc = lib.mlkem_cshake(128, n, b"fn", 2, S, 4, *tail)
        assert rc == 0, kind
        assert (out[:, 32] == 0xA5).all()
        for i in range(n - 1):
            X = lead + head[i, :32].tobytes() + body[offs[i]:offs[i] + lens[i]].tobytes()
            exp = {"kmac": lambda: sp.kmac(256, keys[i].tobytes(), X, 32, S), "shared": lambda: sp.kmac(128, keys[0, :21].tobytes(), X, 32, S, True),
                   "cshake": lambda: sp.cshake(128, X, 32, b"fn", S)}[kind]()
            assert out[i, :32].tobytes() == exp, (kind, i)
        assert not out[n - 1, :32].any() and list(st) == [0] * (n - 1) + [ERR_ARG]


def test_captured_graph_replays_on_changed_inputs(pkg, torch, engines):
    """mlkem_kmac_dev captured after a first eager call -- a per-item key call and a shared-key call: prefix kernel, item kernel and
    the zeroing of the midstate, one linear chain -- then replayed on changed keys and messages"""
    eng = engines[0]
    rng = np.random.default_rng(12)
    n = 40
    lens = [int(x) for x in rng.integers(0, 200, n)]
    offs = [int(x) for x in np.cumsum([1] + lens[:-1])]
    body = rng.integers(0, 256, 1 + sum(lens), dtype=np.uint8)
    keys = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    salt = rng.integers(0, 256, 45, dtype=np.uint8)
    bt, kt, st_ = dev(torch, body), dev(torch, keys), dev(torch, salt)
    ot, lt = dev(torch, np.array(offs, np.int64)), dev(torch, np.array(lens, np.int32))
    eng.kmac(256, kt, bt, ot, lt, outlen=32)                          # the first call is eager
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out1 = eng.kmac(256, kt, bt, ot, lt, outlen=32, custom=b"g", lead=b"\x01")
        out2 = eng.kmac(128, st_, bt, ot, lt, head=kt, outlen=40, custom=b"KDF", lead=b"\x00\x00\x00\x01", xof=True)
    body2 = rng.integers(0, 256, body.size, dtype=np.uint8)
    keys2 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    bt.copy_(dev(torch, body2))
    kt.copy_(dev(torch, keys2))
    out1.zero_(); out2.zero_()
    g.replay()
    torch.cuda.synchronize()
    o1, o2 = out1.cpu().numpy(), out2.cpu().numpy()
    for i, (o, l) in enumerate(zip(offs, lens)):
        m = body2[o:o + l].tobytes()
        assert o1[i].tobytes() == sp.kmac(256, keys2[i].tobytes(), b"\x01" + m, 32, b"g"), i
        assert o2[i].tobytes() == sp.kmac(128, salt.tobytes(), b"\x00\x00\x00\x01" + keys2[i].tobytes() + m, 40, b"KDF", True), i
    del g


def test_zero_items(pkg, torch, engines):
    lib = pkg.load_library()
    for eng in engines:
        empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
        off, ln = torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
        out, st = eng.kmac(256, torch.zeros((0, 32), dtype=torch.uint8, device="cuda"), empty, off, ln, outlen=32, return_status=True)
        assert out.shape == (0, 32) and st.shape == (0,)
        assert eng.cshake(128, [], outlen=16, custom=b"z").shape == (0, 16)
        assert eng.kdf_onestep(torch.zeros((0, 32), dtype=torch.uint8, device="cuda"), [], 32).shape == (0, 32)
        assert lib.mlkem_kmac_dev(eng._ctx, 1, 0, None, 32, 32, None, 0, None, 0, None, 0, 0, None, 0, None, None, None, 32, 32, None, None) == 0
        assert lib.mlkem_cshake_dev(eng._ctx, 256, 0, None, 0, None, 0, None, 0, None, 0, 0, None, 0, None, None, None, 32, 32, None, None) == 0
        assert lib.mlkem_kmac_dev(eng._ctx, 4, 0, None, 32, 32, None, 0, None, 0, None, 0, 0, None, 0, None, None, None, 32, 32, None, None) == ERR_ARG
    torch.cuda.synchronize()
