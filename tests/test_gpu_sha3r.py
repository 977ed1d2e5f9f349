"""GPU tier (-m gpu): SHA-3 / SHAKE over device-resident messages of unequal length -- mlkem_sha3_ragged_dev / mlkem_sha3_ragged
through MLKEM.sha3 and a few raw ctypes calls.  The expected value is always hashlib.  Both kernel forms are reached: by size on the
default engine (n either side of the limit the engine reports) and, for the length x alignment matrix of the CPU tier, on a second
engine created with MLKEM_SHA3_WIDE_ITEMS=0 (always one sponge per lane).  No test passes an offset that lies inside body_bytes but
outside the real allocation."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
ERR_ARG = -101
HASHLIB = {"sha3_224": hashlib.sha3_224, "sha3_256": hashlib.sha3_256, "sha3_384": hashlib.sha3_384, "sha3_512": hashlib.sha3_512,
           "shake128": hashlib.shake_128, "shake256": hashlib.shake_256}
ALG_NAMES = sorted(HASHLIB)


def want(pkg, alg, msg, outlen):
    h = HASHLIB[alg](msg)
    return h.digest() if pkg.SHA3_ALGS[alg][2] else h.digest(outlen)


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
    assert default.sha3_wide_max > 0 and lanes.sha3_wide_max == 0
    yield default, lanes
    default.close()
    lanes.close()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(pkg, torch, eng, alg, body, offs, lens, head=None, outlen=None, bad=()):
    """MLKEM.sha3 on an in-place body tensor; every row against hashlib (zero row and status -101 for the items in `bad`)"""
    outlen = outlen or pkg.SHA3_ALGS[alg][2]
    bt = dev(torch, body)
    ht = None if head is None else dev(torch, head)
    out, st = eng.sha3(alg, bt, dev(torch, np.array(offs, np.uint64).view(np.int64)), dev(torch, np.array(lens, np.uint32).view(np.int32)),
                       head=ht, outlen=outlen, return_status=True)
    torch.cuda.synchronize()
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert out.shape == (len(offs), outlen)
    for i, (o, l) in enumerate(zip(offs, lens)):
        if i in bad:
            assert not out[i].any() and st[i] == ERR_ARG, i
        else:
            msg = (head[i].tobytes() if head is not None else b"") + body[o:o + l].tobytes()
            assert out[i].tobytes() == want(pkg, alg, msg, outlen), (alg, i, o, l)
            assert st[i] == 0


def packed(rng, lens, lead=3):
    """random bytes, the messages back to back after `lead` bytes: every start alignment occurs"""
    offs = [int(x) for x in np.cumsum([lead] + list(lens[:-1]))] if len(lens) else []
    body = rng.integers(0, 256, lead + int(sum(lens)) + 1, dtype=np.uint8)
    return body, offs


@pytest.mark.parametrize("lane_form", (False, True))
@pytest.mark.parametrize("alg", ALG_NAMES)
def test_length_by_alignment_matrix(pkg, torch, engines, alg, lane_form):
    """the CPU tier's matrix: 13 lengths around the rate x 16 start alignments, heads, SHAKE output lengths -- on each form"""
    eng = engines[1] if lane_form else engines[0]
    R, digest = pkg.SHA3_ALGS[alg][1:]
    rng = np.random.default_rng(R)
    offs, lens, pos = [], [], 0
    for L in (0, 1, 7, 8, 9, R - 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 3 * R + 5):
        for a in range(16):
            pos += (a - pos) % 16
            offs.append(pos)
            lens.append(L)
            pos += L
    body = rng.integers(0, 256, pos, dtype=np.uint8)          # the last message ends at the tensor's last byte
    run(pkg, torch, eng, alg, body, offs, lens, outlen=digest or 32)
    blens = [0, 5, R - 1, R + 1] * 17                          # 68 items: two wavefronts of the lane-sliced form
    body, boffs = packed(rng, blens, lead=1)
    for hl in (32, 64, R - 8, R, R + 8):
        wide = rng.integers(0, 256, (len(blens), hl + 24), dtype=np.uint8)
        ht = dev(torch, wide)[:, :hl]                          # a view with a row stride
        out = eng.sha3(alg, dev(torch, body), dev(torch, np.array(boffs, np.int64)), dev(torch, np.array(blens, np.int32)), head=ht,
                       outlen=digest or 48).cpu().numpy()
        for i, (o, l) in enumerate(zip(boffs, blens)):
            assert out[i].tobytes() == want(pkg, alg, wide[i, :hl].tobytes() + body[o:o + l].tobytes(), digest or 48), (alg, hl, i)
    if not digest:
        for outlen in (1, 3, 32, R - 1, R, R + 1, 2 * R + 5):
            run(pkg, torch, eng, alg, body, boffs[:5], blens[:5], outlen=outlen)


@pytest.mark.parametrize("alg", ("sha3_256", "shake128"))
def test_both_forms_by_size(pkg, torch, engines, alg):
    """n = the engine's limit (one sponge per wavefront) and limit + 1 (one per lane): random lengths in [0, 3R] at random byte offsets"""
    eng = engines[0]
    R = pkg.SHA3_ALGS[alg][1]
    limit = eng.sha3_wide_max
    for n in (limit, limit + 1):
        rng = np.random.default_rng(n)
        lens = [int(x) for x in rng.integers(0, 3 * R + 1, n)]
        body, offs = packed(rng, lens)
        run(pkg, torch, eng, alg, body, offs, lens, outlen=pkg.SHA3_ALGS[alg][2] or 64)


def test_sixty_five_thousand_messages(pkg, torch, engines):
    n = 1 << 16
    rng = np.random.default_rng(16)
    lens = [int(x) for x in rng.integers(0, 401, n)]
    body, offs = packed(rng, lens)
    run(pkg, torch, engines[0], "shake256", body, offs, lens, outlen=32)


def test_agrees_with_h_g_j(pkg, torch, engines):
    """equal-length 8-byte aligned rows: sha3_256 = H, sha3_512 = G, shake128 with 32 bytes = J (the reference mode's J)"""
    eng = engines[0]
    n, ln = 3000, 1184
    rng = np.random.default_rng(1)
    msgs = dev(torch, rng.integers(0, 256, (n, ln), dtype=np.uint8))
    offs = torch.arange(n, device=msgs.device, dtype=torch.int64) * ln
    lens = torch.full((n,), ln, device=msgs.device, dtype=torch.int32)
    flat = msgs.reshape(-1)
    assert torch.equal(eng.sha3("sha3_256", flat, offs, lens), eng.H(msgs))
    assert torch.equal(eng.sha3("sha3_512", flat, offs, lens), eng.G(msgs))
    assert torch.equal(eng.sha3("shake128", flat, offs, lens, outlen=32), eng.J(msgs))


@pytest.mark.parametrize("n", (5, 2500))
def test_head_is_the_k_of_a_live_encaps(pkg, torch, engines, n):
    """K of encaps_random used in place as the head (row stride 32, no copy), the contexts a list of bytes: SHAKE256(K[i] || ctx[i])"""
    eng = engines[0]
    eng.rng_seed(bytes(range(32)))
    ek, _ = eng.keygen_random(n)
    _, K = eng.encaps_random(ek)
    rng = np.random.default_rng(n)
    ctxs = [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in rng.integers(0, 200, n)]
    out = eng.sha3("shake256", ctxs, head=K, outlen=64).cpu().numpy()
    Kh = K.cpu().numpy()
    for i in range(n):
        assert out[i].tobytes() == hashlib.shake_256(Kh[i].tobytes() + ctxs[i]).digest(64), i


def test_in_place_body_with_user_offsets(pkg, torch, engines):
    """descending, overlapping and repeated offsets into one tensor, a body that ends at the tensor's last byte, empty bodies"""
    rng = np.random.default_rng(3)
    body = rng.integers(0, 256, 700, dtype=np.uint8)
    offs = [600, 450, 450, 300, 301, 302, 0, 0, 699, 700, 137]
    lens = [100, 200, 200, 250, 250, 9, 700, 0, 1, 0, 136]
    for eng in engines:
        for alg in ("sha3_224", "sha3_384", "shake256"):
            run(pkg, torch, eng, alg, body, offs, lens, outlen=pkg.SHA3_ALGS[alg][2] or 100)


def test_out_of_bounds_items(pkg, torch, engines):
    rng = np.random.default_rng(5)
    body = rng.integers(0, 256, 300, dtype=np.uint8)
    M64 = (1 << 64) - 1
    offs, lens, bad = [M64, 0, 301, 299, 300, 200, M64 - 5, 7], [1, 300, 0, 2, 0, 100, 6, 293], {0, 2, 3, 6}
    for eng in engines:
        for alg in ("sha3_256", "shake128"):
            run(pkg, torch, eng, alg, body, offs, lens, outlen=pkg.SHA3_ALGS[alg][2] or 200, bad=bad)


def test_argument_errors_leave_out_untouched(pkg, torch, engines):
    eng = engines[0]
    lib = pkg.load_library()
    body = torch.zeros(64, dtype=torch.uint8, device="cuda")
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    ln = torch.full((2,), 8, dtype=torch.int32, device="cuda")
    out = torch.full((2, 64), 0xA5, dtype=torch.uint8, device="cuda")
    head = torch.zeros((2, 64), dtype=torch.uint8, device="cuda")
    base = dict(alg=1, n=2, head=None, head_len=0, head_stride=0, body=body.data_ptr(), body_bytes=64, off=off.data_ptr(), ln=ln.data_ptr(),
                out=out.data_ptr(), outlen=32, out_stride=64, status=None)

    def call(**kw):
        a = dict(base, **kw)
        return lib.mlkem_sha3_ragged_dev(eng._ctx, a["alg"], a["n"], a["head"], a["head_len"], a["head_stride"], a["body"], a["body_bytes"],
                                         a["off"], a["ln"], a["out"], a["outlen"], a["out_stride"], a["status"], None)
    for kw in (dict(alg=6), dict(alg=-1), dict(outlen=31), dict(alg=4, outlen=0), dict(alg=5, outlen=65537, out_stride=65540), dict(out=None),
               dict(off=None), dict(ln=None), dict(body=None), dict(out=out.data_ptr() + 8), dict(out_stride=34), dict(out_stride=28),
               dict(head=head.data_ptr(), head_len=12, head_stride=16), dict(head=head.data_ptr() + 4, head_len=8, head_stride=8),
               dict(head=head.data_ptr(), head_len=16, head_stride=8)):
        assert call(**kw) == ERR_ARG, kw
    assert call(n=0, out=None, off=None, ln=None) == 0
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    assert call() == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[0, :32].tobytes() == hashlib.sha3_256(bytes(8)).digest() and (o[:, 32:] == 0xA5).all()


def test_host_pointer_call(pkg, torch, engines):
    """mlkem_sha3_ragged on numpy arrays: the same bytes, unaligned rows of 33 bytes whose last byte is left alone"""
    lib = pkg.load_library()
    rng = np.random.default_rng(9)
    lens = [int(x) for x in rng.integers(0, 300, 100)] + [0, 5]
    body, offs = packed(rng, lens)
    offs[-1], lens[-1] = body.size - 2, 5                     # out of bounds
    n = len(lens)
    head = rng.integers(0, 256, (n, 40), dtype=np.uint8)      # head_len 32 out of rows of 40
    off, ln = np.array(offs, np.uint64), np.array(lens, np.uint32)
    for alg, outlen in (("sha3_256", 32), ("shake128", 32)):
        out = np.full((n, 33), 0xA5, np.uint8)
        st = np.full(n, 7, np.int32)
        rc = lib.mlkem_sha3_ragged(pkg.SHA3_ALGS[alg][0], n, head.ctypes.data, 32, 40, body.ctypes.data, body.size, off.ctypes.data,
                                   ln.ctypes.data, out.ctypes.data, outlen, 33, st.ctypes.data)
        assert rc == 0
        assert (out[:, 32] == 0xA5).all()
        for i in range(n - 1):
            assert out[i, :32].tobytes() == want(pkg, alg, head[i, :32].tobytes() + body[offs[i]:offs[i] + lens[i]].tobytes(), outlen), i
        assert not out[n - 1, :32].any() and list(st) == [0] * (n - 1) + [ERR_ARG]
