"""GPU tier (-m gpu): batched X25519 and the X-Wing hybrid KEM -- mlkem_x25519_dev, mlkem_xwing_{keygen,encaps,decaps}_dev and the two
random calls, through MLKEM.x25519 / xwing_*.

Two references.  The first 16 items of every shape go against the full independent restatement (tests/x25519_py.py: Python integers,
hashlib, tests/fips203_py.py).  ALL items go against a composition of the engine's own seeded FIPS-mode keygen / encaps / decaps, the
Python X25519 and hashlib.  Item i of every shape has the same inputs, so both references are computed once for the largest shape
and shared, read-only."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import x25519_py as X

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
CHUNK, SMALL_CHUNK = 8192, 640
NMAX, NFULL = 1300, 16
ERR_MODULUS, ERR_LOW_ORDER, ERR_ARG = -4, -7, -101
ROOT = hashlib.sha256(b"gpu-xwing-root").digest()
P = X.P


def rows(values, width=32):
    raw = b"".join(v.to_bytes(width, "little") if isinstance(v, int) else bytes(v) for v in values)
    return np.frombuffer(raw, np.uint8).reshape(len(values), width).copy()


def blocks(root, dom, pos, n, nbytes):
    pre = root + bytes([dom])
    return rows([hashlib.shake_256(pre + ((pos + i) & ((1 << 64) - 1)).to_bytes(8, "little")).digest(nbytes) for i in range(n)], nbytes)


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


_engines = {}


@pytest.fixture(scope="module")
def engine(pkg, torch):
    def get(pset, chunk_items=CHUNK, conformance="fips203"):
        key = (pset, chunk_items, conformance)
        if key not in _engines:
            _engines[key] = pkg.MLKEM(pset, device=0, chunk_items=chunk_items, conformance=conformance)
        return _engines[key]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


@pytest.fixture(scope="module")
def inputs():
    X.check_pinned()
    rng = np.random.default_rng(1120)
    sk, eseed = rng.integers(0, 256, (NMAX, 32), dtype=np.uint8), rng.integers(0, 256, (NMAX, 64), dtype=np.uint8)
    sk.setflags(write=False)
    eseed.setflags(write=False)
    return sk, eseed


@pytest.fixture(scope="module")
def restated(inputs):
    """the full restatement of the first NFULL items: pk, ct, ss"""
    sk, eseed = inputs
    pk = [X.xwing_keygen(bytes(s)) for s in sk[:NFULL]]
    enc = [X.xwing_encaps(p, bytes(e)) for p, e in zip(pk, eseed[:NFULL])]
    out = rows(pk, 1216), rows([c for c, _ in enc], 1120), rows([s for _, s in enc])
    for v in out:
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def composed(inputs, engine, torch):
    """all NMAX items from the engine's own seeded FIPS-mode ML-KEM-768 calls, the Python X25519 and hashlib: pk, ct, ss"""
    sk, eseed = inputs
    eng = engine(768, CHUNK, "fips203")
    e = rows([hashlib.shake_256(bytes(s)).digest(96) for s in sk], 96)
    d, z = torch.from_numpy(e[:, :32].copy()), torch.from_numpy(e[:, 32:64].copy())
    ek, dk = eng.keygen(d, z)
    c, K = eng.encaps(ek, torch.from_numpy(eseed[:, :32].copy()))
    Kd, _ = eng.decaps(dk, c, hash_check=False)
    assert torch.equal(K, Kd)
    ek, c, K = ek.cpu().numpy(), c.cpu().numpy(), K.cpu().numpy()
    pk_x = [X.x25519(bytes(r[64:]), X.BASE) for r in e]
    ct_x = [X.x25519(bytes(r[32:]), X.BASE) for r in eseed]
    ss_x = [X.x25519(bytes(r[32:]), p) for r, p in zip(eseed, pk_x)]
    ss = rows([X.combiner(bytes(k), s, c_, p) for k, s, c_, p in zip(K, ss_x, ct_x, pk_x)])
    out = np.concatenate([ek, rows(pk_x)], axis=1), np.concatenate([c, rows(ct_x)], axis=1), ss
    for v in out:
        v.setflags(write=False)
    return out


# ---- x25519 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 1000))
def test_x25519(engine, torch, n):
    """arbitrary u against the Python restatement; the base-point form equals u = 9"""
    eng = engine(768)
    rng = np.random.default_rng(n)
    k, u = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kt = torch.from_numpy(k).to(eng.device)
    out, st = eng.x25519(kt, torch.from_numpy(u).to(eng.device), return_status=True)
    assert [bytes(r) for r in out.cpu().numpy()] == [X.x25519(bytes(a), bytes(b)) for a, b in zip(k, u)]
    assert not st.any().item()
    nine = torch.from_numpy(rows([9] * n)).to(eng.device)
    base = eng.x25519(kt)
    assert torch.equal(base, eng.x25519(kt, nine))
    assert bytes(base[0].cpu().numpy()) == X.x25519(bytes(k[0]), X.BASE)


def test_x25519_edge_inputs(engine, torch):
    """scalars all-zero and all-0xFF; bit 255 of u ignored; u = 2^255 - 10 = 9 mod p; the low-order inputs 0, 1, p - 1, p, p + 1 give an
    all-zero row and status -7, their neighbours status 0"""
    eng = engine(768)
    scal = [bytes(32), bytes([0xFF] * 32), hashlib.sha256(b"edge").digest()]
    us = [9, 9 | (1 << 255), (1 << 255) - 10, (1 << 255) - 1, P - 2, 2] + list(X.LOW_ORDER_U) + [u | (1 << 255) for u in X.LOW_ORDER_U]
    k, u = rows([s for s in scal for _ in us]), rows([v for _ in scal for v in us])
    out, st = eng.x25519(torch.from_numpy(k).to(eng.device), torch.from_numpy(u).to(eng.device), return_status=True)
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert [bytes(r) for r in out] == [X.x25519(bytes(a), bytes(b)) for a, b in zip(k, u)]
    per = len(us)
    for s in range(len(scal)):
        o = out[s * per:(s + 1) * per]
        assert (o[0] == o[1]).all() and (o[0] == o[2]).all()
        assert not o[6:].any() and o[:6].any(axis=1).all()
        assert list(st[s * per:(s + 1) * per]) == [0] * 6 + [ERR_LOW_ORDER] * 10


# ---- X-Wing, seeded ---------------------------------------------------------------------------------------------------------------
# n either side of the wave size and of ML-KEM-768's small_max; 1300 items on 640-item chunks: three slices; 65 and 769 items (the
# one-workgroup-per-item and the batch kernels) on a context left in REFERENCE conformance (the X-Wing calls do not follow the
# context's mode) and 65 on an ML-KEM-512 engine (X-Wing fixes 768)
SHAPES = ((1, 768, CHUNK, "fips203"), (64, 768, CHUNK, "fips203"), (65, 768, CHUNK, "fips203"), (768, 768, CHUNK, "fips203"),
          (769, 768, CHUNK, "fips203"), (1300, 768, SMALL_CHUNK, "fips203"), (65, 768, CHUNK, "reference"), (769, 768, CHUNK, "reference"),
          (65, 512, CHUNK, "reference"))


@pytest.mark.parametrize("n,pset,chunk,conf", SHAPES)
def test_xwing_seeded(engine, torch, inputs, restated, composed, n, pset, chunk, conf):
    eng = engine(pset, chunk, conf)
    sk, eseed = (torch.from_numpy(v[:n].copy()).to(eng.device) for v in inputs)
    before = eng.scratch_bytes
    pk = eng.xwing_keygen(sk)
    ct, ss, st = eng.xwing_encaps(pk, eseed, return_status=True)
    ss_d = eng.xwing_decaps(sk, ct)
    ss_p = eng.xwing_decaps(sk, ct, pk=pk)
    pk_h, ct_h, ss_h = pk.cpu().numpy(), ct.cpu().numpy(), ss.cpu().numpy()
    f = min(n, NFULL)
    assert (pk_h[:f] == restated[0][:f]).all() and (ct_h[:f] == restated[1][:f]).all() and (ss_h[:f] == restated[2][:f]).all()
    assert (pk_h == composed[0][:n]).all()
    assert (ct_h == composed[1][:n]).all()
    assert (ss_h == composed[2][:n]).all()
    assert not st.any().item()
    assert torch.equal(ss_d, ss) and torch.equal(ss_p, ss)
    assert eng.scratch_bytes == before


def test_xwing_rejection_and_status(engine, torch, inputs, restated):
    """a flipped byte in ct_M gives the restatement's implicit-rejection secret, one in ct_X the restatement's secret, neither the
    sender's; a pk_M coefficient >= q gives status -4 on that item and 0 on its neighbours"""
    eng = engine(768)
    n = 5
    sk, eseed = (torch.from_numpy(v[:n].copy()).to(eng.device) for v in inputs)
    pk, ct, ss = (torch.from_numpy(v[:n].copy()).to(eng.device) for v in restated)
    bad = ct.clone()
    bad[1, 700] ^= 0x04
    bad[3, 1088 + 31] ^= 0x01
    got = eng.xwing_decaps(sk, bad).cpu().numpy()
    ss_h = ss.cpu().numpy()
    for i in (1, 3):
        assert bytes(got[i]) == X.xwing_decaps(bytes(inputs[0][i]), bytes(bad[i].cpu().numpy()))
        assert (got[i] != ss_h[i]).any()
    assert (got[[0, 2, 4]] == ss_h[[0, 2, 4]]).all()
    assert (eng.xwing_decaps(sk, bad, pk=pk).cpu().numpy() == got).all()
    pkb = pk.clone()
    pkb[2, 0], pkb[2, 1] = 0xFF, pkb[2, 1] | 0x0F      # coefficient 0 of item 2 = 0xFFF
    _, _, st = eng.xwing_encaps(pkb, eseed, return_status=True)
    assert st.cpu().tolist() == [0, 0, ERR_MODULUS, 0, 0]


# ---- random calls -------------------------------------------------------------------------------------------------------------------
def test_xwing_random_calls(engine, torch):
    """after rng_seed(fixed): sk = block(root, 3, pos)[:32], eseed = block(root, 4, pos)[:64]; the outputs equal the seeded calls on
    them; positions advance by n across mixed X-Wing and ML-KEM random calls (769 items: above small_max, 70: two waves)"""
    eng = engine(768, SMALL_CHUNK)
    eng.rng_seed(ROOT)
    pos = 0
    for n in (70, 769):
        sk, pk = eng.xwing_keygen_random(n)
        sk_w = blocks(ROOT, 3, pos, n, 32)
        assert (sk.cpu().numpy() == sk_w).all()
        assert torch.equal(pk, eng.xwing_keygen(torch.from_numpy(sk_w).to(eng.device)))
        pos += n
        _, _, seed = eng.keygen_random(3, return_seed=True)                    # an ML-KEM random call in between
        assert (seed.cpu().numpy() == blocks(ROOT, 1, pos, 3, 64)).all()
        pos += 3
        ct, ss, st = eng.xwing_encaps_random(pk, return_status=True)
        es = torch.from_numpy(blocks(ROOT, 4, pos, n, 64)).to(eng.device)
        ct_s, ss_s = eng.xwing_encaps(pk, es)
        assert torch.equal(ct, ct_s) and torch.equal(ss, ss_s) and not st.any().item()
        assert torch.equal(eng.xwing_decaps(sk, ct), ss)
        pos += n
    _, seed = eng.keygen_random(2, return_seed=True, dk=False)
    assert (seed.cpu().numpy() == blocks(ROOT, 1, pos, 2, 64)).all()


def test_xwing_random_calls_refuse_a_capturing_stream(engine, torch):
    """as the ML-KEM random calls: MLKEM_ERR_ARG on a capturing stream, nothing launched, no position consumed.  Never replayed."""
    eng = engine(768, SMALL_CHUNK)
    lib, ctx = eng.lib, eng._ctx
    eng.rng_seed(ROOT)
    n = 4
    sk0, pk0 = eng.xwing_keygen_random(n)      # positions 0..3; allocates the context's regions before the capture
    sk = torch.full((n, 32), 0x5A, dtype=torch.uint8, device=eng.device)
    pk = torch.full((n, 1216), 0x5A, dtype=torch.uint8, device=eng.device)
    ct = torch.full((n, 1120), 0x5A, dtype=torch.uint8, device=eng.device)
    ss = torch.full((n, 32), 0x5A, dtype=torch.uint8, device=eng.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=eng.device)
    g = torch.cuda.CUDAGraph()
    rcs = []
    with torch.cuda.graph(g, stream=side):
        st = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
        rcs.append(lib.mlkem_xwing_keygen_random_dev(ctx, n, sk.data_ptr(), pk.data_ptr(), st))
        rcs.append(lib.mlkem_xwing_encaps_random_dev(ctx, n, pk0.data_ptr(), ct.data_ptr(), ss.data_ptr(), None, st))
    assert rcs == [ERR_ARG] * 2
    torch.cuda.synchronize()
    for t in (sk, pk, ct, ss):
        assert (t == 0x5A).all().item()
    del g
    sk1, _ = eng.xwing_keygen_random(2)
    assert (sk1.cpu().numpy() == blocks(ROOT, 3, n, 2, 32)).all()


# ---- unchanged behaviour --------------------------------------------------------------------------------------------------------------
def test_mlkem_unchanged_after_xwing_calls(engine, torch, oracle, inputs):
    """scratch_bytes of a context is the same before and after X-Wing calls, and an ML-KEM encaps / decaps pair run after them still
    matches the oracle (reference mode, ML-KEM-768)"""
    eng = engine(768, CHUNK, "reference")
    before = eng.scratch_bytes
    n = 70
    sk, eseed = (torch.from_numpy(v[:n].copy()).to(eng.device) for v in inputs)
    pk = eng.xwing_keygen(sk)
    ct, ss = eng.xwing_encaps(pk, eseed)
    assert torch.equal(eng.xwing_decaps(sk, ct), ss)
    assert eng.scratch_bytes == before
    d, z, m = (np.ascontiguousarray(inputs[1][:n, a:a + 32]) for a in (0, 32, 16))
    oracle.set_conformance(False)
    ek_o, dk_o = oracle.keygen(768, d, z)
    c_o, K_o = oracle.encaps(768, ek_o, m)
    c, K = eng.encaps(torch.from_numpy(ek_o), torch.from_numpy(m))
    Kd, st = eng.decaps(torch.from_numpy(dk_o), c)
    assert (c.cpu().numpy() == c_o).all() and (K.cpu().numpy() == K_o).all()
    assert torch.equal(Kd, K) and not st.any().item()
