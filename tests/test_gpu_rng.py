"""GPU tier (-m gpu): device-side seed derivation -- mlkem_ctx_rng_seed, mlkem_keygen_random_dev, mlkem_encaps_random_dev,
mlkem_encaps_keyset_random_dev through the C-ABI and MLKEM.rng_seed / keygen_random / encaps_random / KeySet.encaps_random.

The derivation is restated with hashlib (block = SHAKE256(root || dom || LE64(pos)); KeyGen: d || z = block[:64], dom 1; Encaps:
m = block[:32], dom 2).  With a deterministic root every seed_out row must equal it, and every ek / dk / c / K / status must equal
the seeded call of the same engine on those seeds byte for byte (a subset also the oracle), in both conformance modes, at sizes
either side of small_max, wide_kem, the derivation-form switch and the chunk size, and at 2^16 items.  Also: split invariance and
position accounting across call types, OS-seeded behaviour, and the refusal of a capturing stream."""
import ctypes as C
import hashlib

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
SMALL_MAX = {512: 1536, 768: 768, 1024: 512}      # Workspace::small_max_k (mlkem_pipeline.hpp)
WIDE_KEM = {512: 4096, 768: 3072, 1024: 4096}     # Workspace::wide_max_k
RNG_WIDE = 4096                                   # RNG_WIDE_ITEMS (mlkem_rng.hpp): one sponge per wavefront up to here
CHUNK, SMALL_CHUNK = 8192, 640                    # chunk_items of the two kinds of engine the tests use
ERR_PARAM_SET, ERR_MODULUS, ERR_ARG = -1, -4, -101
DOM_KEYGEN, DOM_ENCAPS = 1, 2
ROOT_A = hashlib.sha256(b"gpu-rng-root-a").digest()
ROOT_B = bytes(range(32))


def blocks(root, dom, pos, n, nbytes):
    sh = hashlib.shake_256
    pre = root + bytes([dom])
    return np.frombuffer(b"".join(sh(pre + ((pos + i) & ((1 << 64) - 1)).to_bytes(8, "little")).digest(nbytes) for i in range(n)),
                         np.uint8).reshape(n, nbytes).copy()


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
    def get(pset, chunk_items=CHUNK, conformance="reference", tag=0):
        key = (pset, chunk_items, conformance, tag)
        if key not in _engines:
            _engines[key] = pkg.MLKEM(pset, device=0, chunk_items=chunk_items, conformance=conformance)
        return _engines[key]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


def sizes_for(pset):
    """(n, chunk_items): 1, 64, either side of small_max, wide_kem and the derivation switch on an engine whose chunk holds them; either
    side of the chunk size and 2 chunks + a short one on an engine of 640-item chunks; 2^16 over 8192-item chunks"""
    s = {1, 64, SMALL_MAX[pset], SMALL_MAX[pset] + 1, WIDE_KEM[pset], WIDE_KEM[pset] + 1, RNG_WIDE, RNG_WIDE + 1}
    out = [(n, CHUNK) for n in sorted(s)]
    out += [(SMALL_CHUNK, SMALL_CHUNK), (SMALL_CHUNK + 1, SMALL_CHUNK), (2 * SMALL_CHUNK + 37, SMALL_CHUNK), (1 << 16, CHUNK)]
    return out


def _subset(n):
    """at most 1024 items for the oracle: the first 512 and the last 512"""
    return np.arange(n) if n <= 1024 else np.concatenate([np.arange(512), np.arange(n - 512, n)])


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("fips", (0, 1))
def test_keygen_random_deterministic(engine, torch, oracle, pset, fips):
    conf = "fips203" if fips else "reference"
    try:
        oracle.set_conformance(bool(fips))
        for n, chunk in sizes_for(pset):
            eng = engine(pset, chunk, conf)
            eng.rng_seed(ROOT_A)
            ek, dk, seed = eng.keygen_random(n, return_seed=True)
            want = blocks(ROOT_A, DOM_KEYGEN, 0, n, 64)
            seed_h = seed.cpu().numpy()
            assert (seed_h == want).all(), (n, chunk)
            d, z = torch.from_numpy(want[:, :32].copy()), torch.from_numpy(want[:, 32:].copy())
            ek_s, dk_s = eng.keygen(d, z)
            assert torch.equal(ek, ek_s) and torch.equal(dk, dk_s), (n, chunk)
            sub = _subset(n)
            ek_o, dk_o = oracle.keygen(pset, np.ascontiguousarray(want[sub, :32]), np.ascontiguousarray(want[sub, 32:]))
            assert (ek.cpu().numpy()[sub] == ek_o).all() and (dk.cpu().numpy()[sub] == dk_o).all(), (n, chunk)
            # the same positions again without dk: the same ek and seeds; the seeds decapsulate
            eng.rng_seed(ROOT_A)
            ek2, seed2 = eng.keygen_random(n, return_seed=True, dk=False)
            assert torch.equal(ek2, ek) and torch.equal(seed2, seed), (n, chunk)
            # ... and once more without seed_out
            eng.rng_seed(ROOT_A)
            ek3, dk3 = eng.keygen_random(n)
            assert torch.equal(ek3, ek) and torch.equal(dk3, dk), (n, chunk)
            m = torch.from_numpy(blocks(ROOT_B, DOM_ENCAPS, 5, n, 32))
            c, K = eng.encaps(ek2, m)
            assert torch.equal(eng.decaps_seed(seed2, c), K), (n, chunk)
    finally:
        oracle.set_conformance(False)


def _bad_ek(ek, item):
    """coefficient 0 of `item` becomes 0xFFF >= q"""
    ek[item, 0] = 0xFF
    ek[item, 1] |= 0x0F


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("fips", (0, 1))
def test_encaps_random_equals_seeded_encaps(engine, torch, pset, fips):
    """c, K and status byte for byte those of encaps(ek, m_hashlib); a bad-coefficient ek reports MLKEM_ERR_MODULUS in FIPS mode"""
    conf = "fips203" if fips else "reference"
    base = engine(pset, CHUNK, conf)
    nk = 1 << 16
    base.rng_seed(ROOT_B)
    ek_all = base.keygen_random(nk)[0]
    for n, chunk in sizes_for(pset):
        eng = engine(pset, chunk, conf)
        ek = ek_all[:n].clone()
        bad = sorted({0, n // 2, n - 1}) if n > 1 else [0]
        for i in bad[::2]:
            _bad_ek(ek, i)
        eng.rng_seed(ROOT_A)
        # some positions consumed first, so that the call does not start at 0
        eng.keygen_random(3)
        c, K, st = eng.encaps_random(ek, return_status=True)
        m = torch.from_numpy(blocks(ROOT_A, DOM_ENCAPS, 3, n, 32))
        c_s, K_s, st_s = eng.encaps(ek, m, return_status=True)
        assert torch.equal(c, c_s) and torch.equal(K, K_s) and torch.equal(st, st_s), (n, chunk)
        st_h = st.cpu().numpy()
        want = np.zeros(n, np.int32)
        if fips:
            want[bad[::2]] = ERR_MODULUS
        assert (st_h == want).all(), (n, chunk)
        # without status
        eng.rng_seed(ROOT_A)
        eng.keygen_random(3)
        c2, K2 = eng.encaps_random(ek)
        assert torch.equal(c2, c) and torch.equal(K2, K), (n, chunk)


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("fips", (0, 1))
def test_keyset_encaps_random_equals_keyset_encaps(engine, torch, pset, fips):
    """KeySet.encaps_random == KeySet.encaps on the hashlib m with the same indices; an out-of-range index zeroes the item, reports
    ERR_ARG and still consumes its position"""
    conf = "fips203" if fips else "reference"
    n_keys = 64
    base = engine(pset, CHUNK, conf)
    base.rng_seed(ROOT_B)
    _, seed = base.keygen_random(n_keys, return_seed=True, dk=False)
    ks = base.prepare_keys(seed=seed)
    try:
        for n, chunk in ((1, CHUNK), (64, CHUNK), (SMALL_MAX[pset] + 300, CHUNK), (RNG_WIDE + 1, CHUNK), (5000, CHUNK),
                         (2 * SMALL_CHUNK + 37, SMALL_CHUNK), (1 << 16, CHUNK)):
            eng = engine(pset, chunk, conf)
            rng = np.random.default_rng(n + pset)
            idx = rng.integers(0, n_keys, n).astype(np.uint32)
            badpos = np.unique(rng.integers(0, n, 3)) if n > 1 else np.array([], np.int64)
            idx[badpos] = n_keys + 5
            idx_t = torch.from_numpy(idx.view(np.int32)).cuda()
            eng.rng_seed(ROOT_A)
            c, K, st = ks.encaps_random(key_index=idx_t, return_status=True, engine=eng)
            m = torch.from_numpy(blocks(ROOT_A, DOM_ENCAPS, 0, n, 32))
            c_s, K_s, st_s = ks.encaps(m, key_index=idx_t, return_status=True, engine=eng)
            assert torch.equal(c, c_s) and torch.equal(K, K_s) and torch.equal(st, st_s), (n, chunk)
            st_h = st.cpu().numpy()
            isbad = np.zeros(n, bool)
            isbad[badpos] = True
            assert (st_h == np.where(isbad, ERR_ARG, 0)).all()
            assert not c.cpu().numpy()[isbad].any() and not K.cpu().numpy()[isbad].any()
            # the next call continues at position n: every item consumed one, the refused ones included
            c1, K1 = ks.encaps_random(n=2, engine=eng)
            c1_s, K1_s = ks.encaps(torch.from_numpy(blocks(ROOT_A, DOM_ENCAPS, n, 2, 32)), engine=eng)
            assert torch.equal(c1, c1_s) and torch.equal(K1, K1_s), (n, chunk)
    finally:
        ks.close()


@pytest.mark.parametrize("pset", (512, 768, 1024))
def test_split_invariance_across_the_small_batch_switch(engine, torch, pset):
    """a small call (one workgroup per item, wave-wide derivation) followed by a large one (batch path, lane-sliced derivation,
    several slices) equals one large call; likewise 5 + 3 against 8"""
    eng = engine(pset, SMALL_CHUNK)
    for n1, n2 in ((5, 3), (7, max(SMALL_MAX[pset], RNG_WIDE) + 500)):
        eng.rng_seed(ROOT_A)
        ek, dk, seed = eng.keygen_random(n1 + n2, return_seed=True)
        c, K = eng.encaps_random(ek)
        eng.rng_seed(ROOT_A)
        ek1, dk1, seed1 = eng.keygen_random(n1, return_seed=True)
        ek2, dk2, seed2 = eng.keygen_random(n2, return_seed=True)
        c1, K1 = eng.encaps_random(ek1)
        c2, K2 = eng.encaps_random(ek2)
        for whole, a, b in ((ek, ek1, ek2), (dk, dk1, dk2), (seed, seed1, seed2), (c, c1, c2), (K, K1, K2)):
            assert torch.equal(whole, torch.cat([a, b])), (n1, n2)


def test_position_accounting_across_call_types(engine, torch, pkg):
    """KeyGen 3, Encaps 5, key-set Encaps 2, an empty call, KeyGen 4: positions 0-2, 3-7, 8-9, none, 10-13"""
    eng = engine(768, CHUNK)
    eng.rng_seed(ROOT_B)
    ek_a, _, seed_a = eng.keygen_random(3, return_seed=True)
    assert (seed_a.cpu().numpy() == blocks(ROOT_B, DOM_KEYGEN, 0, 3, 64)).all()
    ek5 = torch.cat([ek_a, ek_a[:2]])
    c, K = eng.encaps_random(ek5)
    c_s, K_s = eng.encaps(ek5, torch.from_numpy(blocks(ROOT_B, DOM_ENCAPS, 3, 5, 32)))
    assert torch.equal(c, c_s) and torch.equal(K, K_s)
    with eng.prepare_keys(seed=seed_a) as ks:
        idx = torch.tensor([2, 1], dtype=torch.int32).cuda()
        c2, K2 = ks.encaps_random(key_index=idx)
        c2_s, K2_s = ks.encaps(torch.from_numpy(blocks(ROOT_B, DOM_ENCAPS, 8, 2, 32)), key_index=idx)
        assert torch.equal(c2, c2_s) and torch.equal(K2, K2_s)
        assert ks.encaps_random(n=0)[0].shape[0] == 0
    assert eng.keygen_random(0)[0].shape[0] == 0
    assert eng.encaps_random(ek_a[:0])[0].shape[0] == 0
    _, seed_b = eng.keygen_random(4, return_seed=True, dk=False)
    assert (seed_b.cpu().numpy() == blocks(ROOT_B, DOM_KEYGEN, 10, 4, 64)).all()


def test_os_seeded_generator(engine, torch, pkg):
    """never seeded: the first random call seeds from the OS.  Two contexts disagree, all 2^16 ek of one call are distinct, rng_seed()
    changes the stream, and KeyGen -> Encaps -> Decaps round-trips"""
    a, b = pkg.MLKEM(768, device=0, chunk_items=CHUNK), pkg.MLKEM(768, device=0, chunk_items=CHUNK)
    try:
        n = 1 << 16
        ek, dk, seed = a.keygen_random(n, return_seed=True)
        ek_b, _, seed_b = b.keygen_random(64, return_seed=True)
        assert not torch.equal(seed[:64], seed_b) and not torch.equal(ek[:64], ek_b)
        rows = ek.cpu().numpy()
        assert len({hashlib.sha256(r.tobytes()).digest() for r in rows}) == n
        assert len({r.tobytes() for r in seed.cpu().numpy()}) == n
        c, K, st = a.encaps_random(ek, return_status=True)
        K2, st2 = a.decaps(dk, c)
        assert torch.equal(K, K2) and not st.any().item() and not st2.any().item()
        assert torch.equal(a.decaps_seed(seed, c), K)
        assert len({r.tobytes() for r in K.cpu().numpy()}) == n
        a.rng_seed()
        _, seed2 = a.keygen_random(64, return_seed=True, dk=False)
        assert not torch.equal(seed2, seed[:64])
        # explicit reseeds with one root agree, across contexts too
        a.rng_seed(ROOT_A)
        b.rng_seed(torch.from_numpy(np.frombuffer(ROOT_A, np.uint8).copy()))
        assert torch.equal(a.keygen_random(9, return_seed=True)[2], b.keygen_random(9, return_seed=True)[2])
    finally:
        a.close()
        b.close()


def test_argument_errors_with_a_context(engine, torch, pkg):
    eng = engine(768, CHUNK)
    lib, ctx, st = eng.lib, eng._ctx, eng._stream()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=eng.device)
    p = buf.data_ptr()
    assert lib.mlkem_keygen_random_dev(ctx, 999, 1, p, p, p, st) == ERR_PARAM_SET
    assert lib.mlkem_keygen_random_dev(ctx, 768, 1, p, None, None, st) == ERR_ARG
    assert lib.mlkem_keygen_random_dev(ctx, 768, 1, None, p, p, st) == ERR_ARG
    assert lib.mlkem_keygen_random_dev(ctx, 768, 1, p + 8, p, p, st) == ERR_ARG
    assert lib.mlkem_encaps_random_dev(ctx, 768, 1, p, p, None, None, st) == ERR_ARG
    assert lib.mlkem_encaps_random_dev(ctx, 768, 1, p, p, p, p + 2, st) == ERR_ARG
    assert lib.mlkem_encaps_keyset_random_dev(ctx, None, 1, None, p, p, None, st) == ERR_ARG
    assert lib.mlkem_ctx_rng_seed(None, None) == ERR_ARG
    # n == 0 is a no-op that leaves the position unchanged
    eng.rng_seed(ROOT_A)
    assert lib.mlkem_keygen_random_dev(ctx, 768, 0, None, None, None, st) == 0
    assert lib.mlkem_encaps_random_dev(ctx, 768, 0, None, None, None, None, st) == 0
    _, seed = eng.keygen_random(2, return_seed=True, dk=False)
    assert (seed.cpu().numpy() == blocks(ROOT_A, DOM_KEYGEN, 0, 2, 64)).all()


def test_random_calls_refuse_a_capturing_stream(engine, torch, pkg):
    """A captured call would replay its positions, and so its keys: on a capturing stream every random call returns MLKEM_ERR_ARG,
    launches nothing and consumes no position.  The graph is never replayed."""
    eng = engine(768, CHUNK)
    lib, ctx = eng.lib, eng._ctx
    eng.rng_seed(ROOT_A)
    n = 4
    ek0, _, seed0 = eng.keygen_random(n, return_seed=True)      # positions 0..3; allocates the context's regions before the capture
    with eng.prepare_keys(seed=seed0) as ks:
        ek = torch.full((n, eng.ek_len), 0x5A, dtype=torch.uint8, device=eng.device)
        dk = torch.full((n, eng.dk_len), 0x5A, dtype=torch.uint8, device=eng.device)
        seed = torch.full((n, 64), 0x5A, dtype=torch.uint8, device=eng.device)
        c = torch.full((n, eng.c_len), 0x5A, dtype=torch.uint8, device=eng.device)
        K = torch.full((n, 32), 0x5A, dtype=torch.uint8, device=eng.device)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=eng.device)
        g = torch.cuda.CUDAGraph()
        rcs = []
        with torch.cuda.graph(g, stream=side):
            st = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
            rcs.append(lib.mlkem_keygen_random_dev(ctx, 768, n, ek.data_ptr(), dk.data_ptr(), seed.data_ptr(), st))
            rcs.append(lib.mlkem_encaps_random_dev(ctx, 768, n, ek0.data_ptr(), c.data_ptr(), K.data_ptr(), None, st))
            rcs.append(lib.mlkem_encaps_keyset_random_dev(ctx, ks._h, n, None, c.data_ptr(), K.data_ptr(), None, st))
        assert rcs == [ERR_ARG] * 3
        torch.cuda.synchronize()
        for t in (ek, dk, seed, c, K):
            assert (t == 0x5A).all().item()
        del g
    # no position was consumed: the next call continues at 4
    _, seed1 = eng.keygen_random(2, return_seed=True, dk=False)
    assert (seed1.cpu().numpy() == blocks(ROOT_A, DOM_KEYGEN, n, 2, 64)).all()
