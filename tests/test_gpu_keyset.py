"""GPU tier (-m gpu): prepared key sets -- mlkem_keyset_create / _destroy / _info, mlkem_encaps_keyset_dev / mlkem_decaps_keyset_dev
through the C-ABI and MLKEM.prepare_keys / KeySet.

Every c / K of a key-set call is compared byte for byte with mlkem_encaps_dev / mlkem_decaps_dev (Decaps_internal) on the keys
gathered by the same indices, in both conformance modes, for sets made from ek, dk and seed; a subset is cross-checked against the
oracle.  Sizes straddle the key-set small limit (one workgroup per item below, the indexed batch path above) and wide_kem; 2^16
items on a context of 4096-item chunks run the chunk loops many times.  Also: implicit rejection, out-of-range indices mixed with
valid ones, refusal with the bits of mlkem_check_keys_dev, Decaps on an ek-only set, one set used from two contexts and a side
stream, destroy and re-create."""
import ctypes as C

import numpy as np
import pytest

from keycheck_cases import corrupt, CLASSES

pytestmark = pytest.mark.gpu
# KeysetLimits (mlkem_keyset.hpp): one workgroup per item up to *_MAX items, eight waves per item up to *_LAT
KS_ENC_MAX, KS_DEC_MAX = {512: 1536, 768: 1024, 1024: 768}, {512: 3072, 768: 2048, 1024: 3072}
KS_ENC_LAT, KS_DEC_LAT = {512: 256, 768: 512, 1024: 256}, {512: 384, 768: 256, 1024: 256}
WIDE_KEM = {512: 4096, 768: 3072, 1024: 4096}     # Workspace::wide_max_k (mlkem_pipeline.hpp)
ERR_KEY, ERR_ARG = -6, -101


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
    def get(pset, chunk_items=0, conformance="reference", tag=0):
        key = (pset, chunk_items, conformance, tag)
        if key not in _engines:
            _engines[key] = pkg.MLKEM(pset, device=0, chunk_items=chunk_items, conformance=conformance)
        return _engines[key]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


def _keys(eng, torch, n_keys, salt):
    rng = np.random.default_rng(7919 * eng.param_set + 31 * n_keys + salt)
    d, z = (rng.integers(0, 256, (n_keys, 32), dtype=np.uint8) for _ in range(2))
    ek, dk = eng.keygen(torch.from_numpy(d), torch.from_numpy(z))
    seed = torch.from_numpy(np.ascontiguousarray(np.concatenate([d, z], axis=1))).to(eng.device)
    return ek, dk, seed


def _indices(torch, n, n_keys, seed, n_bad=0):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_keys, n).astype(np.uint32)
    bad = np.zeros(n, bool)
    if n_bad:
        pos = rng.choice(n, min(n_bad, n), replace=False)
        idx[pos] = n_keys + rng.integers(0, 1 << 20, pos.size).astype(np.uint32)
        idx[pos[:1]] = 0xFFFFFFFF
        bad[pos] = True
    return torch.from_numpy(idx.view(np.int32)).cuda(), idx, bad


def _check_round(eng, torch, ks, ek, dk, n, idx_t, idx, bad, salt, decaps=True, consistent=True):
    """encaps (and decaps) through the set == the per-item calls on the gathered keys; out-of-range items zero + ERR_ARG;
    consistent: ek and dk are pairs, so untouched ciphertexts decapsulate to K and tampered ones are rejected"""
    rng = np.random.default_rng(salt)
    m = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
    c, K, st = ks.encaps(m, key_index=idx_t, return_status=True)
    gi = torch.from_numpy(np.where(bad, 0, idx).astype(np.int64)).cuda()
    ok = ~bad
    c_ref, K_ref = eng.encaps(ek[gi], m)
    torch.cuda.synchronize()
    c_h, K_h, st_h = c.cpu().numpy(), K.cpu().numpy(), st.cpu().numpy()
    assert (st_h == np.where(bad, ERR_ARG, 0)).all()
    assert (c_h[ok] == c_ref.cpu().numpy()[ok]).all() and (K_h[ok] == K_ref.cpu().numpy()[ok]).all()
    assert not c_h[bad].any() and not K_h[bad].any()
    if not decaps:
        return c_h, K_h
    ct = c.clone()
    ct[::3, 5] ^= 0x10                       # every third ciphertext tampered: implicit rejection
    ct[bad] = c_ref[bad]                     # out-of-range items get a real ciphertext to decapsulate
    K2, st2 = ks.decaps(ct, key_index=idx_t, return_status=True)
    K2_ref, _ = eng.decaps(dk[gi], ct, hash_check=False)
    torch.cuda.synchronize()
    K2_h, K2r = K2.cpu().numpy(), K2_ref.cpu().numpy()
    assert (st2.cpu().numpy() == np.where(bad, ERR_ARG, 0)).all()
    assert (K2_h[ok] == K2r[ok]).all()
    assert not K2_h[bad].any()
    if consistent:
        same = (K2_h == K_h).all(axis=1)
        rej = np.zeros(n, bool)
        rej[::3] = True
        assert same[ok & ~rej].all() and not same[ok & rej].any()
    return c_h, K_h


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("mode", ("reference", "fips203"))
def test_keyset_sizes_and_sources(engine, torch, pkg, oracle, pset, mode):
    """sets from dk, seed and ek (n_keys = 7); n = 1, 2, each small-path limit (wave count and size, Encaps and Decaps) and + 1,
    wide_kem and + 1; random and out-of-range indices, NULL key_index; the oracle on a subset"""
    eng = engine(pset, conformance=mode)
    ek, dk, seed = _keys(eng, torch, 7, 1)
    sets = {"dk": eng.prepare_keys(dk=dk), "seed": eng.prepare_keys(seed=seed), "ek": eng.prepare_keys(ek=ek)}
    assert sets["dk"].has_dk and sets["seed"].has_dk and not sets["ek"].has_dk
    assert sets["dk"].n_keys == 7 and sets["dk"].device_bytes >= 7 * (eng.dk_len + 32 + eng.k * eng.k * 512)
    edges = (KS_ENC_LAT[pset], KS_DEC_LAT[pset], KS_ENC_MAX[pset], KS_DEC_MAX[pset], WIDE_KEM[pset])
    for j, n in enumerate(sorted({1, 2} | {e for x in edges for e in (x, x + 1)})):
        idx_t, idx, bad = _indices(torch, n, 7, 100 * pset + j, n_bad=0 if n < 3 else 5)
        for src, ks in sets.items():
            c_h, K_h = _check_round(eng, torch, ks, ek, dk, n, idx_t, idx, bad, 17 * n + j, decaps=src != "ek")
        if j == 5:   # oracle cross-check on the first 6 valid items
            sel = np.nonzero(~bad)[0][:6]
            rng = np.random.default_rng(17 * n + j)
            m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            oracle.set_conformance(mode == "fips203")
            try:
                c_o, K_o = oracle.encaps(pset, np.ascontiguousarray(ek.cpu().numpy()[idx[sel]]), np.ascontiguousarray(m[sel]))
            finally:
                oracle.set_conformance(False)
            assert (c_h[sel] == c_o).all() and (K_h[sel] == K_o).all()
    # NULL key_index: key 0 for every item
    m = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (40, 32), dtype=np.uint8)).cuda()
    c, K = sets["dk"].encaps(m)
    c_ref, K_ref = eng.encaps(ek[:1].expand(40, -1).contiguous(), m)
    assert torch.equal(c, c_ref) and torch.equal(K, K_ref)
    assert torch.equal(sets["seed"].decaps(c), K_ref)
    with pytest.raises(pkg.MLKEMError) as e:
        sets["ek"].decaps(c)
    assert e.value.code == ERR_ARG
    for ks in sets.values():
        ks.close()


@pytest.mark.parametrize("pset", (512, 768, 1024))
def test_keyset_many_keys_chunked(engine, torch, pset):
    """n_keys = 4096 (the import's chunk loop on 4096-item chunks... and 1024), 2^16 items on a context of 4096-item chunks"""
    eng = engine(pset, chunk_items=4096)
    ek, dk, _ = _keys(eng, torch, 4096, 2)
    with eng.prepare_keys(dk=dk) as ks:
        n = 1 << 16
        idx_t, idx, bad = _indices(torch, n, 4096, 3 * pset, n_bad=9)
        _check_round(eng, torch, ks, ek, dk, n, idx_t, idx, bad, 11)
    eng2 = engine(pset, chunk_items=1024)
    with eng2.prepare_keys(ek=ek) as ks:   # import over four chunks
        idx_t, idx, bad = _indices(torch, 5000, 4096, 5, n_bad=3)
        _check_round(eng2, torch, ks, ek, dk, 5000, idx_t, idx, bad, 12, decaps=False)


@pytest.mark.parametrize("pset", (512, 768, 1024))
def test_keyset_one_key(engine, torch, pset):
    """n_keys = 1: the shared-key special case, also against mlkem_encaps_shared_dev"""
    eng = engine(pset)
    ek, dk, _ = _keys(eng, torch, 1, 3)
    with eng.prepare_keys(dk=dk) as ks:
        for n in (1, KS_DEC_MAX[pset] + 1):
            idx_t, idx, bad = _indices(torch, n, 1, n, n_bad=0)
            c_h, K_h = _check_round(eng, torch, ks, ek, dk, n, idx_t, idx, bad, 13 * n)
            m = torch.from_numpy(np.random.default_rng(13 * n).integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
            c_s, K_s = eng.encaps_shared(ek[0], m)
            assert (c_s.cpu().numpy() == c_h).all() and (K_s.cpu().numpy() == K_h).all()


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("mode", ("reference", "fips203"))
def test_keyset_refusal_matches_check_keys(engine, torch, pkg, pset, mode):
    """corrupted keys: the set is refused (ERR_KEY) with exactly the status words of check_keys on ek or dk alone; classes only the
    seed / PCT legs detect are accepted and still give the per-item results"""
    eng = engine(pset, conformance=mode)
    ek, dk, _ = _keys(eng, torch, 2 * len(CLASSES), 4)
    ek_h, dk_h = ek.cpu().numpy(), dk.cpu().numpy()
    cls = corrupt(pset, ek_h, dk_h, ek_h.shape[0])
    for name, arr in (("ek", ek_h), ("dk", dk_h)):
        t = torch.from_numpy(arr).cuda()
        want = eng.check_keys(**{name: t}).cpu().numpy()
        assert want.any()
        with pytest.raises(pkg.MLKEMError) as e:
            eng.prepare_keys(**{name: t})
        assert e.value.code == ERR_KEY
        assert (e.value.key_status.cpu().numpy() == want).all()
        # the keys that pass on their own form a set whose results equal the per-item calls (dk_z, dk_pke, ek_rho, swap included)
        good = np.nonzero(want == 0)[0]
        assert {cls[i] for i in good} >= ({"valid", "dk_z", "dk_pke", "swap"} if name == "dk" else {"valid", "ek_rho", "swap"})
        keep = torch.from_numpy(np.ascontiguousarray(arr[good])).cuda()
        with eng.prepare_keys(**{name: keep}) as ks:
            k = eng.k   # a dk set encapsulates to the ek embedded in dk
            ek_src = dk_h[good][:, 384 * k:768 * k + 32] if name == "dk" else ek_h[good]
            ekg = torch.from_numpy(np.ascontiguousarray(ek_src)).cuda()
            dkg = torch.from_numpy(np.ascontiguousarray(dk_h[good])).cuda()
            n = 2 * len(good) + 1
            idx_t, idx, bad = _indices(torch, n, len(good), 77, n_bad=1)
            # (dk_pke / swap keys do not decapsulate their own ciphertexts: only equality with the per-item calls is asserted)
            _check_round(eng, torch, ks, ekg, dkg, n, idx_t, idx, bad, 78, decaps=name == "dk", consistent=False)
    # REFERENCE mode's per-item Encaps accepts an ek coefficient >= q; a key set refuses it in both modes
    i = cls.index("ek_q")
    with pytest.raises(pkg.MLKEMError) as e:
        eng.prepare_keys(ek=torch.from_numpy(np.ascontiguousarray(ek_h[i:i + 1])).cuda())
    assert e.value.code == ERR_KEY and int(e.value.key_status[0]) == pkg.KEYCHECK_EK_MODULUS


def test_keyset_two_contexts_side_stream_recreate(engine, torch, pkg):
    """one set from two contexts, one of them on a non-default stream; destroy and re-create gives the same bytes"""
    eng, eng2 = engine(768), engine(768, tag=1)
    ek, dk, seed = _keys(eng, torch, 64, 5)
    ks = eng.prepare_keys(seed=seed)
    n = 500
    idx_t, idx, bad = _indices(torch, n, 64, 6, n_bad=2)
    m = torch.from_numpy(np.random.default_rng(8).integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
    c1, K1 = ks.encaps(m, key_index=idx_t)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c2, K2 = ks.encaps(m, key_index=idx_t, engine=eng2)
        Kd = ks.decaps(c2, key_index=idx_t, engine=eng2)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(c1, c2) and torch.equal(K1, K2) and torch.equal(Kd, K1)
    ks.close()
    ks.close()   # idempotent
    with pytest.raises(pkg.MLKEMError):
        ks.encaps(m, key_index=idx_t)
    with eng.prepare_keys(dk=dk) as ks2:
        c3, K3 = ks2.encaps(m, key_index=idx_t)
        assert torch.equal(c1, c3) and torch.equal(K1, K3)


def test_keyset_cabi_arguments(engine, torch, pkg):
    """C-ABI argument errors, n == 0, info"""
    eng = engine(768)
    lib = pkg.load_library()
    ek, dk, seed = _keys(eng, torch, 3, 9)
    h = C.c_void_p()
    st = torch.empty(3, dtype=torch.int32, device="cuda")
    p = dk.data_ptr()
    assert lib.mlkem_keyset_create(eng._ctx, 768, 3, None, p, None, None, C.byref(h), None) == 0
    ps, nk, hd, nb = C.c_int(), C.c_size_t(), C.c_int(), C.c_size_t()
    assert lib.mlkem_keyset_info(h, C.byref(ps), C.byref(nk), C.byref(hd), C.byref(nb)) == 0
    assert (ps.value, nk.value, hd.value) == (768, 3, 1)
    assert 3 * 7000 <= nb.value <= 3 * 7200 + 3 * 256
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    b = buf.data_ptr()
    assert lib.mlkem_encaps_keyset_dev(eng._ctx, h, 0, None, None, None, None, None, None) == 0
    assert lib.mlkem_encaps_keyset_dev(eng._ctx, None, 1, None, b, b, b, None, None) == ERR_ARG
    assert lib.mlkem_encaps_keyset_dev(eng._ctx, h, 1, None, b + 1, b, b, None, None) == ERR_ARG
    assert lib.mlkem_decaps_keyset_dev(eng._ctx, h, 1, b + 4, b, b, None, None) == ERR_ARG
    lib.mlkem_keyset_destroy(h)
    h2 = C.c_void_p()
    assert lib.mlkem_keyset_create(eng._ctx, 768, 0, None, p, None, None, C.byref(h2), None) == ERR_ARG
    assert lib.mlkem_keyset_create(eng._ctx, 768, 3, ek.data_ptr(), p, None, None, C.byref(h2), None) == ERR_ARG
    assert lib.mlkem_keyset_create(eng._ctx, 768, 3, None, None, None, st.data_ptr(), C.byref(h2), None) == ERR_ARG
    assert lib.mlkem_keyset_create(eng._ctx, 999, 3, None, p, None, None, C.byref(h2), None) == -1
    assert h2.value is None
    assert b"key" in lib.mlkem_strerror(ERR_KEY)
