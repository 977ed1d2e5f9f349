"""GPU tier (-m gpu): decapsulation from 64-byte seed-format keys (d || z, FIPS 203 §3.3) through the C-ABI --
mlkem_decaps_seed_dev / mlkem_decaps_seed -- and MLKEM.decaps_seed.

Every call carries tampered ciphertexts (implicit rejection).  Results must equal, bit for bit, mlkem_keygen_dev followed by
mlkem_decaps_dev (no hash check) on the same device, and the oracle's KeyGen + Decaps on all items of small calls and on a
1024-item subset of large ones.  Sizes straddle small_max (the one-workgroup-per-item kernel k_decaps_seed_small below and at
it, the staged batch composition above it); 2^16 items on a context of 4096-item chunks run the staging loop 16 times."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle.loader import SIZES

pytestmark = pytest.mark.gpu
SMALL_MAX = {512: 1536, 768: 768, 1024: 512}   # Workspace::small_max_k (mlkem_pipeline.hpp)
MLKEM_ERR_PARAM_SET, MLKEM_ERR_ARG = -1, -101


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tier needs a HIP device"
    return torch


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_package()
    p.load_library()
    return p


_engines = {}


@pytest.fixture(scope="module")
def engine(pkg, torch):
    def get(pset, chunk_items=0, conformance="reference"):
        key = (pset, chunk_items, conformance)
        if key not in _engines:
            _engines[key] = pkg.MLKEM(pset, device=0, chunk_items=chunk_items, conformance=conformance)
        return _engines[key]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


def _inputs(eng, torch, n, salt):
    """seeds, ciphertexts (every third one tampered) and Encaps' keys, the key pairs and ciphertexts made on the GPU"""
    rng = np.random.default_rng(1000003 * eng.param_set + 7 * n + salt)
    d, z, m = (rng.integers(0, 256, (n, 32), dtype=np.uint8) for _ in range(3))
    ek, dk = eng.keygen(torch.from_numpy(d), torch.from_numpy(z))
    c, K_enc = eng.encaps(ek, torch.from_numpy(m))
    tampered = np.arange(n) % 3 == 1
    idx = np.nonzero(tampered)[0]
    if idx.size:
        cols = torch.from_numpy((idx * 131) % c.shape[1]).cuda()
        rows = torch.from_numpy(idx).cuda()
        c[rows, cols] ^= 0x10
    seed = np.ascontiguousarray(np.concatenate([d, z], axis=1))
    return seed, d, z, dk, c, K_enc.cpu().numpy(), tampered


def _seed_dev(eng, torch, seed_t, c_t, n):
    K = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = eng.lib.mlkem_decaps_seed_dev(eng._ctx, eng.param_set, n, seed_t.data_ptr(), c_t.data_ptr(), K.data_ptr(), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return K.cpu().numpy()


def _check(eng, torch, oracle, n, salt=0, fips=False):
    pset = eng.param_set
    seed, d, z, dk, c, K_enc, tampered = _inputs(eng, torch, n, salt)
    K = _seed_dev(eng, torch, torch.from_numpy(seed).cuda(), c, n)
    K_two, _ = eng.decaps(dk, c, hash_check=False)             # mlkem_keygen_dev + mlkem_decaps_dev on the same device
    assert (K == K_two.cpu().numpy()).all()
    assert (K[~tampered] == K_enc[~tampered]).all() and (K[tampered] != K_enc[tampered]).any(axis=1).all()
    sub = np.arange(n) if n <= 2048 else np.sort(np.random.default_rng(n).choice(n, 1024, replace=False))
    oracle.set_conformance(fips)
    try:
        _, dk_o = oracle.keygen(pset, d[sub], z[sub])
        K_o, st_o = oracle.decaps(pset, dk_o, c.cpu().numpy()[sub])
    finally:
        oracle.set_conformance(False)
    assert (st_o == 0).all() and (K[sub] == K_o).all()


@pytest.mark.parametrize("pset", (512, 768, 1024))
def test_seed_decaps_sizes_around_small_max(engine, torch, oracle, pset):
    """n = 1, 2, 64, small_max - 1 and small_max (the fused kernel at its eight- and four-wave forms) and small_max + 1
    (KeyGen into the context's staging region, Decaps from it)."""
    eng = engine(pset)
    sm = SMALL_MAX[pset]
    for n in (1, 2, 64, sm - 1, sm, sm + 1):
        _check(eng, torch, oracle, n)


@pytest.mark.parametrize("pset", (512, 768, 1024))
def test_seed_decaps_batch_chunks(engine, torch, oracle, pset):
    """2^16 items on a context of 4096-item chunks: the staging loop runs 16 chunks; oracle on a 1024-item subset."""
    _check(engine(pset, chunk_items=4096), torch, oracle, 1 << 16, salt=1)


def test_seed_decaps_fips203_both_paths(engine, torch, oracle):
    """FIPS 203 conformance (PRF and J on SHAKE256 in both stages), ML-KEM-768: the fused kernel and the batch path."""
    eng = engine(768, conformance="fips203")
    for n in (64, SMALL_MAX[768] + 1):
        _check(eng, torch, oracle, n, salt=2, fips=True)


def test_seed_decaps_host_pointers(engine, torch, oracle):
    """mlkem_decaps_seed (host pointers, an engine lane of the current device): a small call and one above small_max."""
    eng = engine(768)
    for n in (3, SMALL_MAX[768] + 40):
        seed, d, z, dk, c, K_enc, tampered = _inputs(eng, torch, n, 3)
        c_h = np.ascontiguousarray(c.cpu().numpy())
        K = np.zeros((n, 32), np.uint8)
        assert eng.lib.mlkem_decaps_seed(768, n, seed.ctypes.data, c_h.ctypes.data, K.ctypes.data) == 0
        K_two, _ = eng.decaps(dk, c, hash_check=False)
        assert (K == K_two.cpu().numpy()).all()
        assert (K[~tampered] == K_enc[~tampered]).all() and (K[tampered] != K_enc[tampered]).any(axis=1).all()


def test_seed_decaps_python_on_side_stream(engine, torch):
    """MLKEM.decaps_seed is enqueued on torch's current stream: a non-default stream, inputs made on it, read after its sync."""
    eng = engine(1024)
    seed, d, z, dk, c, K_enc, tampered = _inputs(eng, torch, 100, 4)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        seed_t = torch.from_numpy(seed).cuda(non_blocking=False)
        c_t = c.clone()
        K = eng.decaps_seed(seed_t, c_t)
    s.synchronize()
    K = K.cpu().numpy()
    assert K.shape == (100, 32)
    assert (K[~tampered] == K_enc[~tampered]).all() and (K[tampered] != K_enc[tampered]).any(axis=1).all()
    K_two, _ = eng.decaps(dk, c, hash_check=False)
    assert (K == K_two.cpu().numpy()).all()


def test_seed_decaps_argument_errors(engine, torch, pkg):
    """As mlkem_decaps_dev: unknown set -> MLKEM_ERR_PARAM_SET; NULL or misaligned pointers -> MLKEM_ERR_ARG; n = 0 -> OK."""
    eng = engine(768)
    lib, ctx = eng.lib, eng._ctx
    _, _, cl = SIZES[768]
    seed = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    c = torch.zeros((4, cl + 16), dtype=torch.uint8, device="cuda")
    K = torch.zeros((5, 32), dtype=torch.uint8, device="cuda")
    sp, cp, kp = seed.data_ptr(), c.data_ptr(), K.data_ptr()
    assert lib.mlkem_decaps_seed_dev(ctx, 769, 1, sp, cp, kp, None) == MLKEM_ERR_PARAM_SET
    assert lib.mlkem_decaps_seed_dev(ctx, 768, 1, None, cp, kp, None) == MLKEM_ERR_ARG
    assert lib.mlkem_decaps_seed_dev(ctx, 768, 1, sp, None, kp, None) == MLKEM_ERR_ARG
    assert lib.mlkem_decaps_seed_dev(ctx, 768, 1, sp, cp, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_decaps_seed_dev(None, 768, 1, sp, cp, kp, None) == MLKEM_ERR_ARG
    assert lib.mlkem_decaps_seed_dev(ctx, 768, 1, sp + 8, cp, kp, None) == MLKEM_ERR_ARG
    assert lib.mlkem_decaps_seed_dev(ctx, 768, 1, sp, cp + 4, kp, None) == MLKEM_ERR_ARG
    assert lib.mlkem_decaps_seed_dev(ctx, 768, 1, sp, cp, kp + 1, None) == MLKEM_ERR_ARG
    assert lib.mlkem_decaps_seed_dev(ctx, 768, 0, sp, cp, kp, None) == 0
    h = np.zeros(64 * 4, np.uint8)
    assert lib.mlkem_decaps_seed(1000, 1, h.ctypes.data, h.ctypes.data, h.ctypes.data) == MLKEM_ERR_PARAM_SET
    assert lib.mlkem_decaps_seed(768, 1, None, h.ctypes.data, h.ctypes.data) == MLKEM_ERR_ARG
    assert lib.mlkem_decaps_seed(768, 0, None, None, None) == 0
    with pytest.raises(pkg.MLKEMError):
        eng.decaps_seed(seed[:2], c[:3, :cl])
    torch.cuda.synchronize()
