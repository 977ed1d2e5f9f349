"""GPU tier (-m gpu): batched key validation through the C-ABI -- mlkem_check_keys_dev / mlkem_check_keys -- and MLKEM.check_keys.

Key pairs come from the GPU's KeyGen; item i then gets corruption class i % 9 of tests/keycheck_cases.py (valid, ek coefficient
q / 4095, dk.ek coefficient >= q, dk.h, dk.z, dk_pke and ek rho byte flips, swapped dks).  Every status word is compared with one
computed independently (numpy ByteDecode_12, hashlib SHA3-256, byte comparison, the oracle's KeyGen and Encaps + Decaps_internal in
the context's conformance mode), on all items of calls up to 2048 items and on a 1024-item subset of larger ones.  Sizes straddle
small_max (the legs' one-workgroup-per-item kernels) and wide_kem (in-kernel wave-wide hash below and at it, the lane-sliced
pre-pass above); 2^16 items on a context of 4096-item chunks run the staging loop many times."""
import numpy as np
import pytest

from keycheck_cases import COMBOS, CLASSES, corrupt, expected, check_against, SEED, PCT
from oracle.loader import SIZES

pytestmark = pytest.mark.gpu
SMALL_MAX = {512: 1536, 768: 768, 1024: 512}   # Workspace::small_max_k (mlkem_pipeline.hpp)
WIDE_KEM = {512: 4096, 768: 3072, 1024: 4096}  # Workspace::wide_max_k
MLKEM_ERR_PARAM_SET, MLKEM_ERR_ARG = -1, -101


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
    def get(pset, chunk_items=0, conformance="reference"):
        key = (pset, chunk_items, conformance)
        if key not in _engines:
            _engines[key] = pkg.MLKEM(pset, device=0, chunk_items=chunk_items, conformance=conformance)
        return _engines[key]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


def _batch(eng, torch, n, salt):
    """n key pairs from the GPU KeyGen of this engine's mode, corrupted by class (host arrays); seed = d || z, m random"""
    rng = np.random.default_rng(1000003 * eng.param_set + 7 * n + salt)
    d, z, m = (rng.integers(0, 256, (n, 32), dtype=np.uint8) for _ in range(3))
    ek, dk = eng.keygen(torch.from_numpy(d), torch.from_numpy(z))
    ek, dk = ek.cpu().numpy(), dk.cpu().numpy()
    cls = corrupt(eng.param_set, ek, dk, n)
    return dict(ek=ek, dk=dk, seed=np.ascontiguousarray(np.concatenate([d, z], axis=1)), m=m), cls


def _given(batch, names):
    return {x: (batch[x] if x in names else None) for x in ("ek", "dk", "seed", "m")}


def _run(eng, torch, given):
    kw = {x: (None if a is None else torch.from_numpy(a).cuda()) for x, a in given.items()}
    st = eng.check_keys(**kw)
    torch.cuda.synchronize()
    return st.cpu().numpy()


def _verify(eng, oracle, given, cls, names, got):
    n = got.shape[0]
    fips = eng.conformance == "fips203"
    sub = np.arange(n) if n <= 2048 else np.sort(np.random.default_rng(n).choice(n, 1024, replace=False))
    try:
        exp = expected(oracle, eng.param_set, fips, given, sub)
    finally:
        oracle.set_conformance(False)
    check_against(got[sub], exp, [cls[i] for i in sub], names)


@pytest.mark.parametrize("pset", (512, 768, 1024))
@pytest.mark.parametrize("conformance", ("reference", "fips203"))
def test_check_keys_every_combination(engine, torch, oracle, pset, conformance):
    """Every optional-argument combination, both conformance modes, 64 items (the legs' small-call kernels, in-kernel hash)."""
    eng = engine(pset, conformance=conformance)
    batch, cls = _batch(eng, torch, 64, 1)
    for combo, names in COMBOS.items():
        given = _given(batch, names)
        _verify(eng, oracle, given, cls, names, _run(eng, torch, given))


@pytest.mark.parametrize("pset", (512, 768, 1024))
def test_check_keys_sizes(engine, torch, oracle, pset):
    """n = 1, small_max, small_max + 1, wide_kem and wide_kem + 1: the structural check alone and with both legs."""
    eng = engine(pset)
    sm, wk = SMALL_MAX[pset], WIDE_KEM[pset]
    for n in (1, sm, sm + 1, wk, wk + 1):
        batch, cls = _batch(eng, torch, n, 2)
        for combo in ("ek+dk", "all"):
            names = COMBOS[combo]
            given = _given(batch, names)
            _verify(eng, oracle, given, cls, names, _run(eng, torch, given))


@pytest.mark.parametrize("pset", (512, 768, 1024))
def test_check_keys_batch_chunks(engine, torch, oracle, pset):
    """2^16 items on a context of 4096-item chunks: staging rounds of 4096 items, of 3056 for ML-KEM-1024 with all four inputs
    (6432 of the region's 4800 bytes per item); the oracle on a 1024-item subset."""
    eng = engine(pset, chunk_items=4096)
    batch, cls = _batch(eng, torch, 1 << 16, 3)
    for combo in ("dk", "all"):
        names = COMBOS[combo]
        given = _given(batch, names)
        _verify(eng, oracle, given, cls, names, _run(eng, torch, given))


def test_check_keys_fips203_above_wide(engine, torch, oracle):
    """FIPS 203 mode above wide_kem (lane-sliced hash, batch KeyGen / Encaps / Decaps with SHAKE256 PRF and J), ML-KEM-768."""
    eng = engine(768, conformance="fips203")
    batch, cls = _batch(eng, torch, WIDE_KEM[768] + 1, 4)
    names = COMBOS["all"]
    given = _given(batch, names)
    _verify(eng, oracle, given, cls, names, _run(eng, torch, given))


def test_check_keys_host_pointers_equal_device(engine, torch):
    """mlkem_check_keys (host pointers, an engine lane of the current device) gives the device call's words: a small call and
    one above small_max, every combination."""
    eng = engine(768)
    for n in (9, SMALL_MAX[768] + 40):
        batch, cls = _batch(eng, torch, n, 5)
        for combo, names in COMBOS.items():
            given = _given(batch, names)
            dev = _run(eng, torch, given)
            st = np.full(n, -1, np.int32)
            ptr = [None if given[x] is None else given[x].ctypes.data for x in ("ek", "dk", "seed", "m")]
            assert eng.lib.mlkem_check_keys(768, n, *ptr, st.ctypes.data) == 0
            assert (st == dev).all(), combo


def test_check_keys_python_on_side_stream(engine, torch):
    """MLKEM.check_keys is enqueued on torch's current stream: a non-default stream, inputs made on it, read after its sync."""
    eng = engine(1024)
    batch, cls = _batch(eng, torch, 100, 6)
    ref = _run(eng, torch, _given(batch, COMBOS["all"]))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        kw = {x: torch.from_numpy(batch[x]).cuda() for x in ("ek", "dk", "seed", "m")}
        st = eng.check_keys(**kw)
    s.synchronize()
    st = st.cpu().numpy()
    assert (st == ref).all()
    assert (st[np.array([c == "valid" for c in cls])] == 0).all()


def test_check_keys_leaves_staging_usable_for_decaps_seed(engine, torch):
    """A check call with both legs, then mlkem_decaps_seed_dev above small_max on the same context (they share the staging
    region): the keys equal the two-call form mlkem_keygen_dev + mlkem_decaps_dev."""
    eng = engine(768)
    n = SMALL_MAX[768] + 7
    batch, _ = _batch(eng, torch, n, 7)
    _run(eng, torch, _given(batch, COMBOS["all"]))
    rng = np.random.default_rng(8)
    d, z, m = (torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda() for _ in range(3))
    ek, dk = eng.keygen(d, z)
    c, _ = eng.encaps(ek, m)
    c[::2, 3] ^= 1
    K_seed = eng.decaps_seed(torch.cat([d, z], dim=1).contiguous(), c)
    K_two, _ = eng.decaps(dk, c, hash_check=False)
    torch.cuda.synchronize()
    assert torch.equal(K_seed, K_two)


def test_check_keys_argument_errors(engine, torch, pkg):
    """As the other entry points: unknown set -> MLKEM_ERR_PARAM_SET; NULL status, neither ek nor dk, m without dk, NULL or
    misaligned context / pointers -> MLKEM_ERR_ARG; n = 0 -> OK (device and host pointers)."""
    eng = engine(768)
    lib, ctx = eng.lib, eng._ctx
    ekl, dkl, _ = SIZES[768]
    buf = torch.zeros((4, dkl + 64), dtype=torch.uint8, device="cuda")
    st = torch.zeros(8, dtype=torch.int32, device="cuda")
    ek, dk, sd, m, sp = buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(), st.data_ptr()
    f = lib.mlkem_check_keys_dev
    assert f(ctx, 769, 1, ek, dk, sd, m, sp, None) == MLKEM_ERR_PARAM_SET
    assert f(ctx, 768, 1, ek, dk, sd, m, None, None) == MLKEM_ERR_ARG
    assert f(ctx, 768, 1, None, None, sd, None, sp, None) == MLKEM_ERR_ARG
    assert f(ctx, 768, 1, ek, None, None, m, sp, None) == MLKEM_ERR_ARG
    assert f(None, 768, 1, ek, dk, None, None, sp, None) == MLKEM_ERR_ARG
    assert f(ctx, 768, 1, ek + 8, dk, None, None, sp, None) == MLKEM_ERR_ARG
    assert f(ctx, 768, 1, ek, dk + 4, None, None, sp, None) == MLKEM_ERR_ARG
    assert f(ctx, 768, 1, ek, dk, sd + 1, None, sp, None) == MLKEM_ERR_ARG
    assert f(ctx, 768, 1, ek, dk, None, m + 2, sp, None) == MLKEM_ERR_ARG
    assert f(ctx, 768, 1, ek, dk, None, None, sp + 2, None) == MLKEM_ERR_ARG
    assert f(ctx, 768, 0, ek, dk, sd, m, sp, None) == 0
    assert f(ctx, 768, 0, None, None, None, None, None, None) == 0
    h = np.zeros(dkl * 2, np.uint8)
    hs = np.zeros(2, np.int32)
    assert lib.mlkem_check_keys(1000, 1, h.ctypes.data, None, None, None, hs.ctypes.data) == MLKEM_ERR_PARAM_SET
    assert lib.mlkem_check_keys(768, 1, None, None, None, None, hs.ctypes.data) == MLKEM_ERR_ARG
    assert lib.mlkem_check_keys(768, 1, h.ctypes.data, None, None, h.ctypes.data, hs.ctypes.data) == MLKEM_ERR_ARG
    assert lib.mlkem_check_keys(768, 1, h.ctypes.data, None, None, None, None) == MLKEM_ERR_ARG
    assert lib.mlkem_check_keys(768, 0, None, None, None, None, None) == 0
    with pytest.raises(pkg.MLKEMError):
        eng.check_keys()
    with pytest.raises(pkg.MLKEMError):
        eng.check_keys(ek=buf[:2, :ekl], m=buf[:2, :32])
    with pytest.raises(pkg.MLKEMError):
        eng.check_keys(ek=buf[:2, :ekl], dk=buf[:3, :dkl])
    assert eng.check_keys(ek=buf[:0, :ekl]).shape == (0,)
    torch.cuda.synchronize()
