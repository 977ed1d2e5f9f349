"""GPU tier: deferred implicit rejection in the lane-sliced batch Decaps (k_hash_decaps without J, encrypt2_body in CMP_DEFER mode,
k_hash_j_rejected) against oracle.decaps, bit for bit.

The engines run with chunk_items = 128 and MLKEM_HCHUNK_ITEMS = 512, MLKEM_SMALL_ITEMS = 0, MLKEM_WIDE_HASH_ITEMS = 0 (and
MLKEM_KEYSET_SMALL_ITEMS = 0 for the key-set batch form), so that n = 1031 items run three h-chunks (512 + 512 + 7: three reject
lists, three k_hash_j_rejected launches) of nine chunks with a ragged tail through the lane-sliced kernels.  The oracle runs twice
per parameter set -- every ciphertext untouched, every ciphertext tampered -- and each pattern picks its rows from the two."""
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from conftest import seeds

pytestmark = pytest.mark.gpu
N = 1031
ENV = {"MLKEM_HCHUNK_ITEMS": "512", "MLKEM_SMALL_ITEMS": "0", "MLKEM_WIDE_HASH_ITEMS": "0", "MLKEM_KEYSET_SMALL_ITEMS": "0"}
SETS = ((768, "reference"), (512, "reference"), (1024, "fips203"))
PATTERNS = {
    "none": [],
    "all": list(range(N)),
    "odd": list(range(1, N, 2)),
    "sparse": [0, 63, 64, 511, 512, 1030],
}
ERR_ARG = -101


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


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def make_engine(pkg, pset, mode, env=ENV):
    """an engine whose context read `env` at creation (the limits are per context); the process environment is put back"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.MLKEM(pset, device=0, chunk_items=128, conformance=mode)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def tamper_all(c):
    ct = c.copy()
    i = np.arange(ct.shape[0])
    ct[i, (131 * i + 7) % ct.shape[1]] ^= (1 << (i % 8)).astype(np.uint8)
    return ct


class Case:
    """keys, ciphertexts and the oracle's answers for per-item keys (dk [N]) or one shared key (dk [1])"""

    def __init__(self, oracle, pset, mode, label, shared=False, n_keys=None):
        oracle.set_conformance(mode == "fips203")
        try:
            nk = 1 if shared else (n_keys or N)
            d, z, m = seeds(label + "-d", nk, pset), seeds(label + "-z", nk, pset), seeds(label + "-m", N, pset)
            self.ek, self.dk = oracle.keygen(pset, d, z)
            self.idx = (np.arange(N) % nk).astype(np.uint32)
            dk_rows = np.ascontiguousarray(self.dk[self.idx])
            self.c, self.K_enc = oracle.encaps(pset, np.ascontiguousarray(self.ek[self.idx]), m)
            self.c_all = tamper_all(self.c)
            self.K_none, st0 = oracle.decaps(pset, dk_rows, self.c)
            self.K_all, st1 = oracle.decaps(pset, dk_rows, self.c_all)
        finally:
            oracle.set_conformance(False)
        assert (st0 == 0).all() and (st1 == 0).all() and (self.K_none == self.K_enc).all()
        assert not (self.K_all == self.K_enc).all(axis=1).any()
        for a in (self.ek, self.dk, self.c, self.c_all, self.K_none, self.K_all):
            a.setflags(write=False)

    def pattern(self, name):
        rej = np.zeros(N, bool)
        rej[PATTERNS[name]] = True
        return np.where(rej[:, None], self.c_all, self.c), np.where(rej[:, None], self.K_all, self.K_none)


@pytest.fixture(scope="module")
def cases(oracle):
    return {(pset, mode): Case(oracle, pset, mode, "gdd-%d" % pset) for pset, mode in SETS}


@pytest.fixture(scope="module")
def engines(pkg):
    made = {}

    def get(pset, mode):
        if (pset, mode) not in made:
            made[pset, mode] = make_engine(pkg, pset, mode)
        return made[pset, mode]
    yield get
    for e in made.values():
        e.close()


def decaps_guarded(torch, e, dk, ct, **kw):
    """Decaps into a K / status pair with one guard row behind the n rows"""
    n = ct.shape[0]
    K = torch.full((n + 1, 32), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    if kw.get("hash_check", True):
        e.decaps(dk, ct, K=K[:n], status=st[:n])
    else:
        e.decaps(dk, ct, K=K[:n], hash_check=False)
    torch.cuda.synchronize()
    Kh, sth = host(K), host(st)
    assert (Kh[n] == 0xA5).all() and sth[n] == 0x5A5A5A5A
    return Kh[:n], sth[:n]


def differing(K, K_o):
    return np.nonzero((K != K_o).any(axis=1))[0].tolist()[:16]


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("pset,mode", SETS)
def test_deferred_rejection_patterns(torch, engines, cases, pset, mode, pattern):
    case, e = cases[pset, mode], engines(pset, mode)
    ct, K_o = case.pattern(pattern)
    K, st = decaps_guarded(torch, e, dev(torch, case.dk), dev(torch, ct))
    assert (st == 0).all()
    assert (K == K_o).all(), differing(K, K_o)


def test_rejected_call_leaves_nothing_for_the_next(torch, engines, cases):
    """all rejected, then none rejected, on one context: the second call must not replay the first one's reject lists"""
    case, e = cases[768, "reference"], engines(768, "reference")
    dk = dev(torch, case.dk)
    K1, _ = decaps_guarded(torch, e, dk, dev(torch, case.c_all))
    K2, st2 = decaps_guarded(torch, e, dk, dev(torch, case.c))
    assert (K1 == case.K_all).all(), differing(K1, case.K_all)
    assert (st2 == 0).all() and (K2 == case.K_none).all(), differing(K2, case.K_none)


def test_deferred_rejection_without_hash_check(torch, engines, cases):
    case, e = cases[768, "reference"], engines(768, "reference")
    ct, K_o = case.pattern("sparse")
    K, _ = decaps_guarded(torch, e, dev(torch, case.dk), dev(torch, ct), hash_check=False)
    assert (K == K_o).all(), differing(K, K_o)


@pytest.mark.parametrize("pattern", ("sparse", "all"))
def test_deferred_rejection_shared_key(torch, engines, oracle, pattern):
    e = engines(768, "reference")
    case = Case(oracle, 768, "reference", "gdd-sh", shared=True)
    ct, K_o = case.pattern(pattern)
    K, st = e.decaps_shared(dev(torch, case.dk), dev(torch, ct))
    torch.cuda.synchronize()
    assert (host(st) == 0).all()
    assert (host(K) == K_o).all(), differing(host(K), K_o)


@pytest.mark.parametrize("pattern", ("sparse", "all"))
def test_deferred_rejection_keyset_batch(torch, engines, oracle, pattern):
    """key-set batch Decaps: z read from the set by index.  Item 511 names a key outside the set and its ciphertext is rejected in
    both patterns: zeros and MLKEM_ERR_ARG, whatever k_hash_j_rejected wrote before k_keyset_fix."""
    e = engines(768, "reference")
    case = Case(oracle, 768, "reference", "gdd-ks", n_keys=5)
    ct, K_o = case.pattern(pattern)
    K_o = K_o.copy()
    idx = case.idx.copy()
    idx[511] = 77
    K_o[511] = 0
    with e.prepare_keys(dk=dev(torch, case.dk)) as ks:
        K, st = ks.decaps(dev(torch, ct), key_index=torch.from_numpy(idx.view(np.int32)).cuda(), return_status=True)
        torch.cuda.synchronize()
    assert (host(st) == np.where(np.arange(N) == 511, ERR_ARG, 0)).all()
    assert (host(K) == K_o).all(), differing(host(K), K_o)


@pytest.mark.parametrize("n", (2048, 768), ids=("wide-regime", "small-regime"))
def test_unchanged_forms_still_agree(torch, pkg, cases, n):
    """default environment: 2048 items hash with one sponge per wavefront and blend K' / Kbar, 768 items run one workgroup per item"""
    case = cases[768, "reference"]
    e = pkg.MLKEM(768, device=0, chunk_items=4096)
    try:
        reps = -(-n // N)
        ct_p, K_p = case.pattern("sparse")
        dk = np.tile(case.dk, (reps, 1))[:n]
        ct, K_o = np.tile(ct_p, (reps, 1))[:n], np.tile(K_p, (reps, 1))[:n]
        K, st = decaps_guarded(torch, e, dev(torch, dk), dev(torch, ct))
    finally:
        e.close()
    assert (st == 0).all()
    assert (K == K_o).all(), differing(K, K_o)
