"""tools/keyset_latency.py -- device-resident time per call of the prepared-key-set calls (mlkem_encaps_keyset_dev /
mlkem_decaps_keyset_dev) against the per-item calls on the gathered keys (mlkem_encaps_dev / mlkem_decaps_dev without the hash check,
keys gathered before the timing) and, with one key, the shared-key calls (mlkem_encaps_shared_dev / mlkem_decaps_shared_dev without
the hash check).  ML-KEM-768, n = 1 / 64 / 768 / 4096 / 65536 items, n_keys = 1 and 64 with random indices.  Calls are queued back
to back on one stream; the figure is the median over 5 runs of R calls each (R shrinks with n).  Every run checks that the forms
give equal outputs."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
RUNS = 5
pset = 768


def per_call(fn, R):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        for _ in range(R):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / R * 1e6)
    return statistics.median(ts)


e = pkg.MLKEM(pset, device=0)
print("ML-KEM-%d, us per call (median of %d runs); ratio = key set / per-item" % (pset, RUNS))
print("%7s %6s | %10s %10s %10s %6s | %10s %10s %10s %6s" % ("n", "n_keys", "enc set", "enc item", "enc shared", "ratio",
                                                           "dec set", "dec item", "dec shared", "ratio"), flush=True)
for n_keys in (1, 64):
    rng = np.random.default_rng(n_keys)
    d, z = (torch.from_numpy(rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)).cuda() for _ in range(2))
    ek, dk = e.keygen(d, z)
    ks = e.prepare_keys(dk=dk)
    for n in (1, 64, 768, 4096, 65536):
        R = max(5, min(200, 400000 // (n * 16)))
        idx = torch.from_numpy(rng.integers(0, n_keys, n).astype(np.int32)).cuda()
        m = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
        ekg, dkg = ek[idx.long()].contiguous(), dk[idx.long()].contiguous()
        c_s, K_s = e._out(n, e.c_len), e._out(n, 32)
        c_i, K_i = e._out(n, e.c_len), e._out(n, 32)
        K2_s, K2_i = e._out(n, 32), e._out(n, 32)
        te_s = per_call(lambda: ks.encaps(m, key_index=idx, c=c_s, K=K_s), R)
        te_i = per_call(lambda: e.encaps(ekg, m, c=c_i, K=K_i), R)
        assert torch.equal(c_s, c_i) and torch.equal(K_s, K_i)
        c = c_s.clone()
        c[::2, 5] ^= 1                                   # half the items take the implicit rejection
        td_s = per_call(lambda: ks.decaps(c, key_index=idx, K=K2_s), R)
        td_i = per_call(lambda: e.decaps(dkg, c, K=K2_i, hash_check=False), R)
        assert torch.equal(K2_s, K2_i)
        te_sh = td_sh = float("nan")
        if n_keys == 1:
            te_sh = per_call(lambda: e.encaps_shared(ek[0], m), R)
            td_sh = per_call(lambda: e.decaps_shared(dk[0], c, hash_check=False), R)
            c_sh, K_sh = e.encaps_shared(ek[0], m)
            assert torch.equal(c_sh, c_s) and torch.equal(K_sh, K_s) and torch.equal(e.decaps_shared(dk[0], c, hash_check=False)[0], K2_s)
        print("%7d %6d | %10.1f %10.1f %10.1f %6.2f | %10.1f %10.1f %10.1f %6.2f" % (n, n_keys, te_s, te_i, te_sh, te_s / te_i,
                                                                                   td_s, td_i, td_sh, td_s / td_i), flush=True)
    ks.close()
e.close()
