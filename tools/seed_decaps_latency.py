"""tools/seed_decaps_latency.py -- device-resident latency of decapsulation from 64-byte seed-format keys (mlkem_decaps_seed_dev)
against the two-call form it replaces (mlkem_keygen_dev into caller buffers, then mlkem_decaps_dev without the hash check), ML-KEM-768
at 1 / 64 / 768 items (all three run the one-workgroup-per-item kernels).  Calls are queued back to back on one stream; the figure
is the median over 5 runs of R calls each.  Every run checks that both forms give the same keys."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
R, RUNS = 200, 5


def per_call(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        for _ in range(R):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / R * 1e6)
    return statistics.median(ts), min(ts), max(ts)


pset = 768
for n in (1, 64, 768):
    e = pkg.MLKEM(pset, device=0)
    rng = np.random.default_rng(n)
    d, z, m = (torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda() for _ in range(3))
    seed = torch.cat([d, z], dim=1).contiguous()
    ek, dk = e.keygen(d, z)
    c, K = e.encaps(ek, m)
    c[::2, 5] ^= 1                                   # half the items take the implicit rejection
    K_two, K_seed = torch.empty_like(K), torch.empty_like(K)
    ek2, dk2 = torch.empty_like(ek), torch.empty_like(dk)

    def two():
        e.keygen(d, z, ek=ek2, dk=dk2)
        e.decaps(dk2, c, K=K_two, hash_check=False)

    def fused():
        e.decaps_seed(seed, c, K=K_seed)

    t2 = per_call(two)
    tf = per_call(fused)
    assert torch.equal(K_two, K_seed)
    print("ML-KEM-%d n=%d: keygen_dev + decaps_dev %.1f us [%.1f..%.1f]  decaps_seed_dev %.1f us [%.1f..%.1f]  ratio %.2f"
          % (pset, n, t2[0], t2[1], t2[2], tf[0], tf[1], tf[2], tf[0] / t2[0]), flush=True)
    e.close()
