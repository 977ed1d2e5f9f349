"""tools/check_keys_latency.py -- device-resident time of batched key validation (mlkem_check_keys_dev) for ML-KEM-768 at 1 / 64 /
768 / 2^20 items: the structural check alone (ek + dk), + the seed leg (ek + dk + seed), + the PCT (ek + dk + m), against a
hash-checked mlkem_decaps_dev on the same keys (the bar the structural check must stay under).  Calls are queued back to back on
one stream; the figure is the median over 5 runs of R calls each.  Every run checks that valid keys give status 0."""
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
    return statistics.median(ts), min(ts), max(ts)


pset = 768
sizes = [int(x) for x in sys.argv[1:]] or [1, 64, 768, 1 << 20]
for n in sizes:
    R = 200 if n <= 768 else 3
    e = pkg.MLKEM(pset, device=0)
    g = torch.Generator(device="cpu").manual_seed(n)
    d, z, m = (torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g).cuda() for _ in range(3))
    seed = torch.cat([d, z], dim=1).contiguous()
    ek, dk = e.keygen(d, z)
    c, _ = e.encaps(ek, m)
    st = torch.empty(n, dtype=torch.int32, device="cuda")
    K = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    dst = torch.empty(n, dtype=torch.int32, device="cuda")
    rows = [
        ("decaps_dev (hash check)", lambda: e.decaps(dk, c, K=K, status=dst, hash_check=True)),
        ("check ek+dk", lambda: e.check_keys(ek=ek, dk=dk, status=st)),
        ("check ek+dk+seed", lambda: e.check_keys(ek=ek, dk=dk, seed=seed, status=st)),
        ("check ek+dk+m (PCT)", lambda: e.check_keys(ek=ek, dk=dk, m=m, status=st)),
    ]
    out = []
    for name, fn in rows:
        t = per_call(fn, R)
        if name.startswith("check"):
            assert int((st != 0).sum()) == 0, name
        out.append("%s %.1f us [%.1f..%.1f]" % (name, t[0], t[1], t[2]))
    print("ML-KEM-%d n=%d: " % (pset, n) + "  |  ".join(out), flush=True)
    del ek, dk, c, d, z, m, seed, st, K, dst
    e.close()
    torch.cuda.empty_cache()
