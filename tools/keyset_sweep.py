"""tools/keyset_sweep.py -- where the one-workgroup-per-item key-set kernels (k_encaps_keyset_small / k_decaps_keyset_small) stop
paying, per parameter set and per operation: device-resident key-set Encaps and Decaps (64 keys from dk, random indices) against
the call size, with the small kernels in both forms (MLKEM_KEYSET_SMALL_ITEMS=1000000 and MLKEM_KEYSET_LATENCY_ITEMS=1000000: eight
waves per item; =0: four) and the indexed batch path (MLKEM_KEYSET_SMALL_ITEMS=0).  The limits are read when a context is created,
so each form gets a context of its own.  Figure: us per call, median of 3 runs of R back-to-back calls.  Every point checks that the
three forms give the same bytes.  The last lines derive the limits: small_max = the largest size below the first one where the
batch path is more than 2 % faster; latency = the largest size below the first one where four waves are more than 2 % faster than
eight (the margin keeps run-to-run noise of about 1 % from deciding a limit).

    python tools/keyset_sweep.py [--sets 512,768,1024]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
SIZES = (1, 64, 128, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096)
FORMS = {"small8": ("1000000", "1000000"), "small4": ("1000000", "0"), "batch": ("0", "0")}


def per_call(fn, R):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(R):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / R * 1e6)
    return statistics.median(ts)


def limits(rows, a, b, margin=0.98):
    """largest size before the first one where form b is more than 2 % faster than form a (a is kept up to there)"""
    last = 0
    for n, t in rows:
        if t[b] < margin * t[a]:
            break
        last = n
    return last


ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="512,768,1024")
args = ap.parse_args()
for pset in (int(x) for x in args.sets.split(",")):
    engines = {}
    for form, (small, lat) in FORMS.items():
        os.environ["MLKEM_KEYSET_SMALL_ITEMS"], os.environ["MLKEM_KEYSET_LATENCY_ITEMS"] = small, lat
        engines[form] = pkg.MLKEM(pset, device=0, chunk_items=1 << 16)
    del os.environ["MLKEM_KEYSET_SMALL_ITEMS"], os.environ["MLKEM_KEYSET_LATENCY_ITEMS"]
    e0 = engines["batch"]
    rng = np.random.default_rng(pset)
    d, z = (torch.from_numpy(rng.integers(0, 256, (64, 32), dtype=np.uint8)).cuda() for _ in range(2))
    ek, dk = e0.keygen(d, z)
    ks = e0.prepare_keys(dk=dk)
    print("ML-KEM-%d, us per call | %s" % (pset, " ".join("enc %-7s" % f for f in FORMS) + " | " + " ".join("dec %-7s" % f for f in FORMS)),
          flush=True)
    enc_rows, dec_rows = [], []
    for n in SIZES:
        R = max(5, min(100, 20000 // n))
        idx = torch.from_numpy(rng.integers(0, 64, n).astype(np.int32)).cuda()
        m = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
        te, td, outs = {}, {}, {}
        for form, eng in engines.items():
            c, K = eng._out(n, eng.c_len), eng._out(n, 32)
            te[form] = per_call(lambda: ks.encaps(m, key_index=idx, c=c, K=K, engine=eng), R)
            ct = c.clone()
            ct[::2, 5] ^= 1
            K2 = eng._out(n, 32)
            td[form] = per_call(lambda: ks.decaps(ct, key_index=idx, K=K2, engine=eng), R)
            outs[form] = (c, K, K2)
        ref = outs["batch"]
        for form in FORMS:
            assert all(torch.equal(x, y) for x, y in zip(outs[form], ref)), (pset, n, form)
        enc_rows.append((n, te))
        dec_rows.append((n, td))
        print("%5d %s | %s" % (n, " ".join("%11.1f" % te[f] for f in FORMS), " ".join("%11.1f" % td[f] for f in FORMS)), flush=True)
    best = lambda rows: [(n, {"small": min(t["small8"], t["small4"]), "batch": t["batch"]}) for n, t in rows]
    print("ML-KEM-%d limits: encaps small_max %d latency %d | decaps small_max %d latency %d" % (
        pset, limits(best(enc_rows), "small", "batch"), limits(enc_rows, "small8", "small4"),
        limits(best(dec_rows), "small", "batch"), limits(dec_rows, "small8", "small4")), flush=True)
    ks.close()
    for eng in engines.values():
        eng.close()
