"""tools/rng_latency.py -- device-resident time per call of the randomised calls (mlkem_keygen_random_dev, mlkem_encaps_random_dev,
mlkem_encaps_keyset_random_dev: seeds derived on the device) against their seeded siblings on seeds already resident
(mlkem_keygen_dev, mlkem_encaps_dev, mlkem_encaps_keyset_dev), through the C-ABI on preallocated tensors.  ML-KEM-768,
n = 1 / 64 / 768 / 4096 / 65536 / 2^20.  Calls are queued back to back on one stream; a run is R calls (R shrinks with n) ended by a
synchronise; the two forms alternate run by run and the figure is the median of RUNS runs each.  Every size checks that the random
call equals the seeded call on the hashlib seeds (n <= 4096) and on its own seed_out (all sizes).

    python tools/rng_latency.py            # the table above, then the host-pointer mlkem_keygen_random / mlkem_encaps_random
    python tools/rng_latency.py --sweep    # the derivation-form sweep: k_rng_derive alone (HIP events) and the whole Encaps call,
                                           # one sponge per wavefront against lane-sliced, n = 64 .. 16384
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/rng_latency.py --trace keyset-random   # or keyset-seeded, keygen-random,
                                           # keygen-seeded, encaps-random, encaps-seeded: 10 calls of 2^20 items, for a kernel trace
"""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
RUNS = 7
pset = 768
ROOT = hashlib.sha256(b"rng-latency").digest()


def alternate(fns, R):
    """median us per call of each fn: RUNS rounds, every round times R calls of each fn in turn"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(RUNS):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(R):
                fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) / R * 1e6)
    return [statistics.median(t) for t in ts]


def reps(n):
    return max(5, min(200, 400000 // (n * 16)))


def blocks(dom, pos, n, nbytes):
    return np.frombuffer(b"".join(hashlib.shake_256(ROOT + bytes([dom]) + (pos + i).to_bytes(8, "little")).digest(nbytes)
                                  for i in range(n)), np.uint8).reshape(n, nbytes).copy()


def u8(*shape):
    return torch.empty(shape, dtype=torch.uint8, device="cuda")


def main_table():
    e = pkg.MLKEM(pset, device=0)
    lib, ctx, st = e.lib, e._ctx, e._stream()
    n_keys = 64
    e.rng_seed(ROOT)
    _, ks_seed = e.keygen_random(n_keys, return_seed=True, dk=False)
    ks = e.prepare_keys(seed=ks_seed)
    print("ML-KEM-%d, us per call (median of %d runs, forms alternating); ratio = random / seeded; +us = random - seeded" % (pset, RUNS))
    print("%8s | %10s %10s %6s %7s | %10s %10s %6s %7s | %10s %10s %6s %7s" % (
        "n", "kg random", "kg seeded", "ratio", "+us", "enc random", "enc seeded", "ratio", "+us", "ks random", "ks seeded", "ratio", "+us"), flush=True)
    for n in (1, 64, 768, 4096, 65536, 1 << 20):
        R = reps(n)
        ek, dk, seed, ek2, dk2 = u8(n, e.ek_len), u8(n, e.dk_len), u8(n, 64), u8(n, e.ek_len), u8(n, e.dk_len)
        # correctness first: positions 0 .. n - 1 of a fresh stream
        e.rng_seed(ROOT)
        e._check(lib.mlkem_keygen_random_dev(ctx, pset, n, ek.data_ptr(), dk.data_ptr(), seed.data_ptr(), st))
        d, z = seed[:, :32].contiguous(), seed[:, 32:].contiguous()
        e._check(lib.mlkem_keygen_dev(ctx, pset, n, d.data_ptr(), z.data_ptr(), ek2.data_ptr(), dk2.data_ptr(), st))
        assert torch.equal(ek, ek2) and torch.equal(dk, dk2)
        if n <= 4096:
            assert (seed.cpu().numpy() == blocks(1, 0, n, 64)).all()
        t_kr, t_ks = alternate([
            lambda: lib.mlkem_keygen_random_dev(ctx, pset, n, ek.data_ptr(), dk.data_ptr(), None, st),
            lambda: lib.mlkem_keygen_dev(ctx, pset, n, d.data_ptr(), z.data_ptr(), ek2.data_ptr(), dk2.data_ptr(), st)], R)
        del dk, dk2, ek2
        c, K, c2, K2 = u8(n, e.c_len), u8(n, 32), u8(n, e.c_len), u8(n, 32)
        m = u8(n, 32)
        m.copy_(d)
        t_er, t_es = alternate([
            lambda: lib.mlkem_encaps_random_dev(ctx, pset, n, ek.data_ptr(), c.data_ptr(), K.data_ptr(), None, st),
            lambda: lib.mlkem_encaps_dev(ctx, pset, n, ek.data_ptr(), m.data_ptr(), c2.data_ptr(), K2.data_ptr(), st)], R)
        if n <= 4096:
            e.rng_seed(ROOT)
            e._check(lib.mlkem_encaps_random_dev(ctx, pset, n, ek.data_ptr(), c.data_ptr(), K.data_ptr(), None, st))
            mh = torch.from_numpy(blocks(2, 0, n, 32)).cuda()
            e._check(lib.mlkem_encaps_dev(ctx, pset, n, ek.data_ptr(), mh.data_ptr(), c2.data_ptr(), K2.data_ptr(), st))
            assert torch.equal(c, c2) and torch.equal(K, K2)
        idx = torch.from_numpy(np.random.default_rng(n).integers(0, n_keys, n).astype(np.int32)).cuda()
        t_sr, t_ss = alternate([
            lambda: lib.mlkem_encaps_keyset_random_dev(ctx, ks._h, n, idx.data_ptr(), c.data_ptr(), K.data_ptr(), None, st),
            lambda: lib.mlkem_encaps_keyset_dev(ctx, ks._h, n, idx.data_ptr(), m.data_ptr(), c2.data_ptr(), K2.data_ptr(), None, st)], R)
        print("%8d | %10.1f %10.1f %6.3f %7.1f | %10.1f %10.1f %6.3f %7.1f | %10.1f %10.1f %6.3f %7.1f" % (
            n, t_kr, t_ks, t_kr / t_ks, t_kr - t_ks, t_er, t_es, t_er / t_es, t_er - t_es, t_sr, t_ss, t_sr / t_ss, t_sr - t_ss), flush=True)
        del ek, seed, d, z, c, K, c2, K2, m, idx
        torch.cuda.empty_cache()
    ks.close()
    e.close()


def host_table():
    """the host-pointer wrappers: seeds from getrandom(2) 256 bytes per system call, pageable host buffers, synchronous"""
    lib = pkg.load_library()
    ekl, dkl, cl = pkg.SIZES[pset]
    print("\nhost-pointer mlkem_keygen_random / mlkem_encaps_random, us per call (median of 5 calls after one warm-up) and items/s")
    print("%8s | %12s %12s | %12s %12s" % ("n", "keygen us", "pairs/s", "encaps us", "items/s"), flush=True)
    for n in (1, 64, 768, 4096, 65536, 1 << 20):
        ek, dk = np.empty((n, ekl), np.uint8), np.empty((n, dkl), np.uint8)
        c, K = np.empty((n, cl), np.uint8), np.empty((n, 32), np.uint8)
        out = []
        for fn in (lambda: lib.mlkem_keygen_random(pset, n, ek.ctypes.data, dk.ctypes.data),
                   lambda: lib.mlkem_encaps_random(pset, n, ek.ctypes.data, ekl, c.ctypes.data, K.ctypes.data)):
            assert fn() == 0
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                rc = fn()
                ts.append((time.perf_counter() - t0) * 1e6)
                assert rc == 0
            out.append(statistics.median(ts))
        print("%8d | %12.1f %12.3g | %12.1f %12.3g" % (n, out[0], n / out[0] * 1e6, out[1], n / out[1] * 1e6), flush=True)
    lib.mlkem_host_release()


def sweep():
    """one engine per derivation form (MLKEM_RNG_WIDE_ITEMS is read when a context is created)"""
    engines = {}
    for name, lim in (("wave", str(1 << 30)), ("lane", "0")):
        os.environ["MLKEM_RNG_WIDE_ITEMS"] = lim
        engines[name] = pkg.MLKEM(pset, device=0, chunk_items=16384)
    del os.environ["MLKEM_RNG_WIDE_ITEMS"]
    for e in engines.values():
        e.rng_seed(ROOT)
    base = engines["wave"]
    ek_all = base.keygen_random(16384)[0]
    print("derivation-form sweep, ML-KEM-%d: k_rng_derive alone (HIP events round each launch, us per launch, median of %d runs) and the" % (pset, RUNS))
    print("whole mlkem_encaps_random_dev / mlkem_keygen_random_dev call (us per call); wave = one sponge per wavefront, lane = lane-sliced")
    print("%6s | %9s %9s | %9s %9s | %9s %9s" % ("n", "drv wave", "drv lane", "enc wave", "enc lane", "kg wave", "kg lane"), flush=True)
    for n in (64, 256, 512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192, 12288, 16384):
        R = max(5, min(100, 200000 // (n * 16)))
        ek = ek_all[:n].contiguous()
        c, K = u8(n, base.c_len), u8(n, 32)
        ek_o, dk_o = u8(n, base.ek_len), u8(n, base.dk_len)
        fe, fk, drv = [], [], {}
        for name, e in engines.items():
            lib, ctx, st = e.lib, e._ctx, e._stream()
            fe.append(lambda lib=lib, ctx=ctx, st=st: lib.mlkem_encaps_random_dev(ctx, pset, n, ek.data_ptr(), c.data_ptr(), K.data_ptr(), None, st))
            fk.append(lambda lib=lib, ctx=ctx, st=st: lib.mlkem_keygen_random_dev(ctx, pset, n, ek_o.data_ptr(), dk_o.data_ptr(), None, st))
        te, tk = alternate(fe, R), alternate(fk, R)
        for k, name in enumerate(engines):
            per = []
            for _ in range(RUNS):
                with pkg.kernel_timing() as kt:
                    for _ in range(R):
                        fe[k]()
                ms, cnt = kt.rows["k_rng_derive"]
                per.append(ms / cnt * 1e3)
            drv[name] = statistics.median(per)
        print("%6d | %9.2f %9.2f | %9.1f %9.1f | %9.1f %9.1f" % (n, drv["wave"], drv["lane"], te[0], te[1], tk[0], tk[1]), flush=True)
    for e in engines.values():
        e.close()


def trace(case, n=1 << 20, calls=10):
    """`calls` calls of one form at n items and nothing else on the device besides the set-up: for rocprofv3 --kernel-trace --stats"""
    op, form = case.split("-")
    e = pkg.MLKEM(pset, device=0)
    lib, ctx, st = e.lib, e._ctx, e._stream()
    e.rng_seed(ROOT)
    ek, seed = e.keygen_random(n, return_seed=True, dk=False)
    d, z, m = seed[:, :32].contiguous(), seed[:, 32:].contiguous(), seed[:, 32:].contiguous()
    c, K = u8(n, e.c_len), u8(n, 32)
    if op == "keygen":
        dk = u8(n, e.dk_len)
        fn = (lambda: lib.mlkem_keygen_random_dev(ctx, pset, n, ek.data_ptr(), dk.data_ptr(), None, st)) if form == "random" else \
             (lambda: lib.mlkem_keygen_dev(ctx, pset, n, d.data_ptr(), z.data_ptr(), ek.data_ptr(), dk.data_ptr(), st))
    elif op == "encaps":
        fn = (lambda: lib.mlkem_encaps_random_dev(ctx, pset, n, ek.data_ptr(), c.data_ptr(), K.data_ptr(), None, st)) if form == "random" else \
             (lambda: lib.mlkem_encaps_dev(ctx, pset, n, ek.data_ptr(), m.data_ptr(), c.data_ptr(), K.data_ptr(), st))
    else:
        ks = e.prepare_keys(seed=seed[:64].contiguous())
        idx = torch.from_numpy(np.random.default_rng(n).integers(0, 64, n).astype(np.int32)).cuda()
        fn = (lambda: lib.mlkem_encaps_keyset_random_dev(ctx, ks._h, n, idx.data_ptr(), c.data_ptr(), K.data_ptr(), None, st)) if form == "random" else \
             (lambda: lib.mlkem_encaps_keyset_dev(ctx, ks._h, n, idx.data_ptr(), m.data_ptr(), c.data_ptr(), K.data_ptr(), None, st))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        assert fn() == 0
    torch.cuda.synchronize()
    print("%s: %d calls of %d items, %.1f us per call" % (case, calls, n, (time.perf_counter() - t0) / calls * 1e6))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", choices=[o + "-" + f for o in ("keygen", "encaps", "keyset") for f in ("random", "seeded")])
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    if a.trace:
        trace(a.trace)
    elif a.sweep:
        sweep()
    else:
        main_table()
        if not a.no_host:
            host_table()
