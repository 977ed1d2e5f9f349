"""tools/xwing_bench.py -- device time per call of the batched X25519 and X-Wing calls (mlkem_x25519.hpp, mlkem_xwing.hpp) against the
existing ML-KEM-768 calls on the ML-KEM parts of the same buffers, written to profiles/xwing.txt.  At n = 1, 64, 4096 and 2^20:

  x25519 with an arbitrary u and with the base point
  X-Wing KeyGen, Encaps, Decaps without and with pk
  the yardstick: keygen (d, z of the same sk), encaps (pk_M, eseed[0:32]), decaps_seed (d || z, ct_M) of a FIPS 203 engine

Sampled rows are compared with the restatement tests/x25519_py.py, and Decaps(Encaps) with the sender's secret on every row.
Timing: HIP events around R back-to-back calls on one stream after a warm-up, the median of RUNS such runs; the calls of one size
alternate.  One engine with the default chunk size; a last section sweeps the slice size of the X-Wing calls at 2^20 items (the
launch geometry -- one item per lane, one wave per block -- is assumed, not swept).  Without arguments the tool is a driver that touches no GPU itself: it runs the measurement as a child process under its own
`timeout -k 10` and writes what it printed to --out.

    python tools/xwing_bench.py [--out profiles/xwing.txt]
    python tools/xwing_bench.py --measure            # the measurement, to stdout
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 5
LIMIT = 540   # seconds
SIZES = ((1, 50), (64, 50), (4096, 20), (1 << 20, 2))   # (items, back-to-back calls per timed run)
SLICES = (1 << 14, 1 << 15, 1 << 16, 1 << 17, 1 << 18)


def alternate(torch, fns, R):
    """median us per call of each fn: RUNS rounds, every round times R calls of each fn in turn with events"""
    for fn in fns:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(RUNS):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(R):
                fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3 / R)
    return [statistics.median(t) for t in ts]


def measure():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    import x25519_py as X
    pkg = ge.load_package()
    X.check_pinned()
    rng = np.random.default_rng(25519)
    print("xwing_bench: %s, us per call (median of %d runs of R back-to-back calls, HIP events); ML-KEM-768, FIPS 203 mode"
          % (torch.cuda.get_device_name(0), RUNS))
    eng = pkg.MLKEM(768, device=0, conformance="fips203")
    u8 = torch.uint8
    for n, R in SIZES:
        sk = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
        eseed = torch.from_numpy(rng.integers(0, 256, (n, 64), dtype=np.uint8)).cuda()
        u = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
        pk = eng.xwing_keygen(sk)
        ct, ss = eng.xwing_encaps(pk, eseed)
        assert torch.equal(eng.xwing_decaps(sk, ct), ss) and torch.equal(eng.xwing_decaps(sk, ct, pk=pk), ss)
        out = eng.x25519(sk, u)
        for i in sorted({0, n // 2, n - 1}):
            s, e = bytes(sk[i].cpu().numpy()), bytes(eseed[i].cpu().numpy())
            assert bytes(pk[i].cpu().numpy()) == X.xwing_keygen(s), i
            assert (bytes(ct[i].cpu().numpy()), bytes(ss[i].cpu().numpy())) == X.xwing_encaps(bytes(pk[i].cpu().numpy()), e), i
            assert bytes(out[i].cpu().numpy()) == X.x25519(s, bytes(u[i].cpu().numpy())), i
        # the ML-KEM parts of the same buffers
        off = torch.arange(n, device="cuda", dtype=torch.int64) * 32
        ln = torch.full((n,), 32, device="cuda", dtype=torch.int32)
        seed = eng.sha3("shake256", sk.reshape(-1), off, ln, outlen=64)            # d || z of expand(sk)
        d, z, m = seed[:, :32].contiguous(), seed[:, 32:].contiguous(), eseed[:, :32].contiguous()
        ek, c = pk[:, :1184].contiguous(), ct[:, :1088].contiguous()
        ek_o, dk_o = torch.empty((n, 1184), dtype=u8, device="cuda"), torch.empty((n, 2400), dtype=u8, device="cuda")
        c_o, K_o, K2_o = torch.empty((n, 1088), dtype=u8, device="cuda"), torch.empty((n, 32), dtype=u8, device="cuda"), torch.empty((n, 32), dtype=u8, device="cuda")
        eng.keygen(d, z, ek=ek_o, dk=dk_o)
        eng.encaps(ek, m, c=c_o, K=K_o)
        eng.decaps_seed(seed, c, K=K2_o)
        assert torch.equal(ek_o, ek) and torch.equal(c_o, c) and torch.equal(K2_o, K_o)
        names = ("x25519, arbitrary u", "x25519, base point", "X-Wing KeyGen", "X-Wing Encaps", "X-Wing Decaps", "X-Wing Decaps, pk given",
                 "ML-KEM-768 keygen", "ML-KEM-768 encaps", "ML-KEM-768 decaps_seed")
        fns = (lambda: eng.x25519(sk, u), lambda: eng.x25519(sk), lambda: eng.xwing_keygen(sk), lambda: eng.xwing_encaps(pk, eseed),
               lambda: eng.xwing_decaps(sk, ct), lambda: eng.xwing_decaps(sk, ct, pk=pk),
               lambda: eng.keygen(d, z, ek=ek_o, dk=dk_o), lambda: eng.encaps(ek, m, c=c_o, K=K_o), lambda: eng.decaps_seed(seed, c, K=K2_o))
        t = alternate(torch, fns, R)
        base = {2: t[6], 3: t[7], 4: t[8], 5: t[8]}
        print("\nn = %d items (R = %d), sampled rows verified" % (n, R))
        for k, (name, us) in enumerate(zip(names, t)):
            ratio = "   %6.2f x %s" % (us / base[k], names[{2: 6, 3: 7, 4: 8, 5: 8}[k]]) if k in base else ""
            print("    %-28s %11.1f us   %8.4f us per item%s" % (name, us, us / n, ratio))
        del sk, eseed, u, pk, ct, ss, out, seed, d, z, m, ek, c, ek_o, dk_o, c_o, K_o, K2_o
        torch.cuda.empty_cache()
    eng.close()
    # the slice size of the X-Wing calls (the staging region's capacity): one engine per value, 2^20 items
    n, R = 1 << 20, 2
    sk = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
    eseed = torch.from_numpy(rng.integers(0, 256, (n, 64), dtype=np.uint8)).cuda()
    print("\nslice size of the X-Wing calls (MLKEM_XWING_SLICE_ITEMS), n = 2^20 items: KeyGen / Encaps / Decaps / Decaps with pk, us per call")
    for slice_items in SLICES:
        os.environ["MLKEM_XWING_SLICE_ITEMS"] = str(slice_items)
        try:
            eng = pkg.MLKEM(768, device=0, conformance="fips203")
            pk = eng.xwing_keygen(sk)
            ct, ss = eng.xwing_encaps(pk, eseed)
            assert torch.equal(eng.xwing_decaps(sk, ct), ss)
            t = alternate(torch, (lambda: eng.xwing_keygen(sk), lambda: eng.xwing_encaps(pk, eseed), lambda: eng.xwing_decaps(sk, ct),
                                  lambda: eng.xwing_decaps(sk, ct, pk=pk)), R)
            print("    %8d items per slice  %10.1f %10.1f %10.1f %10.1f" % ((slice_items,) + tuple(t)))
            del pk, ct, ss
            eng.close()
            torch.cuda.empty_cache()
        finally:
            os.environ.pop("MLKEM_XWING_SLICE_ITEMS", None)
    eng = None
    print("\n    (KeyGen and Decaps with pk run one scalar multiplication per item, Encaps and Decaps without pk two, in one launch;")
    print("     an X-Wing call is the ML-KEM call plus one Keccak permutation each for expand / combine, the row copies and the ladder)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xwing.txt"))
    ap.add_argument("--measure", action="store_true")
    a = ap.parse_args()
    if a.measure:
        measure()
        return 0
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--measure"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    if r.returncode != 0:
        print("xwing_bench: the measurement ended with status %d; %s not written" % (r.returncode, a.out))
        return 1
    with open(a.out, "w") as f:
        f.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
