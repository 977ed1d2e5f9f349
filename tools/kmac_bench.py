"""tools/kmac_bench.py -- device time per call of mlkem_kmac_dev (SP 800-185 KMAC over messages of unequal length, mlkem_kmac.hpp)
against mlkem_sha3_ragged_dev SHAKE256 with head = K over the same bodies, written to profiles/kmac.txt:

  (a) 2^20 items: KMAC256 with per-item 32-byte keys (the K rows, in place) over 64-byte bodies, 32 bytes out
                  kdf_onestep (KMAC256, the default 132-byte salt as the shared key, 00000001 || K || body), 32 bytes out
                  SHAKE256(K || body), 32 bytes out: the baseline, unchanged by this feature
      a sample of rows of each is compared with the restatement tests/sp800185_py.py / hashlib
  (b) a call of ONE item of the three, with each kernel form forced (engines created with MLKEM_SHA3_WIDE_ITEMS = 2^30 / 0)

Timing: HIP events around R back-to-back calls on one stream after a warm-up, the median of RUNS such runs; the runs of the calls
that are compared alternate.  Without arguments the tool is a driver that touches no GPU itself: it runs the measurement as a child
process under its own `timeout -k 10` and writes what it printed to --out.

    python tools/kmac_bench.py [--out profiles/kmac.txt]
    python tools/kmac_bench.py --measure            # the measurement, to stdout
"""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 5
LIMIT = 300   # seconds


def engine(pkg, wide=None):
    old = os.environ.get("MLKEM_SHA3_WIDE_ITEMS")
    if wide is not None:
        os.environ["MLKEM_SHA3_WIDE_ITEMS"] = str(wide)
    try:
        return pkg.MLKEM(768, device=0, chunk_items=1024)
    finally:
        if old is None:
            os.environ.pop("MLKEM_SHA3_WIDE_ITEMS", None)
        else:
            os.environ["MLKEM_SHA3_WIDE_ITEMS"] = old


def alternate(torch, fns, R):
    """median us per call of each fn: RUNS rounds, every round times R calls of each fn in turn with events"""
    for fn in fns:
        for _ in range(3):
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
    import sp800185_py as sp
    pkg = ge.load_package()
    rng = np.random.default_rng(185)
    print("kmac_bench: %s, us per call (median of %d runs of R back-to-back calls, HIP events)" % (torch.cuda.get_device_name(0), RUNS))

    def shapes(n):
        K = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).cuda()
        body = torch.from_numpy(rng.integers(0, 256, n * 64, dtype=np.uint8)).cuda()
        off = torch.arange(n, device="cuda", dtype=torch.int64) * 64
        ln = torch.full((n,), 64, device="cuda", dtype=torch.int32)
        return K, body, off, ln

    def calls(eng, K, body, off, ln):
        salt = torch.zeros(132, dtype=torch.uint8, device="cuda")
        return (lambda: eng.kmac(256, K, body, off, ln, outlen=32, custom=b"bench"),
                lambda: eng.kdf_onestep(K, (body, off, ln), 32, salt=salt),
                lambda: eng.sha3("shake256", body, off, ln, head=K, outlen=32))

    def verify(K, body, outs, rows):
        Kh, bh = K.cpu().numpy(), body.cpu().numpy()
        o = [x.cpu().numpy() for x in outs]
        for i in rows:
            k, m = Kh[i].tobytes(), bh[64 * i:64 * i + 64].tobytes()
            assert o[0][i].tobytes() == sp.kmac(256, k, m, 32, b"bench"), i
            assert o[1][i].tobytes() == sp.kdf_onestep(256, k, m, 32), i
            assert o[2][i].tobytes() == hashlib.shake_256(k + m).digest(32), i

    names = ("KMAC256, per-item 32-byte key, 64-byte body", "kdf_onestep, default salt, K || 64-byte body", "SHAKE256(K || 64-byte body)  [baseline]")
    eng = engine(pkg)
    n = 1 << 20
    K, body, off, ln = shapes(n)
    fns = calls(eng, K, body, off, ln)
    verify(K, body, [fn() for fn in fns], (0, 1, 63, 64, n // 2, n - 1))
    t = alternate(torch, fns, 5)
    print("\n(a) n = 2^20 items (one sponge per lane), sampled rows verified")
    for name, us in zip(names, t):
        print("    %-52s %9.1f us   %6.3f x baseline" % (name, us, us / t[2]))
    print("    permutations per item: KMAC256 2 (key block, message), kdf_onestep 1, SHAKE256 1; the call-uniform prefix is absorbed once per call")
    eng.close()
    print("\n(b) n = 1 item")
    for label, wide in (("one sponge per wavefront", 1 << 30), ("one sponge per lane", 0)):
        eng = engine(pkg, wide)
        K, body, off, ln = shapes(1)
        fns = calls(eng, K, body, off, ln)
        verify(K, body, [fn() for fn in fns], (0,))
        t = alternate(torch, fns, 200)
        print("  %s" % label)
        for name, us in zip(names, t):
            print("    %-52s %9.1f us   %6.3f x baseline" % (name, us, us / t[2]))
        eng.close()
    print("    (a KMAC / kdf call is two launches -- prefix kernel, item kernel -- and, with a shared key, the zeroing of the midstate)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmac.txt"))
    ap.add_argument("--measure", action="store_true")
    a = ap.parse_args()
    if a.measure:
        measure()
        return 0
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--measure"], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    sys.stderr.write(r.stderr)
    if r.returncode != 0:
        print("kmac_bench: the measurement ended with status %d; %s not written" % (r.returncode, a.out))
        return 1
    with open(a.out, "w") as f:
        f.write(r.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
