"""tools/sha3_ragged_bench.py -- device time per call of mlkem_sha3_ragged_dev (SHA-3 / SHAKE over messages of unequal length,
mlkem_sha3r.hpp) for SHA3-256 and SHAKE128, written to profiles/sha3_ragged.txt:

  (a) 2^20 equal-length, 8-byte aligned messages of 1184 bytes through the new call against mlkem_hash_dev (k_hash_batch, the
      equal-length kernel) on the same buffer; the outputs of the two must be equal
  (b) the same byte volume as 2^20 messages with lengths uniform in [0, 2368] packed back to back (random byte offsets); a sample of
      rows is compared with hashlib
  (c) n = 64 .. 16384 with each kernel form forced (engines created with MLKEM_SHA3_WIDE_ITEMS = 0 / 2^30), for two shapes: a
      32-byte head + a body uniform in [0, 256] (a shared secret hashed with a session context), and 1184-byte messages
  (d) a call of one item (32-byte head + 100-byte body), each form

Timing: HIP events around R back-to-back calls on one stream after a warm-up, the median of RUNS such runs; where two things are
compared their runs alternate.  Without arguments the tool is a driver that touches no GPU itself: it runs every section as a child
process under its own `timeout -k 10`, stops at the first one that fails, and writes what the sections printed to --out.

    python tools/sha3_ragged_bench.py [--out profiles/sha3_ragged.txt]
    python tools/sha3_ragged_bench.py --section a|b|c|d        # one section, to stdout
"""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = 5
ALGS = (("sha3_256", 0, 32), ("shake128", 2, 32))      # name, mlkem_hash_dev kind of the same function, output bytes
SECTION_LIMIT = {"a": 240, "b": 300, "c": 300, "d": 120}   # seconds


def setup():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    return np, torch, pkg


def engine(pkg, wide=None):
    """an engine with the form switch at its default (wide None), or forced: 0 = always one sponge per lane, 2^30 = per wavefront"""
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


class Call:
    """a prepared mlkem_sha3_ragged_dev call on preallocated tensors"""

    def __init__(self, torch, pkg, eng, alg, body, offs, lens, head=None, outlen=32):
        self.eng, self.code = eng, pkg.SHA3_ALGS[alg][0]
        self.body, self.offs, self.lens, self.head = body, offs, lens, head
        self.n, self.outlen = offs.numel(), outlen
        self.out = torch.empty((self.n, outlen), dtype=torch.uint8, device="cuda")
        self.st = eng._stream()

    def __call__(self):
        h = self.head
        rc = self.eng.lib.mlkem_sha3_ragged_dev(self.eng._ctx, self.code, self.n, None if h is None else h.data_ptr(),
                                                0 if h is None else h.shape[1], 0 if h is None else h.stride(0), self.body.data_ptr(),
                                                self.body.numel(), self.offs.data_ptr(), self.lens.data_ptr(), self.out.data_ptr(),
                                                self.outlen, self.outlen, None, self.st)
        assert rc == 0, rc


def check_rows(np, alg, call, body_h, offs_h, lens_h, head_h, rows):
    out = call.out.cpu().numpy()
    fn = getattr(hashlib, alg.replace("shake", "shake_"))
    for i in rows:
        msg = (head_h[i].tobytes() if head_h is not None else b"") + body_h[int(offs_h[i]):int(offs_h[i]) + int(lens_h[i])].tobytes()
        h = fn(msg)
        assert out[i].tobytes() == (h.digest(call.outlen) if alg.startswith("shake") else h.digest()), (alg, i)


def section_a():
    np, torch, pkg = setup()
    eng = engine(pkg)
    n, ln = 1 << 20, 1184
    g = torch.Generator(device="cuda").manual_seed(1)
    msgs = torch.randint(0, 256, (n, ln), dtype=torch.uint8, device="cuda", generator=g)
    offs = torch.arange(n, device="cuda", dtype=torch.int64) * ln
    lens = torch.full((n,), ln, device="cuda", dtype=torch.int32)
    print("(a) n = 2^20 messages of 1184 bytes, 8-byte aligned rows, us per call (median of %d runs of R = 5 calls, alternating)" % RUNS)
    print("%10s | %14s %14s %7s | %10s" % ("alg", "sha3_ragged", "mlkem_hash_dev", "ratio", "GB/s new"), flush=True)
    for alg, kind, outlen in ALGS:
        new = Call(torch, pkg, eng, alg, msgs.reshape(-1), offs, lens, outlen=outlen)
        ref_out = torch.empty((n, outlen), dtype=torch.uint8, device="cuda")
        st = eng._stream()

        def old():
            rc = eng.lib.mlkem_hash_dev(eng._ctx, kind, n, msgs.data_ptr(), ln, ln, ref_out.data_ptr(), st)
            assert rc == 0, rc
        new()
        old()
        torch.cuda.synchronize()
        assert torch.equal(new.out, ref_out), alg
        t_new, t_old = alternate(torch, [new, old], 5)
        print("%10s | %14.1f %14.1f %7.3f | %10.1f" % (alg, t_new, t_old, t_new / t_old, n * ln / t_new / 1e3), flush=True)
    eng.close()


def section_b():
    np, torch, pkg = setup()
    eng = engine(pkg)
    n = 1 << 20
    rng = np.random.default_rng(2)
    lens_h = rng.integers(0, 2369, n).astype(np.uint32)
    offs_h = np.zeros(n, np.uint64)
    offs_h[1:] = np.cumsum(lens_h[:-1], dtype=np.uint64)
    offs_h += 3
    total = int(offs_h[-1]) + int(lens_h[-1])
    g = torch.Generator(device="cuda").manual_seed(2)
    body = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda", generator=g)
    body_h = body.cpu().numpy()
    offs, lens = torch.from_numpy(offs_h.view(np.int64)).cuda(), torch.from_numpy(lens_h.view(np.int32)).cuda()
    print("(b) n = 2^20 messages, lengths uniform in [0, 2368] back to back from byte 3 (%.3f GB; (a) has %.3f GB), us per call" % (
        total / 1e9, n * 1184 / 1e9))
    print("%10s | %14s | %10s" % ("alg", "sha3_ragged", "GB/s"), flush=True)
    for alg, _, outlen in ALGS:
        c = Call(torch, pkg, eng, alg, body, offs, lens, outlen=outlen)
        c()
        torch.cuda.synchronize()
        check_rows(np, alg, c, body_h, offs_h, lens_h, None, list(range(0, n, n // 64)) + [n - 1])
        (t,) = alternate(torch, [c], 5)
        print("%10s | %14.1f | %10.1f" % (alg, t, total / t / 1e3), flush=True)
    eng.close()


def sweep_shapes(np, torch, n):
    """(label, body tensor, offsets, lengths, head) of the two shapes of section (c)"""
    rng = np.random.default_rng(n)
    lens_h = rng.integers(0, 257, n).astype(np.uint32)
    offs_h = np.zeros(n, np.uint64)
    offs_h[1:] = np.cumsum(lens_h[:-1], dtype=np.uint64)
    g = torch.Generator(device="cuda").manual_seed(n)
    body = torch.randint(0, 256, (int(lens_h.sum()) + 1,), dtype=torch.uint8, device="cuda", generator=g)
    head = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    yield ("K + ctx", body, torch.from_numpy(offs_h.view(np.int64)).cuda(), torch.from_numpy(lens_h.view(np.int32)).cuda(), head)
    msgs = torch.randint(0, 256, (n * 1184,), dtype=torch.uint8, device="cuda", generator=g)
    yield ("1184 B", msgs, torch.arange(n, device="cuda", dtype=torch.int64) * 1184, torch.full((n,), 1184, device="cuda", dtype=torch.int32), None)


def section_c():
    np, torch, pkg = setup()
    lanes, waves = engine(pkg, 0), engine(pkg, 1 << 30)
    print("(c) form sweep, us per call: one sponge per lane (k_sha3_ragged) against one per wavefront (k_sha3_ragged_w), each forced")
    print("    shapes: K + ctx = 32-byte head + body uniform in [0, 256];  1184 B = equal 1184-byte messages")
    print("%7s | %10s %9s %9s | %10s %9s %9s | %10s %9s %9s | %10s %9s %9s" % (
        "n", "sha3_256", "K+ctx", "", "shake128", "K+ctx", "", "sha3_256", "1184 B", "", "shake128", "1184 B", ""))
    print("%7s | %10s %9s %9s | %10s %9s %9s | %10s %9s %9s | %10s %9s %9s" % (("",) + ("lane", "wave", "wave/lane") * 4), flush=True)
    for sh in range(6, 15):
        n = 1 << sh
        cells = {}
        for label, body, offs, lens, head in sweep_shapes(np, torch, n):
            for alg, _, outlen in ALGS:
                a = Call(torch, pkg, lanes, alg, body, offs, lens, head, outlen)
                b = Call(torch, pkg, waves, alg, body, offs, lens, head, outlen)
                a()
                b()
                torch.cuda.synchronize()
                assert torch.equal(a.out, b.out), (n, label, alg)
                cells[(label, alg)] = alternate(torch, [a, b], 20)
        row = []
        for label in ("K + ctx", "1184 B"):
            for alg, _, _ in ALGS:
                tl, tw = cells[(label, alg)]
                row += [tl, tw, tw / tl]
        print("%7d | %10.1f %9.1f %9.2f | %10.1f %9.1f %9.2f | %10.1f %9.1f %9.2f | %10.1f %9.1f %9.2f" % tuple([n] + row), flush=True)
    lanes.close()
    waves.close()


def section_d():
    np, torch, pkg = setup()
    lanes, waves = engine(pkg, 0), engine(pkg, 1 << 30)
    g = torch.Generator(device="cuda").manual_seed(4)
    body = torch.randint(0, 256, (100,), dtype=torch.uint8, device="cuda", generator=g)
    head = torch.randint(0, 256, (1, 32), dtype=torch.uint8, device="cuda", generator=g)
    offs, lens = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), 100, dtype=torch.int32, device="cuda")
    print("(d) one item (32-byte head + 100-byte body), us per call queued back to back (R = 200)")
    print("%10s | %10s %10s" % ("alg", "lane form", "wave form"), flush=True)
    for alg, _, outlen in ALGS:
        a, b = Call(torch, pkg, lanes, alg, body, offs, lens, head, outlen), Call(torch, pkg, waves, alg, body, offs, lens, head, outlen)
        a()
        b()
        torch.cuda.synchronize()
        assert torch.equal(a.out, b.out)
        check_rows(np, alg, b, body.cpu().numpy(), [0], [100], head.cpu().numpy(), [0])
        tl, tw = alternate(torch, [a, b], 200)
        print("%10s | %10.1f %10.1f" % (alg, tl, tw), flush=True)
    lanes.close()
    waves.close()


def driver(out_path):
    lines = ["tools/sha3_ragged_bench.py: mlkem_sha3_ragged_dev on one MI355X, HIP-event time per call", ""]
    failed = None
    for sec in "abcd":
        r = subprocess.run(["timeout", "-k", "10", str(SECTION_LIMIT[sec]), sys.executable, os.path.abspath(__file__), "--section", sec],
                           capture_output=True, text=True)
        lines += r.stdout.rstrip().splitlines() + [""]
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:      # a fault, an abort or a time limit: nothing more is started on the GPU
            failed = "section (%s) ended with exit status %d; stopped there\n%s" % (sec, r.returncode, r.stderr[-2000:])
            break
    if failed:
        lines.append(failed)
        print(failed, file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines).rstrip() + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=list("abcd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sha3_ragged.txt"))
    args = ap.parse_args()
    if args.section:
        {"a": section_a, "b": section_b, "c": section_c, "d": section_d}[args.section]()
    else:
        sys.exit(driver(args.out))
