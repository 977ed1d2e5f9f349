#!/usr/bin/env python3
"""tools/reject_sweep.py -- what a rejected ciphertext costs: device time of mlkem_decaps_dev alone (ML-KEM-768, 2^20 items by
default, device-resident) with a fraction 0, 1/1024, 1/16 and 1 of the ciphertexts tampered.  The batch path computes J(z || c) for the
rejected items only (k_hash_j_rejected), so the call's duration grows with that fraction; a build that hashes J for every item is flat.

  tools/reject_sweep.py [--items N] [--calls 10] [--label NAME]

The library is the one MLKEM_LIB_PATH names (default: the tree's build); run it once per build ON THE SAME BOX and compare the lines.
Time per call = HIP events around `--calls` calls queued back to back, median of 5 such runs.  Every fraction is checked: the keys of
untouched items equal Encaps' K, those of tampered items do not."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

FRACTIONS = (("0", 0), ("1/1024", 1024), ("1/16", 16), ("1", 1))
RUNS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--label", default=os.environ.get("MLKEM_LIB_PATH", "tree"))
    a = ap.parse_args()
    pkg = ge.load_package()
    n, pset = a.items, 768
    e = pkg.MLKEM(pset, device=0)
    g = torch.Generator(device="cuda").manual_seed(pset)
    d, z, m = (torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g) for _ in range(3))
    ek, dk = e.keygen(d, z)
    c, K_enc = e.encaps(ek, m)
    K, st = torch.empty_like(K_enc), torch.empty(n, dtype=torch.int32, device="cuda")
    base = None
    for name, every in FRACTIONS:
        ct = c.clone()
        rej = torch.zeros(n, dtype=torch.bool, device="cuda")
        if every:
            rej[::every] = True
            ct[::every, 5] ^= 1
        for _ in range(2):
            e.decaps(dk, ct, K=K, status=st)
        torch.cuda.synchronize()
        ts = []
        for _ in range(RUNS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                e.decaps(dk, ct, K=K, status=st)
            t1.record()
            torch.cuda.synchronize()
            ts.append(t0.elapsed_time(t1) / a.calls)
        same = (K == K_enc).all(dim=1)
        assert bool((same == ~rej).all()) and int(st.abs().max()) == 0, "results do not match the tamper pattern"
        med = statistics.median(ts)
        base = base or med
        print("%s ML-KEM-%d decaps n=%d rejected %-6s : %.3f ms per call [%.3f..%.3f]  x%.3f of the fraction-0 call"
              % (a.label, pset, n, name, med, min(ts), max(ts), med / base), flush=True)
    e.close()


if __name__ == "__main__":
    main()
