"""The reference's answers for the CPU tier, live or recorded — test infrastructure only.

tests/test_oracle_vs_reference.py compares the oracle with the real reference (oracle/_ref).  That build needs the
reference sources, which a clean checkout does not carry, so every call those tests make of the reference is recorded
once, with its arguments hashed, into tests/golden/ref_calls.npz.  `open_ref()` hands the tests the live build when it
exists and otherwise a `Replay` that answers the same calls from the recording; a call that was never recorded is an
error, not a skip.  Compress / Decompress are answered from the full tables of tests/golden/mlkem_golden.npz
(g4_compress_full / g4_decompress_full, generated from the same -O2 build by oracle/gen_golden.py).

Regenerate the recording where the reference build exists:
    MLKEM_REF_RECORD=1 python -m pytest tests/test_oracle_vs_reference.py
"""
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = os.path.join(ROOT, "tests", "golden", "ref_calls.npz")
TABLES = os.path.join(ROOT, "tests", "golden", "mlkem_golden.npz")
RECORD = os.environ.get("MLKEM_REF_RECORD") == "1"
FROM_TABLES = ("compress", "decompress")   # answered from the committed tables, not recorded call by call


def call_key(build, method, args):
    """sha256 over the build label, the method and every argument (arrays by dtype, shape and bytes)."""
    h = hashlib.sha256(("%s:%s" % (build, method)).encode())
    for a in args:
        if isinstance(a, (np.ndarray, list, tuple, bytes, bytearray)):
            a = np.ascontiguousarray(np.frombuffer(bytes(a), np.uint8) if isinstance(a, (bytes, bytearray)) else a)
            h.update(("|%s%s|" % (a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
        else:
            h.update(("|%d|" % int(a)).encode())
    return h.hexdigest()[:32]


def _label(o0):
    return "O0" if o0 else "O2"


class Recorder:
    """Forwards to the live build and keeps the first answer to every distinct call."""

    def __init__(self, ref, o0, store):
        self._ref, self._build, self._store = ref, _label(o0), store

    def __getattr__(self, name):
        fn = getattr(self._ref, name)
        if name in FROM_TABLES:
            return fn

        def call(*args):
            out = fn(*args)
            self._store.setdefault(call_key(self._build, name, args), out)
            return out
        return call


class Replay:
    """Answers recorded calls of one build (O2 or O0) from tests/golden/ref_calls.npz."""

    def __init__(self, o0=False):
        self._build = _label(o0)
        self._calls = load(CALLS)
        t = np.load(TABLES, allow_pickle=False)
        self._compress, self._decompress = np.asarray(t["g4_compress_full"]), np.asarray(t["g4_decompress_full"])

    def compress(self, x, d):
        assert self._build == "O2", "the committed Compress table is the -O2 build's"
        return int(self._compress[int(d) - 1][int(x)])

    def decompress(self, y, d):
        assert self._build == "O2", "the committed Decompress table is the -O2 build's"
        return int(self._decompress[int(d) - 1][int(y)])

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args):
            k = call_key(self._build, name, args)
            if k not in self._calls:
                raise KeyError("no recorded reference answer for %s.%s with these arguments: regenerate %s (see oracle/ref_replay.py)"
                               % (self._build, name, os.path.relpath(CALLS, ROOT)))
            return self._calls[k]
        return call


def save(store, path=CALLS):
    """One npz entry per answer: `<key>` for a single value, `<key>.<i>` for the members of a tuple."""
    flat = {}
    for k, out in store.items():
        if isinstance(out, tuple):
            for i, v in enumerate(out):
                flat["%s.%d" % (k, i)] = np.asarray(v)
        else:
            flat[k] = np.asarray(out)
    np.savez_compressed(path, **flat)


def _plain(a):
    return a.item() if a.ndim == 0 else a


def load(path=CALLS):
    z = np.load(path, allow_pickle=False)
    out, parts = {}, {}
    for name in z.files:
        k, _, i = name.partition(".")
        if i:
            parts.setdefault(k, {})[int(i)] = _plain(z[name])
        else:
            out[k] = _plain(z[name])
    for k, p in parts.items():
        out[k] = tuple(p[i] for i in range(len(p)))
    return out


def open_ref(o0=False, store=None):
    """The live reference build when it exists (wrapped in a Recorder when MLKEM_REF_RECORD=1), else its recording."""
    from oracle.loader import Ref
    if Ref.available(o0):
        ref = Ref(o0)
        return Recorder(ref, o0, store) if RECORD else ref
    if RECORD:
        raise RuntimeError("MLKEM_REF_RECORD=1 needs the reference build oracle/_ref")
    return Replay(o0)
