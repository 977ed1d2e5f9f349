"""pytest configuration: `gpu` marker + shared fixtures.

CPU tier  (-m "not gpu"): oracle vs golden vectors / live reference, host logic, C-ABI exports.
GPU tier  (-m gpu)      : parity of the HIP path (through the C-ABI) against the oracle + golden.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def expand_seed(label: str, index: int, seed: int) -> bytes:
    """SHAKE128(label || LE64(index) || LE64(seed))[:32] — same expander as oracle/gen_golden.py."""
    return hashlib.shake_128(label.encode() + index.to_bytes(8, "little") + seed.to_bytes(8, "little")).digest(32)


def seeds(label, n, seed):
    return np.frombuffer(b"".join(expand_seed(label, i, seed) for i in range(n)), np.uint8).reshape(n, 32).copy()


@pytest.fixture(scope="session")
def golden():
    with open(os.path.join(GOLDEN_DIR, "mlkem_golden.json")) as f:
        return json.load(f)


@pytest.fixture(scope="session")
def golden_npz():
    return np.load(os.path.join(GOLDEN_DIR, "mlkem_golden.npz"), allow_pickle=False)


@pytest.fixture(scope="session")
def oracle():
    from oracle.loader import Oracle, build
    build()
    return Oracle()


@pytest.fixture(scope="session")
def _ref_store():
    """Answers of the live reference collected under MLKEM_REF_RECORD=1; written to tests/golden/ref_calls.npz at the end."""
    from oracle import ref_replay
    store = {}
    yield store
    if ref_replay.RECORD and store:
        ref_replay.save(store)


@pytest.fixture(scope="session")
def ref(_ref_store):
    """The real reference build (oracle/_ref, -O2) when it exists, otherwise its recorded answers
    (tests/golden/ref_calls.npz, oracle/ref_replay.py)."""
    from oracle.ref_replay import open_ref
    return open_ref(o0=False, store=_ref_store)


@pytest.fixture(scope="session")
def ref_o0(_ref_store):
    """The reference built at its makefile's own flags (-O0), live or recorded like `ref`."""
    from oracle.ref_replay import open_ref
    return open_ref(o0=True, store=_ref_store)


def unhex(s):
    return np.frombuffer(bytes.fromhex(s), np.uint8).copy()


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
