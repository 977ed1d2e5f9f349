"""Cases of batched key validation (mlkem_check_keys): valid key pairs with one corruption class per item, and the expected
status words computed independently of the engine -- the modulus bits from a numpy ByteDecode_12, the hash bit from hashlib's
SHA3-256, the mismatch bit from a byte comparison, the seed bit from the oracle's KeyGen and the PCT bit from the oracle's
Encaps followed by its Decaps_internal, all in the conformance mode of the context under test."""
import hashlib

import numpy as np

from conftest import seeds
from oracle.loader import SIZES

EK_MODULUS, DK_MODULUS, DK_HASH, EK_MISMATCH, SEED, PCT = 1, 2, 4, 8, 16, 32
Q = 3329

# optional-argument combinations: which of ek, dk, seed, m a call passes
COMBOS = {
    "ek": ("ek",),
    "dk": ("dk",),
    "ek+dk": ("ek", "dk"),
    "ek+dk+seed": ("ek", "dk", "seed"),
    "ek+dk+m": ("ek", "dk", "m"),
    "dk+m": ("dk", "m"),
    "all": ("ek", "dk", "seed", "m"),
}
# corruption classes, item i gets CLASSES[i % len(CLASSES)]
CLASSES = ("valid", "ek_q", "ek_4095", "dkek_q", "dk_h", "dk_z", "dk_pke", "ek_rho", "swap")


def k_of(pset):
    return (SIZES[pset][0] - 32) // 384


def set_coeff(row, off, idx, value):
    """ByteEncode_12 coefficient `idx` of the polynomial vector starting at byte `off` of `row` to `value` (12 bits)"""
    b = off + 3 * (idx // 2)
    if idx % 2 == 0:
        row[b] = value & 0xFF
        row[b + 1] = (row[b + 1] & 0xF0) | (value >> 8)
    else:
        row[b + 1] = (row[b + 1] & 0x0F) | ((value & 0xF) << 4)
        row[b + 2] = value >> 4


def corrupt(pset, ek, dk, n):
    """apply class i % 9 to item i of (ek, dk) in place (the valid pairs come from the same seeds); returns the class names"""
    k = k_of(pset)
    cls = [CLASSES[i % len(CLASSES)] for i in range(n)]
    last = 256 * (k - 1)   # first coefficient of the last polynomial
    swaps = []
    for i, c in enumerate(cls):
        if c == "ek_q":
            set_coeff(ek[i], 0, last + (0 if i % 2 == 0 else 255), Q)
        elif c == "ek_4095":
            set_coeff(ek[i], 0, last + (255 if i % 2 == 0 else 0), 4095)
        elif c == "dkek_q":
            set_coeff(dk[i], 384 * k, last + (i % 256), Q + (i % (4096 - Q)))
        elif c == "dk_h":
            dk[i, 768 * k + 32 + i % 32] ^= 1 << (i % 8)
        elif c == "dk_z":
            dk[i, 768 * k + 64 + (11 * i) % 32] ^= 1 << (i % 8)   # item 5: byte 23, item 32: byte 0 -- both halves
        elif c == "dk_pke":
            dk[i, (37 * i) % (384 * k)] ^= 1 << (i % 8)
        elif c == "ek_rho":
            ek[i, 384 * k + i % 32] ^= 1 << (i % 8)
        elif c == "swap":
            swaps.append(i)
    # the "swap" items exchange their dks pairwise (a lone last one swaps with the valid item 0 ... of its own, so it is kept valid)
    for a, b in zip(swaps[0::2], swaps[1::2]):
        dk[[a, b]] = dk[[b, a]]
    if len(swaps) % 2:
        cls[swaps[-1]] = "valid"
    return cls


def make_batch(oracle, pset, fips, n, label):
    """n valid key pairs from the oracle's KeyGen (in the given mode), corrupted by class; seed = d || z, m random"""
    oracle.set_conformance(bool(fips))
    d, z, m = seeds(label + "-d", n, pset), seeds(label + "-z", n, pset), seeds(label + "-m", n, pset)
    ek, dk = oracle.keygen(pset, d, z)
    cls = corrupt(pset, ek, dk, n)
    seed = np.ascontiguousarray(np.concatenate([d, z], axis=1))
    return dict(ek=ek, dk=dk, seed=seed, m=m), cls


def byte_decode12_over_q(rows):
    """per row: does any ByteDecode_12 coefficient of the bytes reach q"""
    b = rows.reshape(rows.shape[0], -1, 3).astype(np.uint16)
    c0 = b[:, :, 0] | ((b[:, :, 1] & 0xF) << 8)
    c1 = (b[:, :, 1] >> 4) | (b[:, :, 2] << 4)
    return (c0 >= Q).any(axis=1) | (c1 >= Q).any(axis=1)


def expected(oracle, pset, fips, given, idx=None):
    """status words of the items `idx` (all by default) for the inputs in `given` (dict name -> array or None)"""
    k = k_of(pset)
    ek, dk, seed, m = (given.get(x) for x in ("ek", "dk", "seed", "m"))
    n = (ek if ek is not None else dk).shape[0]
    idx = np.arange(n) if idx is None else np.asarray(idx)
    sel = lambda a: None if a is None else np.ascontiguousarray(a[idx])
    ek, dk, seed, m = sel(ek), sel(dk), sel(seed), sel(m)
    st = np.zeros(len(idx), np.int32)
    if ek is not None:
        st |= np.where(byte_decode12_over_q(ek[:, :384 * k]), EK_MODULUS, 0).astype(np.int32)
    if dk is not None:
        dkek = dk[:, 384 * k:768 * k + 32]
        st |= np.where(byte_decode12_over_q(dkek[:, :384 * k]), DK_MODULUS, 0).astype(np.int32)
        for j in range(len(idx)):
            if hashlib.sha3_256(dkek[j].tobytes()).digest() != dk[j, 768 * k + 32:768 * k + 64].tobytes():
                st[j] |= DK_HASH
    if ek is not None and dk is not None:
        st |= np.where((ek != dk[:, 384 * k:768 * k + 32]).any(axis=1), EK_MISMATCH, 0).astype(np.int32)
    oracle.set_conformance(bool(fips))
    if seed is not None:
        ek_s, dk_s = oracle.keygen(pset, seed[:, :32].copy(), seed[:, 32:].copy())
        bad = np.zeros(len(idx), bool)
        if ek is not None:
            bad |= (ek != ek_s).any(axis=1)
        if dk is not None:
            bad |= (dk != dk_s).any(axis=1)
        st |= np.where(bad, SEED, 0).astype(np.int32)
    if m is not None:
        ekp = ek if ek is not None else np.ascontiguousarray(dk[:, 384 * k:768 * k + 32])
        c, K = oracle.encaps(pset, ekp, m)
        for j in range(len(idx)):
            if (oracle.decaps_internal(pset, dk[j], c[j]) != K[j]).any():
                st[j] |= PCT
    return st


def target(cls, names):
    """the bit a corruption class must set for a call passing `names` (0: the class's input is absent or not checked)"""
    ek, dk, seed, m = ("ek" in names), ("dk" in names), ("seed" in names), ("m" in names)
    return {
        "valid": 0,
        "ek_q": EK_MODULUS if ek else 0,
        "ek_4095": EK_MODULUS if ek else 0,
        "dkek_q": DK_MODULUS if dk else 0,
        "dk_h": DK_HASH if dk else 0,
        "dk_z": SEED if (dk and seed) else 0,
        "dk_pke": SEED if (dk and seed) else (PCT if m else 0),
        "ek_rho": EK_MISMATCH if (ek and dk) else 0,
        "swap": EK_MISMATCH if (ek and dk) else 0,   # dk + m alone: the PCT to the swapped dk's own ek passes
    }[cls]


def check_against(got, exp, cls, names):
    """got == expected word for word; every class sets its target bit; valid items are 0; dk_z sets SEED alone"""
    assert got.shape == exp.shape
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, "items %s: got %s expected %s (classes %s)" % (
        bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist(), [cls[i] for i in bad[:8]])
    for i, c in enumerate(cls):
        t = target(c, names)
        assert exp[i] & t == t, (i, c, exp[i])
        if c == "valid":
            assert exp[i] == 0
        if c == "dk_z":
            assert exp[i] == (SEED if ("dk" in names and "seed" in names) else 0)
