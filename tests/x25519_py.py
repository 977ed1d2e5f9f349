"""An independent restatement of X25519 (RFC 7748 section 5) with Python integers, and of the X-Wing hybrid KEM composed from it,
hashlib and tests/fips203_py.py -- test infrastructure only; it shares no code with the engine.

    expand(sk):  e = SHAKE256(sk, 96); d, z, sk_X = e[0:32], e[32:64], e[64:96]
    KeyGen(sk) -> pk = pk_M || X25519(sk_X, 9);  Encaps(pk, eseed) -> ct = ct_M || X25519(ek_X, 9), ek_X = eseed[32:64]
    ss = SHA3-256(ss_M || ss_X || ct_X || pk_X || 5c2e2f2f5e5c);  ML-KEM-768 is always FIPS 203
check_pinned() asserts two RFC 7748 vectors (section 5.2's first vector and the first iteration of its iterated test).  The X-Wing
draft's own test vectors are not available here and have not been run."""
import hashlib

import fips203_py as F

P = (1 << 255) - 19
A24 = 121665
LABEL = bytes.fromhex("5c2e2f2f5e5c")
BASE = (9).to_bytes(32, "little")
SK_BYTES, PK_BYTES, CT_BYTES, SS_BYTES, ESEED_BYTES = 32, 1216, 1120, 32, 64
LOW_ORDER_U = (0, 1, P - 1, P, P + 1)   # all give the all-zero output under a clamped scalar


def clamp(k):
    k = bytearray(k)
    k[0] &= 248
    k[31] &= 127
    k[31] |= 64
    return int.from_bytes(k, "little")


def x25519(k, u):
    """k, u: 32 bytes each -> 32 bytes.  Bit 255 of u is ignored and u is taken mod p; the output is canonical."""
    k = clamp(bytes(k))
    x1 = (int.from_bytes(bytes(u), "little") & ((1 << 255) - 1)) % P
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        kt = (k >> t) & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b = (x2 + z2) % P, (x2 - z2) % P
        aa, bb = a * a % P, b * b % P
        e = (aa - bb) % P
        c, d = (x3 + z3) % P, (x3 - z3) % P
        da, cb = d * a % P, c * b % P
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, z2 = x3, z3
    return (x2 * pow(z2, P - 2, P) % P).to_bytes(32, "little")


def check_pinned():
    h = bytes.fromhex
    assert x25519(h("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4"),
                  h("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c")) == \
        h("c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552")
    assert x25519(BASE, BASE) == h("422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079")


def fe_encode(v):
    """canonical encoding of the 255-bit input v"""
    return (v % P).to_bytes(32, "little")


def xwing_expand(sk):
    e = hashlib.shake_256(bytes(sk)).digest(96)
    return e[:32], e[32:64], e[64:]


def combiner(ss_m, ss_x, ct_x, pk_x):
    return hashlib.sha3_256(bytes(ss_m) + bytes(ss_x) + bytes(ct_x) + bytes(pk_x) + LABEL).digest()


def xwing_keygen(sk):
    d, z, sk_x = xwing_expand(sk)
    pk_m, _ = F.keygen(768, d, z)
    return bytes(pk_m) + x25519(sk_x, BASE)


def xwing_encaps(pk, eseed):
    pk, eseed = bytes(pk), bytes(eseed)
    ct_m, ss_m = F.encaps(768, pk[:1184], eseed[:32])
    ek_x, pk_x = eseed[32:], pk[1184:]
    ct_x, ss_x = x25519(ek_x, BASE), x25519(ek_x, pk_x)
    return bytes(ct_m) + ct_x, combiner(ss_m, ss_x, ct_x, pk_x)


def xwing_decaps(sk, ct):
    ct = bytes(ct)
    d, z, sk_x = xwing_expand(sk)
    _, dk_m = F.keygen(768, d, z)
    ss_m = F.decaps(768, dk_m, ct[:1088])
    ct_x = ct[1088:]
    return combiner(ss_m, x25519(sk_x, ct_x), ct_x, x25519(sk_x, BASE))
