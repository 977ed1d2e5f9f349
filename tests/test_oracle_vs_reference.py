"""CPU tier: the oracle against the reference build (oracle/_ref/libmlkem_ref.so), on seeded inputs.  Where that build is
absent (a clean checkout carries no reference sources) the reference's answers come from tests/golden/ref_calls.npz, which
recorded these very calls (oracle/ref_replay.py).
Also covers BASELINE config[0]: ML-KEM-512 single KeyGen+Encaps+Decaps on the CPU via ml_kem.c."""
import numpy as np
import pytest

from conftest import seeds
from oracle.loader import SIZES


def test_config0_mlkem512_public_api_roundtrip(ref):
    """configs[0]: the reference's own public API (random seeds from /dev/urandom): shared secrets agree."""
    rc, ek, dk = ref.kem_keygen_public(512)
    assert rc == 0
    rc, c, K = ref.kem_encaps_public(512, ek)
    assert rc == 0
    rc, K2 = ref.kem_decaps(512, dk, c)
    assert rc == 0 and (K == K2).all()


def test_config0_oracle_agrees_on_reference_generated_keys(ref, oracle):
    rc, ek, dk = ref.kem_keygen_public(512)
    rc, c, K = ref.kem_encaps_public(512, ek)
    Ko, st = oracle.decaps(512, dk, c)
    assert st[0] == 0 and (Ko[0] == K).all()


@pytest.mark.parametrize("pset", (512, 768, 1024))
def test_kem_oracle_equals_reference(ref, oracle, pset):
    n = 3
    d, z, m = seeds("cpu-d", n, pset), seeds("cpu-z", n, pset), seeds("cpu-m", n, pset)
    ek, dk = oracle.keygen(pset, d, z)
    ek2, dk2 = ref.keygen(pset, d, z)
    assert (ek == ek2).all() and (dk == dk2).all()
    c, K = oracle.encaps(pset, ek, m)
    c2, K2 = ref.encaps(pset, ek, m)
    assert (c == c2).all() and (K == K2).all()
    cb = c.copy()
    cb[1, SIZES[pset][2] - 1] ^= 0x80  # tamper inside c2 -> implicit rejection for item 1
    Kd, st = oracle.decaps(pset, dk, cb)
    Kd2, st2 = ref.decaps(pset, dk, cb)
    assert (Kd == Kd2).all() and (st == st2).all()
    assert (Kd[0] == K[0]).all() and not (Kd[1] == K[1]).all()


def test_primitives_oracle_equals_reference(ref, oracle):
    rng = np.random.default_rng(7)
    for _ in range(8):
        f = rng.integers(0, 3329, 256).astype(np.uint16)
        g = rng.integers(0, 4096, 256).astype(np.uint16)
        assert (oracle.ntt(f) == ref.ntt(f)).all() and (oracle.intt(f) == ref.intt(f)).all()
        assert (oracle.ntt(g) == ref.ntt(g)).all() and (oracle.intt(g) == ref.intt(g)).all()
        assert (oracle.multiply_ntts(f, g) == ref.multiply_ntts(f, g)).all()
        B = rng.integers(0, 256, 34).astype(np.uint8)
        assert (oracle.sample_ntt(B) == ref.sample_ntt(B)).all()
    for n in (0, 5, 135, 136, 168, 169, 1184):
        x = rng.integers(0, 256, n).astype(np.uint8)
        assert (oracle.H(x) == ref.H(x)).all() and (oracle.G(x) == ref.G(x)).all() and (oracle.J(x) == ref.J(x)).all()


def test_reference_sha3_bit_api_matches_oracle_bits(ref, oracle):
    rng = np.random.default_rng(9)
    for nbits in (0, 1, 5, 30, 1086, 1087, 1088, 1341, 1343, 1344, 1605):
        bits = rng.integers(0, 2, nbits).astype(np.uint8)
        for rate, xof, dbits in ((136, False, 256), (168, True, 1024), (72, False, 512)):
            cap = 1600 - 8 * rate
            if (nbits + (4 if xof else 2) + 2) % (8 * rate) == 0:
                continue  # the reference's latent pad bug; the oracle follows FIPS 202 there
            want = np.packbits(ref.sha3_bits(bits, dbits, cap, xof), bitorder="little")
            assert (oracle.sponge_bits(rate, xof, bits, dbits // 8) == want).all(), (nbits, rate)


def test_compress_decompress_whole_12bit_field_every_d(ref, oracle, golden_npz):
    """Test_Archive/CompressDecompress_test04.c sweeps d = 1..12; here every 12-bit input (values >= q and >= 2^d
    included: the reference's field arithmetic wraps at 12 bits): oracle == live reference == committed tables."""
    gc, gd = np.asarray(golden_npz["g4_compress_full"]), np.asarray(golden_npz["g4_decompress_full"])
    oc, od, rc, rd = oracle.lib.orc_compress, oracle.lib.orc_decompress, ref.compress, ref.decompress
    for d in range(1, 13):
        o_c = np.fromiter((oc(v, d) for v in range(4096)), np.int64, 4096)
        o_d = np.fromiter((od(v, d) for v in range(4096)), np.int64, 4096)
        r_c = np.fromiter((rc(v, d) for v in range(4096)), np.int64, 4096)
        r_d = np.fromiter((rd(v, d) for v in range(4096)), np.int64, 4096)
        assert (o_c == r_c).all() and (o_c == gc[d - 1]).all(), (d, np.nonzero(o_c != r_c)[0][:4])
        assert (o_d == r_d).all() and (o_d == gd[d - 1]).all(), (d, np.nonzero(o_d != r_d)[0][:4])
        ys = np.arange(1 << min(d, 11))
        assert (o_c[o_d[ys]] == ys).all()   # test04's property: Compress(Decompress(y)) == y


def test_sha3_b_appends_the_callers_suffix_verbatim(ref, oracle, golden):
    """sha3.c:414-429: sfx[2] picks the suffix LENGTH, the bits themselves are the caller's (RawSHAKE "11", ...)."""
    for g in golden["G9_sha3_suffix"]:
        bits = np.array([int(ch) for ch in g["msg_bits"]], np.uint8)
        sfx = np.array(g["sfx"], np.uint8)
        nsfx = 4 if sfx[2] == 1 else 2
        want = np.frombuffer(bytes.fromhex(g["out"]), np.uint8)
        got_ref = np.packbits(ref.sha3_bits_sfx(bits, 8 * want.size, g["cap"], sfx), bitorder="little")
        assert (got_ref == want).all()
        assert (oracle.sponge_bits_sfx(g["rate_bytes"], sfx[:nsfx], bits, want.size) == want).all(), g["sfx"]


def test_inverse_ntt_above_q_is_undefined_in_the_reference(ref, ref_o0, oracle):
    """Why mlkem_intt's contract is [0, q): for inputs >= q the reference's InverseNTT (ml_kem.c:364-367) computes
    Q - (t - f[j+len]) in a 24-bit field and multiplies it by zeta in a (promoted, signed) int, which overflows: the
    reference built with its own makefile flags (-O0) and the -O2 build return DIFFERENT polynomials.  There is nothing
    to be bit-exact against; the forward NTT has no such overflow and both builds (and the oracle) agree on every
    12-bit input, including those whose outputs stay >= q."""
    r2, r0 = ref, ref_o0
    rng = np.random.default_rng(1)
    differ = 0
    for _ in range(20):
        f = rng.integers(0, 4096, 256).astype(np.uint16)
        f[0::4] = rng.integers(3900, 4096, 64)      # a - b > q at (j, j + 2): the wrap of ml_kem.c:365
        f[2::4] = rng.integers(0, 50, 64)
        differ += int((np.asarray(r2.intt(f)) != np.asarray(r0.intt(f))).any())
        g = rng.integers(0, 4096, 256).astype(np.uint16)
        assert (np.asarray(r2.ntt(g)) == np.asarray(r0.ntt(g))).all() and (oracle.ntt(g).ravel() == np.asarray(r2.ntt(g)).ravel()).all()
        canon = (f % 3329).astype(np.uint16)        # inside the contract everything agrees
        assert (np.asarray(r2.intt(canon)) == np.asarray(r0.intt(canon))).all()
        assert (oracle.intt(canon).ravel() == np.asarray(r2.intt(canon)).ravel()).all()
    assert differ == 20
    one = np.zeros(256, np.uint16)
    one[0] = 4095
    assert np.asarray(r2.ntt(one)).ravel()[254] == 4095 == np.asarray(r0.ntt(one)).ravel()[254] == oracle.ntt(one).ravel()[254]


def test_poly_add_sub_raw_12bit_inputs_oracle_equals_reference(ref, oracle):
    """PolyAddition / PolySubtraction (ml_kem.c:580-613) on every kind of 12-bit input, also above q where the subtraction's
    `Q - (v - u)` wraps in the reference's 12-bit field: oracle == live reference."""
    rng = np.random.default_rng(580)
    a = rng.integers(0, 4096, (8, 256)).astype(np.uint16)
    b = rng.integers(0, 4096, (8, 256)).astype(np.uint16)
    a[0], b[0] = 0, 4095
    a[1], b[1] = 4095, 4095
    a[2], b[2] = 4095, 0
    for i in range(8):
        assert (oracle.poly_add(a[i], b[i]) == ref.poly_add(a[i], b[i])).all()
        assert (oracle.poly_sub(a[i], b[i]) == ref.poly_sub(a[i], b[i])).all()


def test_sponge_at_any_byte_aligned_capacity(ref, oracle):
    """The reference's Sponge takes ANY capacity (sha3.c:257-317; sha3_b's `c`), not only the four SHA-3 / two SHAKE ones.  The
    oracle's bit-granular sponge at odd byte rates (capacity = 1600 - 8 * rate bits) equals the live reference for empty, short,
    rate-straddling and multi-block messages and outputs longer than one block -- the pin for the engine's one-sponge-per-wave
    kernel k_sponge_raw_w, which serves every rate of 1..199 bytes (tests/test_emulated_kernels.py, tests/test_gpu_round3.py)."""
    rng = np.random.default_rng(31)
    for rate in (1, 8, 13, 40, 100, 137, 168, 199):
        for nbits in (0, 5, 8 * rate - 4, 8 * rate + 3, 1700):
            for sfx in ((0, 1, 0, 0), (1, 1, 1, 1)):
                nsfx = 4 if sfx[2] == 1 else 2
                if (nbits + nsfx + 2) % (8 * rate) == 0:
                    continue   # the reference's latent pad() bug (message + suffix = -2 mod r), deliberately not reproduced
                bits = rng.integers(0, 2, nbits).astype(np.uint8)
                outlen = max(4, (5 * rate) // 2)
                want = np.packbits(ref.sha3_bits_sfx(bits, 8 * outlen, 1600 - 8 * rate, np.array(sfx, np.uint8)), bitorder="little")
                got = oracle.sponge_bits_sfx(rate, np.array(sfx[:nsfx], np.uint8), bits, outlen)
                assert (got == want).all(), (rate, nbits, sfx)
