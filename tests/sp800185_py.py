"""An independent restatement of SP 800-185 in plain Python: Keccak-f[1600], the sponge, left_encode / right_encode / encode_string /
bytepad, cSHAKE128 / 256, KMAC128 / 256 and KMACXOF128 / 256.  It shares no code with the engine; the tests that use it as the
expected value first pin it against hashlib (SHAKE, SHA3-256 through the same sponge) and the NIST sample values (SAMPLES)."""

MASK = (1 << 64) - 1
RC = []
RHO = [[0] * 5 for _ in range(5)]


def _init():
    r = 1
    for _ in range(24):
        c = 0
        for j in range(7):
            r = ((r << 1) ^ ((r >> 7) * 0x71)) & 0xFF
            if r & 2:
                c ^= 1 << ((1 << j) - 1)
        RC.append(c)
    x, y = 1, 0
    for t in range(24):
        RHO[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5


_init()


def rol(v, n):
    n %= 64
    return ((v << n) | (v >> (64 - n))) & MASK if n else v


def keccak_f(A):
    """A[x][y], 25 lanes of 64 bits, in place"""
    for rnd in range(24):
        C = [A[x][0] ^ A[x][1] ^ A[x][2] ^ A[x][3] ^ A[x][4] for x in range(5)]
        D = [C[(x - 1) % 5] ^ rol(C[(x + 1) % 5], 1) for x in range(5)]
        for x in range(5):
            for y in range(5):
                A[x][y] ^= D[x]
        B = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                B[y][(2 * x + 3 * y) % 5] = rol(A[x][y], RHO[x][y])
        for x in range(5):
            for y in range(5):
                A[x][y] = B[x][y] ^ (~B[(x + 1) % 5][y] & MASK & B[(x + 2) % 5][y])
        A[0][0] ^= RC[rnd]


def sponge(rate, msg, suffix, outlen):
    """Keccak[1600 - 8 rate](msg || suffix bits, outlen bytes); suffix is the domain byte that also carries the first padding bit"""
    p = bytearray(msg)
    p.append(suffix)
    p.extend(bytes(-len(p) % rate))
    p[-1] ^= 0x80
    A = [[0] * 5 for _ in range(5)]
    for off in range(0, len(p), rate):
        for i in range(rate // 8):
            A[i % 5][i // 5] ^= int.from_bytes(p[off + 8 * i:off + 8 * i + 8], "little")
        keccak_f(A)
    out = bytearray()
    while True:
        for i in range(rate // 8):
            out += A[i % 5][i // 5].to_bytes(8, "little")
        if len(out) >= outlen:
            return bytes(out[:outlen])
        keccak_f(A)


def left_encode(x):
    b = x.to_bytes(max(1, (x.bit_length() + 7) // 8), "big")
    return bytes([len(b)]) + b


def right_encode(x):
    b = x.to_bytes(max(1, (x.bit_length() + 7) // 8), "big")
    return b + bytes([len(b)])


def encode_string(s):
    return left_encode(8 * len(s)) + bytes(s)


def bytepad(x, w):
    z = left_encode(w) + bytes(x)
    return z + bytes(-len(z) % w)


def rate_of(bits):
    return {128: 168, 256: 136}[bits]


def cshake(bits, X, outlen, N=b"", S=b""):
    """cSHAKE128 / 256 (X, L = 8 outlen, N, S)"""
    if not N and not S:
        return sponge(rate_of(bits), X, 0x1F, outlen)
    return sponge(rate_of(bits), bytepad(encode_string(N) + encode_string(S), rate_of(bits)) + bytes(X), 0x04, outlen)


def kmac(bits, K, X, outlen, S=b"", xof=False):
    """KMAC128 / 256 (K, X, L = 8 outlen, S), or KMACXOF128 / 256 with xof"""
    newX = bytepad(encode_string(K), rate_of(bits)) + bytes(X) + right_encode(0 if xof else 8 * outlen)
    return cshake(bits, newX, outlen, b"KMAC", S)


def kdf_onestep(bits, Z, fixed_info, outlen, salt=None):
    """SP 800-56C r2 section 4.1 option 3 with H_outputBits = L (one repetition): KMAC#(salt, 00000001 || Z || FixedInfo, L, "KDF")"""
    if salt is None:
        salt = bytes(164 if bits == 128 else 132)
    return kmac(bits, salt, b"\x00\x00\x00\x01" + bytes(Z) + bytes(fixed_info), outlen, b"KDF")


K_SAMPLE = bytes(range(0x40, 0x60))
X4 = bytes(range(4))
X200 = bytes(range(200))
# (function, arguments, expected hex): the sample values of NIST's cSHAKE_samples.pdf and KMAC_samples.pdf / KMACXOF_samples.pdf
SAMPLES = (
    (cshake, (128, X4, 32, b"", b"Email Signature"), "C1C36925B6409A04F1B504FCBCA9D82B4017277CB5ED2B2065FC1D3814D5AAF5"),
    (cshake, (128, X200, 32, b"", b"Email Signature"), "C5221D50E4F822D96A2E8881A961420F294B7B24FE3D2094BAED2C6524CC166B"),
    (cshake, (256, X4, 64, b"", b"Email Signature"),
     "D008828E2B80AC9D2218FFEE1D070C48B8E4C87BFF32C9699D5B6896EEE0EDD164020E2BE0560858D9C00C037E34A96937C561A74C412BB4C746469527281C8C"),
    (kmac, (128, K_SAMPLE, X4, 32, b""), "E5780B0D3EA6F7D3A429C5706AA43A00FADBD7D49628839E3187243F456EE14E"),
    (kmac, (128, K_SAMPLE, X4, 32, b"My Tagged Application"), "3B1FBA963CD8B0B59E8C1A6D71888B7143651AF8BA0A7070C0979E2811324AA5"),
    (kmac, (128, K_SAMPLE, X200, 32, b"My Tagged Application"), "1F5B4E6CCA02209E0DCB5CA635B89A15E271ECC760071DFD805FAA38F9729230"),
    (kmac, (256, K_SAMPLE, X4, 64, b"My Tagged Application"),
     "20C570C31346F703C9AC36C61C03CB64C3970D0CFC787E9B79599D273A68D2F7F69D4CC3DE9D104A351689F27CF6F5951F0103F33F4F24871024D9C27773A8DD"),
    (kmac, (256, K_SAMPLE, X200, 64, b""),
     "75358CF39E41494E949707927CEE0AF20A3FF553904C86B08F21CC414BCFD691589D27CF5E15369CBBFF8B9A4C2EB17800855D0235FF635DA82533EC6B759B69"),
    (kmac, (128, K_SAMPLE, X4, 32, b"", True), "CD83740BBD92CCC8CF032B1481A0F4460E7CA9DD12B08A0C4031178BACD6EC35"),
    (kmac, (256, K_SAMPLE, X4, 64, b"My Tagged Application", True),
     "1755133F1534752AAD0748F2C706FB5C784512CAB835CD15676B16C0C6647FA96FAA7AF634A0BF8FF6DF39374FA00FAD9A39E322A7C92065A64EB1FB0801EB2B"),
)


def check_pinned():
    """the restatement against hashlib and the sample table; raises AssertionError"""
    import hashlib
    for n in (0, 1, 135, 136, 137, 167, 168, 169, 400):
        m = bytes((7 * i + n) & 0xFF for i in range(n))
        assert sponge(168, m, 0x1F, 200) == hashlib.shake_128(m).digest(200), n
        assert sponge(136, m, 0x1F, 137) == hashlib.shake_256(m).digest(137), n
        assert sponge(136, m, 0x06, 32) == hashlib.sha3_256(m).digest(), n
        assert cshake(128, m, 33) == hashlib.shake_128(m).digest(33) and cshake(256, m, 33) == hashlib.shake_256(m).digest(33)
    for fn, args, hexval in SAMPLES:
        assert fn(*args).hex().upper() == hexval, (fn.__name__, args[0], len(args[1]))
