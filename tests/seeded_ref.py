"""numpy restatement of seeded ciphertexts over the oracle's ChaCha20, sampler, encode
and NTT.  Test infrastructure: tests/test_seeded_ref.py checks it for meaning on the CPU (the draw against
keygen's, the ciphertext under oracle.decrypt), tests/test_gpu_seeded_wire.py compares the HIP path with it
bit for bit.

The c1 stream: ciphertext k of its blob, tower t, coefficient j of the stored EVALUATION order <- the
ChaCha20 block with key = the blob's 32-byte seed (eight little-endian words), counter j >> 2, nonce
(9 << 56) | (k << 8) | t, read as eight 64-bit words: lo = word 2 (j & 3), hi = the next, a = (hi 2^64 + lo)
mod q_t.  The seed of a call: the first eight words of the block (counter 0, nonce (9 << 56) | g0) of the
call's stream key."""
import numpy as np

import arena_layout as A
import oracle as O

DOMAIN = 9 << 56
LEAD_BYTES = 128  # the 64-byte header, the 32-byte seed, 32 zero bytes


def block_draw(key_words, nonce, block, q):
    """The four residues j = 4 block .. 4 block + 3 of one ChaCha20 block."""
    w = [int(v) for v in O.chacha20_block(key_words, block, nonce)]
    out = []
    for i in range(4):
        lo = w[4 * i] | (w[4 * i + 1] << 32)
        hi = w[4 * i + 2] | (w[4 * i + 3] << 32)
        out.append(((hi << 64) | lo) % int(q))
    return out


def uniform_draw(key_words, nonce, N, q):
    """N residues mod q from blocks 0 .. N / 4 - 1 of (key, nonce): keygen's draw of a_t."""
    out = np.zeros(N, np.uint64)
    for b in range(N // 4):
        out[4 * b:4 * b + 4] = block_draw(key_words, nonce, b, q)
    return out


def seed_words(seed_bytes):
    assert len(seed_bytes) == 32
    return np.frombuffer(bytes(seed_bytes), dtype="<u4").copy()


def nonce(k, t):
    assert 0 <= k < 1 << 48 and 0 <= t < 256
    return DOMAIN | (k << 8) | t


def expand(seed_bytes, k, moduli, N):
    """c1 [L][N] of ciphertext k of the blob with this seed."""
    key = seed_words(seed_bytes)
    return np.stack([uniform_draw(key, nonce(k, t), N, q) for t, q in enumerate(moduli)])


def expand_blocks(seed_bytes, k, t, q, blocks):
    """{block: its four residues} of row (k, t): the large rings are checked on a sample of blocks."""
    key = seed_words(seed_bytes)
    return {b: block_draw(key, nonce(k, t), b, q) for b in blocks}


def call_seed(seed_int, g0):
    """The public seed of the encrypt call whose stream key comes from set_seed(seed_int) and whose first
    ciphertext has the global index g0."""
    return O.chacha20_block(O.seed_to_key(seed_int), 0, DOMAIN | g0)[:8].astype("<u4").tobytes()


def mulmod(a, b, q):
    return np.array([int(x) * int(y) % int(q) for x, y in zip(a, b)], np.uint64)


def encrypt_seeded(x, sk_eval, seed_int, g, seed_bytes, k, N, slots, delta, q, psi):
    """(c0, c1) [2][L][N] of one ciphertext: c1 = expand(...), c0_t = NTT(m + e) - c1_t . sk_t with m the
    encode of x (at most `slots` values) and e the e0 of the public-key encrypt at (seed_int, g)."""
    me = O.encode_coeffs(x, N, slots, delta) + O.sample_encrypt(seed_int, g, N)[1]
    c1 = expand(seed_bytes, k, q, N)
    c0 = np.zeros_like(c1)
    for t in range(len(q)):
        qt = int(q[t])
        r = np.array([int(v) % qt for v in me], np.uint64)
        u = O.ntt_fwd(r, qt, int(psi[t]))
        c0[t] = (u + np.uint64(qt) - mulmod(c1[t], sk_eval[t], qt)) % np.uint64(qt)
    return np.stack([c0, c1])


def packed_poly_bytes(q, N):
    return N * sum(A.widths(q)) // 8


def blob_payload(c0s, q, N):
    """The payload of a seeded blob (bytes from offset 128): ciphertext k's c0 [L][N] as one group of the
    packed wire format -- the first half of pack_one's two groups of a ciphertext (c0, anything)."""
    out = []
    for c0 in c0s:
        ct = np.stack([c0, np.zeros_like(c0)])[None]
        words = A.pack_one(ct, q, N)
        out.append(words[:words.size // 2].tobytes())
    return b"".join(out)
