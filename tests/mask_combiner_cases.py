"""Inputs shared by the mask combiner's device-form tests (test_mask_combiner_reach.py proves on the CPU what
test_mask_combiner_dev_gpu.py relies on): the ChaCha shapes, the generator seed of each, and a vectorised count of the
candidates a seed's rand-0.3 stream rejects."""
import numpy as np

P62 = 4611686006577364993
Q_SHIFT = (1 << 62) - (1 << 51)          # 2^-11 rejection: most seeds repaired by the shift pass, some by the exact-order one
Q_HEAVY = (1 << 61) + 1                  # ~12% rejection

# (q, dimension, seeds) of test_chacha_combine_vs_oracle: the smallest shapes known to reach the clean, shift, exact-order and
# all-exact-order paths and the tail walk
CHACHA_SHAPES = [(433, 1000, 5), (P62, 4099, 9), (P62, 8, 1), (97, 3, 300), (Q_HEAVY, 3000, 6),
                 ((1 << 62) - (1 << 49), 2000, 60), (Q_SHIFT, 1500, 300), (Q_SHIFT, 40, 3000), (Q_HEAVY, 8, 500)]
BOTH_LISTS = (Q_SHIFT, 1500, 300)        # meant for both repair lists in one chunk
SHORT_STREAMS = [(Q_SHIFT, 40, 3000), (Q_HEAVY, 8, 500)]
STREAM_ORDER = (Q_SHIFT, 1000, 20)       # q, dimension, seeds per call (two calls through one device buffer)


def generator_seed(q, dim, seeds):
    """numpy seed of a shape's seed matrix (test_mask_combiner_reach.py asserts that it reaches what the shape is meant for)"""
    return dim + seeds


def seed_matrix(q, dim, seeds, words=4):
    return np.random.default_rng(generator_seed(q, dim, seeds)).integers(0, 1 << 32, size=(seeds, words), dtype=np.int64)


def stream_order_seeds():
    q, dim, n = STREAM_ORDER
    rng = np.random.default_rng(7)
    return (rng.integers(0, 1 << 32, size=(n, 4), dtype=np.int64), rng.integers(0, 1 << 32, size=(n, 4), dtype=np.int64))


def zone(q):
    """rand 0.3 Range<i64>: candidates >= zone are rejected"""
    return (1 << 64) - 1 - ((1 << 64) - 1) % q


def all_exact_order(q, dim):
    """the host-side choice the library makes from (modulus, dimension) alone"""
    return ((1 << 64) - zone(q)) / 2.0 ** 64 * dim > 1.0


def candidates(S, n_blocks):
    """the first 8 * n_blocks next_u64 values of rand-0.3 ChaChaRng::from_seed(row) for every row of S: uint64 [rows][8 n_blocks]"""
    S = np.asarray(S, dtype=np.int64)
    rows = S.shape[0]
    st = np.zeros((16, rows, n_blocks), dtype=np.uint32)
    for i, c in enumerate((0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)):
        st[i] = c
    for w in range(min(8, S.shape[1])):
        st[4 + w] = (S[:, w] & 0xFFFFFFFF).astype(np.uint32)[:, None]
    st[12] = np.arange(n_blocks, dtype=np.uint32)[None, :]
    x = st.copy()

    def rotl(v, n):
        return (v << np.uint32(n)) | (v >> np.uint32(32 - n))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7)
    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    x += st
    hi, lo = x[0::2].astype(np.uint64), x[1::2].astype(np.uint64)            # [8][rows][blocks]
    v = (hi << np.uint64(32)) | lo
    return np.ascontiguousarray(v.transpose(1, 2, 0)).reshape(rows, 8 * n_blocks)


def rejections(S, q, dim, extra=16):
    """per seed: how many of its first `dim` candidates are rejected, and whether one of the `extra` candidates after them is"""
    v = candidates(S, (dim + extra + 7) // 8)
    bad = v >= np.uint64(zone(q))
    return bad[:, :dim].sum(axis=1), bad[:, dim:dim + extra].any(axis=1)
