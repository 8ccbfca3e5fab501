"""The bf16 GEMM of the sequence path (csrc/nsd_gemm_bf16.hip) restated in float64 numpy from the GemmArgs comment of
csrc/nsd_bf16.h, and operands for which that product is EXACT in fp32.  A plain helper module; tests/test_gemm_ref_cpu.py holds
gemm_ref to a triple loop, tests/test_gpu_gemm_bf16_exact.py holds every kernel to gemm_ref bit for bit.

Why a GEMM can be tested without a tolerance: with operands that are multiples of 0.5 of magnitude <= 4 every product is a multiple
of 0.25 of magnitude <= 16, and so is every partial sum of at most K of them, of magnitude <= 16 K.  A multiple of 0.25 below 2^22 in
magnitude is an fp32 number (24 bits of significand), so while 16 K * 4 < 2^24 NO addition of the accumulation rounds, whatever
its order: tile, split, kernel and pipeline cannot change a bit of the result, and it equals the float64 product."""
import numpy as np

GK = 64                                                  # rows of a K chunk: split-K ranges are whole chunks


def exact_operands(shape, seed, quantum=0.5, K=None):
    """NONZERO multiples of `quantum` (0.5: operands; 0.25: bias and addend) with |v| <= 4, float32.  No zero: a dropped or doubled
    element always changes its sum.  K: the rows of the contraction the values go into -- assert_exact's condition is asserted for it."""
    if K is not None:
        assert_exact(K, extra=4.0)
    rs = np.random.RandomState(seed)
    n = int(round(4 / quantum))
    mag = rs.randint(1, n + 1, size=shape)
    sign = 2 * rs.randint(0, 2, size=shape) - 1
    v = (mag * sign * quantum).astype(np.float32)
    assert np.all(v != 0) and np.abs(v).max() <= 4
    return v


def assert_exact(K, extra=0.0):
    """the condition of the module's docstring for a contraction over K rows (+ a bias or addend of magnitude <= extra, a multiple
    of 0.25): every intermediate is a multiple of 0.25 below 2^22"""
    assert (K * 16 + extra) * 4 < 2 ** 24, K


def view(full, off, rows, cols, ld):
    """rows x cols elements of the flat buffer `full`, row r at off + r * ld"""
    flat = np.asarray(full).reshape(-1)
    idx = off + np.arange(rows, dtype=np.int64)[:, None] * ld + np.arange(cols, dtype=np.int64)[None, :]
    assert idx.min() >= 0 and idx.max() < flat.size, (off, rows, cols, ld, flat.size)
    return flat[idx]


def split_ranges(K, splits):
    """[(k_lo, k_hi)] of the `splits` parts: per = ceil(ceil(K / 64) / splits) chunks of 64 each; a part beyond the last chunk is empty"""
    nchunks = -(-K // GK)
    per = -(-nchunks // splits)
    out = []
    for z in range(splits):
        lo, hi = min(z * per, nchunks), min((z + 1) * per, nchunks)
        out.append((min(lo * GK, K), min(hi * GK, K)))
    return out


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even) as float32; finite inputs"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_ties(x):
    """how many elements of the float32 array lie exactly between two bf16 numbers"""
    return int(np.count_nonzero((np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & 0xFFFF) == 0x8000))


def tile_rows():
    """[64 lanes][16 registers] -> row of the 32 x 32 accumulator tile: 8 (r / 4) + 4 (l >> 5) + r % 4; the column is l & 31"""
    lane, r = np.arange(64)[:, None], np.arange(16)[None, :]
    return 8 * (r // 4) + 4 * (lane >> 5) + (r % 4), np.broadcast_to(lane & 31, (64, 16))


def to_tiles(c, wave_major=False):
    """[M][N] -> accumulator tiles [N/32][M/32][64][16], or register group first [N/32][M/32][4][64][4]"""
    M, N = c.shape
    assert M % 32 == 0 and N % 32 == 0
    rows, cols = tile_rows()
    t = c.reshape(M // 32, 32, N // 32, 32).transpose(2, 0, 1, 3)[:, :, rows, cols]      # [N/32][M/32][64][16]
    return np.ascontiguousarray(t.reshape(N // 32, M // 32, 64, 4, 4).transpose(0, 1, 3, 2, 4)) if wave_major else np.ascontiguousarray(t)


def shifted_rows(K, shift, period):
    """(source row, valid) per row k of the contraction: row k meets row k + shift of the operand; it reads zero where that row leaves
    [0, K), or, with period > 0 and a shift, leaves k's own block of `period` rows"""
    k = np.arange(K, dtype=np.int64)
    ks = k + shift
    ok = (ks >= 0) & (ks < K)
    if period > 0 and shift != 0:
        kin = k % period + shift
        ok &= (kin >= 0) & (kin < period)
    return np.where(ok, ks, 0), ok


def gemm_ref(A, B, *, M, N, K, a_off=0, lda=None, a_kmajor=False, b_off=0, ldb=None, b_kmajor=False, b_shift=0, b_period=0,
             B2=None, b2_off=0, ldb2=None, b2_shift=0, n_split=0, epilogue=0, bias=None, add=None, splits=1):
    """C[m][n] = sum_k A(m, k) B(k, n) in float64.  A, B, B2: buffers of any shape, read flat; an operand is the view from *_off with
    leading dimension ld* (default: its own row length).  A is [M][lda], or [K][lda] when a_kmajor; B [N][ldb], or [K][ldb] when
    b_kmajor; row k of A meets row k + b_shift of a k-major B (shifted_rows); columns n >= n_split come from B2 [K][ldb2] with
    b2_shift (and the same period) where B2 is given.
    epilogue 0 -> float64 [splits][M][N]: the partial of every split-K range (split_ranges), + add [M][N] where splits == 1;
             1 -> float32 [M][N] rounded to bf16, ties to even;
             2 -> [N/32][M/32][64][16] accumulator tiles of C + bias[m], rounded likewise;  3 -> [N/32][M/32][4][64][4]."""
    lda = lda if lda is not None else (M if a_kmajor else K)
    ldb = ldb if ldb is not None else (N if b_kmajor else K)
    Am = view(A, a_off, K, M, lda).T if a_kmajor else view(A, a_off, M, K, lda)          # [M][K]
    Am = Am.astype(np.float64)
    if b_kmajor:
        n1 = n_split if B2 is not None else N
        src, ok = shifted_rows(K, b_shift, b_period)
        Bm = np.where(ok[:, None], view(B, b_off, K, n1, ldb)[src], 0).astype(np.float64)
        if B2 is not None:
            assert 0 < n_split < N
            src2, ok2 = shifted_rows(K, b2_shift, b_period)
            ldb2 = ldb2 if ldb2 is not None else N - n_split
            Bm = np.concatenate([Bm, np.where(ok2[:, None], view(B2, b2_off, K, N - n_split, ldb2)[src2], 0).astype(np.float64)], axis=1)
    else:
        assert b_shift == 0 and B2 is None
        Bm = view(B, b_off, N, K, ldb).T.astype(np.float64)                              # [K][N]
    splits = splits if (epilogue == 0 and splits > 1) else 1
    parts = np.zeros((splits, M, N), dtype=np.float64)
    for z, (lo, hi) in enumerate(split_ranges(K, splits)):
        if lo < hi:
            parts[z] = Am[:, lo:hi] @ Bm[lo:hi]
    if epilogue == 0:
        if add is not None:
            assert splits == 1
            parts[0] += np.asarray(add, dtype=np.float64).reshape(M, N)
        return parts
    c = parts[0]
    if epilogue == 1:
        return bf16_rne(c.astype(np.float32))
    if bias is not None:
        c = c + np.asarray(bias, dtype=np.float64).reshape(M, 1)
    return to_tiles(bf16_rne(c.astype(np.float32)), wave_major=(epilogue == 3))
