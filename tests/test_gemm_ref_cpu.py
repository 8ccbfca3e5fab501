"""No GPU: (1) tests/gemm_ref.py -- the float64 restatement of the bf16 GEMM that tests/test_gpu_gemm_bf16_exact.py compares every
kernel with -- against a triple loop that takes every index from the GemmArgs comment of csrc/nsd_bf16.h on its own, at tiny
sizes, for every feature and both shift signs; (2) the rejections of nsd_gemm_bf16_launch, which return before any HIP call: through
the public nsd_gemm_bf16 where it can reach the clause, else through nsd_diag_gemm_bf16 of the diagnostic library."""
import ctypes as C

import numpy as np
import pytest
import torch

import nsd_amd
from nsd_amd import _lib
from tests import gemm_ref as gr


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference against a triple loop
# ---------------------------------------------------------------------------------------------------------------------------------
def naive(A, B, M, N, K, a_off=0, lda=None, a_kmajor=False, b_off=0, ldb=None, b_kmajor=False, b_shift=0, b_period=0,
          B2=None, b2_off=0, ldb2=None, b2_shift=0, n_split=0, splits=1):
    """[splits][M][N] partial sums, one element at a time from the flat buffers"""
    A, B = np.asarray(A).reshape(-1), np.asarray(B).reshape(-1)
    B2 = None if B2 is None else np.asarray(B2).reshape(-1)
    lda = lda if lda is not None else (M if a_kmajor else K)
    ldb = ldb if ldb is not None else (N if b_kmajor else K)
    ldb2 = ldb2 if ldb2 is not None else N - n_split
    nchunks = (K + 63) // 64
    per = (nchunks + splits - 1) // splits
    out = np.zeros((splits, M, N))
    for z in range(splits):
        k_lo, k_hi = z * per * 64, min((z + 1) * per * 64, K)
        for m in range(M):
            for n in range(N):
                s = 0.0
                for k in range(k_lo, k_hi):
                    a = A[a_off + (k * lda + m if a_kmajor else m * lda + k)]
                    if not b_kmajor:
                        b = B[b_off + n * ldb + k]
                    else:
                        second = B2 is not None and n >= n_split
                        sh = b2_shift if second else b_shift
                        ks = k + sh
                        b = 0.0
                        if 0 <= ks < K and not (b_period > 0 and sh != 0 and not (0 <= k % b_period + sh < b_period)):
                            b = B2[b2_off + ks * ldb2 + (n - n_split)] if second else B[b_off + ks * ldb + n]
                    s += float(a) * float(b)
                out[z, m, n] = s
    return out


def _check(kw, A, B, M, N, K, **extra):
    got = gr.gemm_ref(A, B, M=M, N=N, K=K, **kw, **extra)
    want = naive(A, B, M, N, K, **kw)
    assert got.shape == want.shape and np.array_equal(got, want), (kw, np.argwhere(got != want)[:4])
    return got


@pytest.mark.parametrize("a_kmajor,b_kmajor", [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_ref_layouts_views_and_splits(a_kmajor, b_kmajor):
    M, N, K = 24, 16, 136                                   # two chunks and a tail of 8
    lda, ldb = (M + 8 if a_kmajor else K + 16), (N + 24 if b_kmajor else K + 8)
    A = gr.exact_operands(5 + (K if a_kmajor else M) * lda, 1, K=K)
    B = gr.exact_operands(3 + (K if b_kmajor else N) * ldb, 2, K=K)
    for splits in (1, 2, 3, 5):                             # 3 chunks: 2 + 1 (a tail chunk alone); 1 + 1 + 1; 5: two empty parts
        got = _check(dict(a_off=5, lda=lda, a_kmajor=a_kmajor, b_off=3, ldb=ldb, b_kmajor=b_kmajor, splits=splits), A, B, M, N, K)
        if splits == 5:
            assert not got[3].any() and not got[4].any() and got[2].any()
    # the sum of the partials is the whole product, and the addend lands on it
    whole = gr.gemm_ref(A, B, M=M, N=N, K=K, a_off=5, lda=lda, a_kmajor=a_kmajor, b_off=3, ldb=ldb, b_kmajor=b_kmajor)
    parts = gr.gemm_ref(A, B, M=M, N=N, K=K, a_off=5, lda=lda, a_kmajor=a_kmajor, b_off=3, ldb=ldb, b_kmajor=b_kmajor, splits=3)
    assert whole.shape == (1, M, N) and np.array_equal(parts.sum(0), whole[0])
    add = gr.exact_operands((M, N), 3, quantum=0.25)
    with_add = gr.gemm_ref(A, B, M=M, N=N, K=K, a_off=5, lda=lda, a_kmajor=a_kmajor, b_off=3, ldb=ldb, b_kmajor=b_kmajor, add=add)
    assert np.array_equal(with_add[0], whole[0] + add)


@pytest.mark.parametrize("shift,period", [(s, p) for p in (0, 8, 24, 40) for s in (-8, 8, -3, 3)])
def test_gemm_ref_shift_and_period(shift, period):
    """both signs; no period, |shift| == period (8), a period that divides neither a chunk nor K (24, 40)"""
    M, N, K = 8, 16, 80
    A, B = gr.exact_operands((K, M), 4, K=K), gr.exact_operands((K, N), 5, K=K)
    for splits in (1, 2):
        got = _check(dict(a_kmajor=True, b_kmajor=True, b_shift=shift, b_period=period, splits=splits), A, B, M, N, K)
        if period and abs(shift) == period:                  # no row has a partner inside its block: all zero
            assert not got.any()
        else:
            assert got.any()
    # against the unshifted product of an operand shifted by hand
    Bs = np.zeros_like(B)
    for k in range(K):
        ks = k + shift
        if 0 <= ks < K and (period == 0 or ks // period == k // period):
            Bs[k] = B[ks]
    want = gr.gemm_ref(A, Bs, M=M, N=N, K=K, a_kmajor=True, b_kmajor=True)
    assert np.array_equal(gr.gemm_ref(A, B, M=M, N=N, K=K, a_kmajor=True, b_kmajor=True, b_shift=shift, b_period=period), want)


@pytest.mark.parametrize("b_shift,b2_shift", [(-8, 0), (8, 0), (0, 0), (-8, 8)])
def test_gemm_ref_second_source(b_shift, b2_shift):
    M, N, K, n_split = 8, 24, 72, 16                         # (the launcher wants n_split % 256 == 0; the operation does not care)
    A, B, B2 = gr.exact_operands((K, M), 6, K=K), gr.exact_operands((K, n_split + 8), 7, K=K), gr.exact_operands(4 + K * 16, 8, K=K)
    for a_kmajor in (True, False):
        Aa = A if a_kmajor else np.ascontiguousarray(A.T)
        _check(dict(a_kmajor=a_kmajor, b_kmajor=True, ldb=n_split + 8, b_shift=b_shift, b_period=24, B2=B2, b2_off=4, ldb2=16,
                    b2_shift=b2_shift, n_split=n_split, splits=2), Aa, B, M, N, K)
    # the two halves are the two single-source products
    both = gr.gemm_ref(A, B, M=M, N=N, K=K, a_kmajor=True, b_kmajor=True, ldb=n_split + 8, b_shift=b_shift, b_period=24, B2=B2, b2_off=4,
                       ldb2=16, b2_shift=b2_shift, n_split=n_split)[0]
    first = gr.gemm_ref(A, B, M=M, N=n_split, K=K, a_kmajor=True, b_kmajor=True, ldb=n_split + 8, b_shift=b_shift, b_period=24)[0]
    second = gr.gemm_ref(A, B2, M=M, N=N - n_split, K=K, a_kmajor=True, b_kmajor=True, b_off=4, ldb=16, b_shift=b2_shift, b_period=24)[0]
    assert np.array_equal(both[:, :n_split], first) and np.array_equal(both[:, n_split:], second)


def test_gemm_ref_rounding_and_tile_layouts():
    # round to nearest even against torch's conversion, ties included
    x = np.concatenate([np.arange(-2100, 2100) * 0.25, [129.5, 130.5, -129.5, -130.5, 257.0, 259.0, 65.25, 65.75]]).astype(np.float32)
    assert gr.bf16_ties(x) > 100
    assert np.array_equal(gr.bf16_rne(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert gr.bf16_rne(np.float32([129.5, 130.5, 257.0, 259.0])).tolist() == [130.0, 130.0, 256.0, 260.0]
    M, N, K = 64, 96, 72
    A, B = gr.exact_operands((M, K), 9, K=K), gr.exact_operands((N, K), 10, K=K)
    bias = gr.exact_operands(M, 11, quantum=0.25)
    c = naive(A, B, M, N, K)[0]
    assert np.array_equal(gr.gemm_ref(A, B, M=M, N=N, K=K, epilogue=1), gr.bf16_rne(c.astype(np.float32)))
    cb = torch.from_numpy((c + bias[:, None]).astype(np.float32)).to(torch.bfloat16).float().numpy()
    t2 = gr.gemm_ref(A, B, M=M, N=N, K=K, epilogue=2, bias=bias)
    t3 = gr.gemm_ref(A, B, M=M, N=N, K=K, epilogue=3, bias=bias)
    assert t2.shape == (N // 32, M // 32, 64, 16) and t3.shape == (N // 32, M // 32, 4, 64, 4)
    f2, f3 = t2.reshape(-1), t3.reshape(-1)
    for nt in range(N // 32):
        for mt in range(M // 32):
            for lane in range(64):
                for r in range(16):
                    want = cb[32 * mt + 8 * (r // 4) + 4 * (lane >> 5) + r % 4, 32 * nt + (lane & 31)]
                    assert f2[((nt * (M // 32) + mt) * 64 + lane) * 16 + r] == want
                    assert f3[(((nt * (M // 32) + mt) * 4 + r // 4) * 64 + lane) * 4 + r % 4] == want
    assert not np.array_equal(t2, gr.gemm_ref(A, B, M=M, N=N, K=K, epilogue=2))          # the bias is in


def test_exact_operands_and_the_exactness_condition():
    v = gr.exact_operands((300, 40), 0, K=65536)
    assert v.dtype == np.float32 and np.all(v != 0) and np.all(v * 2 == np.round(v * 2)) and np.abs(v).max() == 4
    assert set(np.unique(np.abs(v))) == {0.5 * i for i in range(1, 9)}
    assert np.array_equal(torch.from_numpy(v).to(torch.bfloat16).float().numpy(), v)      # bf16 holds them
    q = gr.exact_operands(1000, 1, quantum=0.25)
    assert np.all(q != 0) and np.all(q * 4 == np.round(q * 4)) and np.abs(q).max() <= 4
    gr.assert_exact(65536, extra=4.0)
    assert 65536 * 16 * 4 * 4 <= 2 ** 24                                                  # met 4 times over at the largest K in use
    with pytest.raises(AssertionError):
        gr.assert_exact(1 << 18)
    # the claim itself on the host: a sum of such products in fp32, in any order, is the float64 sum
    a, b = gr.exact_operands(4096, 2), gr.exact_operands(4096, 3)
    p = a * b
    want = float(np.sum(p.astype(np.float64)))
    for order in (np.arange(4096), np.arange(4096)[::-1], np.random.RandomState(0).permutation(4096)):
        s = np.float32(0)
        for i in order:
            s = np.float32(s + p[i])
        assert float(s) == want
    assert gr.split_ranges(200, 3) == [(0, 128), (128, 200), (200, 200)] and gr.split_ranges(64, 2) == [(0, 64), (64, 64)]


# ---------------------------------------------------------------------------------------------------------------------------------
# what the launcher refuses, before any HIP call
# ---------------------------------------------------------------------------------------------------------------------------------
E_INVALID = -1
FAKE = 4096                                                  # never dereferenced: every call below is refused first


def _public(L, *, lda=64, a_kmajor=0, ldb=64, b_kmajor=0, b_shift=0, ldc=64, epilogue=0, M=64, N=64, K=64, splits=1):
    return L.nsd_gemm_bf16(FAKE, lda, a_kmajor, FAKE, ldb, b_kmajor, b_shift, FAKE, ldc, epilogue, None, M, N, K, splits, None)


def test_gemm_launcher_rejections_through_the_public_entry():
    L = nsd_amd.load_library()
    for kw, text in ((dict(K=60), b"multiples of 8"), (dict(lda=68), b"multiples of 8"), (dict(ldb=68), b"multiples of 8"),
                     (dict(a_kmajor=1, M=60), b"multiples of 8"), (dict(b_kmajor=1, N=60), b"multiples of 8"),
                     (dict(epilogue=2, M=80), b"tile output"), (dict(epilogue=3, N=80), b"tile output"),
                     (dict(epilogue=2, M=80, N=80), b"tile output"), (dict(b_shift=8), b"b_shift needs a k-major B"),
                     (dict(b_shift=-8, a_kmajor=1), b"b_shift needs a k-major B"), (dict(M=0), b"empty problem")):
        assert _public(L, **kw) == E_INVALID, kw
        assert text in L.nsd_last_error(), (kw, L.nsd_last_error())
    assert L.nsd_gemm_bf16(None, 64, 0, FAKE, 64, 0, 0, FAKE, 64, 0, None, 64, 64, 64, 1, None) == E_INVALID
    assert not hasattr(L, "nsd_diag_gemm_bf16") and not hasattr(L, "nsd_diag_reduce_dw") and not hasattr(L, "nsd_diag_reduce_db")


def _diag(DL, **kw):
    f = dict(A=FAKE, B=FAKE, lda=512, ldb=512, a_kmajor=1, b_kmajor=1, b_shift=0, b_period=0, B2=None, ldb2=0, b2_shift=0, n_split=0,
             epilogue=0, C=FAKE, ldc=512, bias=None, add=None, M=512, N=512, K=512, splits=1, kernel=0)
    f.update(kw)
    return DL.nsd_diag_gemm_bf16(C.byref(_lib.DiagGemm(**f)), None)


def test_gemm_launcher_rejections_through_the_diagnostic_entry():
    """b_period, the second source, the addend and the kernel selector: each case breaks ONE clause of an otherwise legal call"""
    two = dict(B2=FAKE, ldb2=256, n_split=256)               # a legal second source: N = 512, n_split = 256
    cases = [
        (dict(b_period=-64), b"bad b_period"), (dict(b_period=64, b_shift=72), b"bad b_period"),
        (dict(b_period=64, b_shift=-72), b"bad b_period"), (dict(b_period=64, b_shift=32, K=1 << 31), b"bad b_period"),
        (dict(two, b_kmajor=0), b"second B source"), (dict(two, n_split=0), b"second B source"), (dict(two, n_split=-256), b"second B source"),
        (dict(two, n_split=512), b"second B source"), (dict(two, n_split=768), b"second B source"), (dict(two, n_split=128), b"second B source"),
        # ((N - n_split) % 8 cannot fail alone: N % 8 == 0 is asked of every k-major B first, n_split % 256 == 0 beside it)
        (dict(two, ldb2=260), b"second B source"), (dict(two, N=516, ldb=520, ldc=520), b"multiples of 8"),
        (dict(add=FAKE, epilogue=1), b"addend needs"), (dict(add=FAKE, splits=2), b"addend needs"),
        (dict(add=FAKE, epilogue=2), b"addend needs"),
        # the selector: unknown; a 256 x 256 kernel without a whole tile; the LDS-DMA kernel with a k-major operand or beyond its
        # descriptor range (256 rows of lda or ldb elements + K must stay below 0x7f000000 bytes)
        (dict(kernel=3), b"unknown kernel selector"), (dict(kernel=-1), b"unknown kernel selector"), (dict(kernel=33), b"unknown kernel selector"),
        (dict(kernel=2, M=248), b"needs M, N >= 256"), (dict(kernel=2, N=248), b"needs M, N >= 256"),
        (dict(kernel=22, a_kmajor=0, b_kmajor=0, N=128), b"needs M, N >= 256"),
        (dict(kernel=22), b"k-contiguous"), (dict(kernel=23, a_kmajor=0), b"k-contiguous"), (dict(kernel=32, b_kmajor=0), b"k-contiguous"),
        (dict(kernel=22, a_kmajor=0, b_kmajor=0, lda=1 << 22), b"descriptor range"),
        (dict(kernel=32, a_kmajor=0, b_kmajor=0, ldb=1 << 22), b"descriptor range"),
    ]
    with _lib.diagnostic_library() as DL:
        for kw, text in cases:
            assert _diag(DL, **kw) == E_INVALID, kw
            assert text in DL.nsd_last_error(), (kw, DL.nsd_last_error())
        # the argument checks come before the selector's: a bad problem is refused whatever kernel is asked for
        assert _diag(DL, kernel=1, a_kmajor=0, K=60) == E_INVALID and b"multiples of 8" in DL.nsd_last_error()
        assert DL.nsd_diag_gemm_bf16(None, None) == E_INVALID
        assert DL.nsd_diag_reduce_dw(None, 1, 64, 64, 64, FAKE, None) == E_INVALID
        assert DL.nsd_diag_reduce_dw(FAKE, 1, 64, 64, 72, FAKE, None) == E_INVALID       # I > N
        assert DL.nsd_diag_reduce_dw(FAKE, 0, 64, 64, 64, FAKE, None) == E_INVALID
        assert DL.nsd_diag_reduce_db(FAKE, 1, 64, None, FAKE, None) == E_INVALID
        assert DL.nsd_diag_reduce_db(FAKE, 0, 64, FAKE, FAKE, None) == E_INVALID


def test_gemm_bf16_diag_needs_the_diagnostic_library():
    from nsd_amd import ops
    t = torch.zeros(8, dtype=torch.bfloat16)
    with pytest.raises(nsd_amd.NsdError, match="diagnostic build"):
        ops.gemm_bf16_diag(t, t, t, M=8, N=8, K=8)
    with pytest.raises(nsd_amd.NsdError, match="diagnostic build"):
        ops.reduce_dw_diag(torch.zeros(8), 1, 1, 1, 1)
    with _lib.diagnostic_library():
        with pytest.raises(nsd_amd.NsdError, match="on the MI355X"):                    # host tensors are refused: no CPU path
            ops.gemm_bf16_diag(t, t, t, M=8, N=8, K=8)
