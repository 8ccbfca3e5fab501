"""The bf16 GEMM of the sequence path (csrc/nsd_gemm_bf16.hip) held BIT FOR BIT to the float64 product, on every kernel and route.
Needs a real MI355X: run with `pytest -m gpu`.

No tolerance anywhere: the operands are nonzero multiples of 0.5 with |v| <= 4 (tests/gemm_ref.py, exact_operands), so every product
and every partial sum is an fp32 number and the result does not depend on summation order, tile, split or kernel -- it IS the
float64 product (gemm_ref, held to a triple loop by tests/test_gemm_ref_cpu.py), computed on the host.  Every comparison is
np.array_equal on the whole output buffer, sentinel padding included; a mismatch prints its count and the first few
(plane, m, n, got, want).  Kernels are pinned through ops.gemm_bf16_diag (nsd_diag_gemm_bf16 of the diagnostic library: 1 the
128 x 128 kernel, 2 the register-staged 256 x 256 kernel, 22 / 23 / 32 the LDS-DMA kernel with those stages) or chosen by the
launcher (0) at shapes that fill the machine: tiles * splits >= CUs, from the `cus` fixture.

Sections: (a) kernel x operand layout, ragged M and N, padded output; (b) K of 1..5 chunks with and without a tail on every pipeline;
(c) split-K, every partial; (d) views: column block of a wider k-major A, ldb > N, ldc > N; (e) b_shift with and without b_period;
(f) the second B source, then seq_reduce_dw_kernel / seq_reduce_db_kernel on the partials; (g) bf16, tile and wave-major tile
epilogues at exact ties, and the addend; (h) the XCD-aware tile order.

Wall time of the file on one MI355X and what three deliberately wrong kernels fail here: profiles/gemm_bf16_exact.md."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as gr
from tests.gpu_harness import cus, dev, nsd, sync_at_the_end  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F32_SENTINEL = 1234.5625          # not a multiple of 0.25: no sum of the exact operands can be it
BF16_SENTINEL = 3.140625          # a bf16 number that no rounded multiple of 0.25 is
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
DMA = (22, 23, 32)


def _ragged(n, kmajor):
    """a size that is no multiple of the tile; of 8 only where the layout wants 16-byte pieces along it"""
    return n - n % 8 if kmajor else n


class Problem:
    """One GEMM problem on exact operands: the buffers (every element nonzero, the padding of a leading dimension included), the
    float64 reference laid into a sentinel-filled copy of the output buffer, and check(kernel): run, compare the whole buffer."""

    def __init__(self, dev, M, N, K, *, a_kmajor=False, b_kmajor=False, a_off=0, lda=None, b_off=0, ldb=None, ldc=None, epilogue=0,
                 splits=1, bias=False, add=False, b_shift=0, b_period=0, n_split=0, b2_off=0, ldb2=None, b2_shift=0, seed=0):
        gr.assert_exact(K, extra=4.0)
        self.dev, self.M, self.N, self.K, self.epilogue = dev, M, N, K, epilogue
        second = n_split > 0
        lda = lda if lda is not None else (M if a_kmajor else K)
        ldb = ldb if ldb is not None else ((n_split if second else N) if b_kmajor else K)
        self.ldc = ldc = ldc if ldc is not None else N
        A = gr.exact_operands(a_off + (K if a_kmajor else M) * lda, 1000 + seed)
        B = gr.exact_operands(b_off + (K if b_kmajor else N) * ldb, 2000 + seed)
        self.A, self.B = A, B
        self.kw = dict(M=M, N=N, K=K, a_off=a_off, lda=lda, a_kmajor=a_kmajor, b_off=b_off, ldb=ldb, b_kmajor=b_kmajor, b_shift=b_shift,
                       b_period=b_period, epilogue=epilogue, splits=splits)
        B2 = None
        if second:
            ldb2 = ldb2 if ldb2 is not None else N - n_split
            B2 = gr.exact_operands(b2_off + K * ldb2, 3000 + seed)
            self.kw.update(b2_off=b2_off, ldb2=ldb2, b2_shift=b2_shift, n_split=n_split)
        self.bias = gr.exact_operands(M, 4000 + seed, quantum=0.25) if bias else None
        self.add = gr.exact_operands((M, ldc), 5000 + seed, quantum=0.25) if add else None
        ref = gr.gemm_ref(A, B, B2=B2, bias=self.bias, add=None if self.add is None else self.add[:, :N], **self.kw)
        self.ref = ref
        self.planes = ref.shape[0] if epilogue == 0 else 1
        if epilogue in (0, 1):                               # [planes][M][ldc], then three more rows and a bit: all sentinel
            body = self.planes * M * ldc
            want = np.full(body + 3 * ldc + 5, F32_SENTINEL if epilogue == 0 else BF16_SENTINEL, dtype=np.float32)
            want[:body].reshape(self.planes, M, ldc)[:, :, :N] = ref.astype(np.float32).reshape(self.planes, M, N)
        else:
            want = np.full(M * N + 64, BF16_SENTINEL, dtype=np.float32)
            want[:M * N] = ref.reshape(-1)
        self.want = want
        bf = lambda a: None if a is None else torch.from_numpy(a).to(dev).to(torch.bfloat16)
        f32 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.a_d, self.b_d, self.b2_d, self.bias_d, self.add_d = bf(A), bf(B), bf(B2), f32(self.bias), f32(self.add)

    def run(self, kernel):
        """-> the whole output buffer as float32 numpy (bf16 outputs widened: exact)"""
        from nsd_amd import _lib, ops
        c = torch.full((self.want.size,), F32_SENTINEL if self.epilogue == 0 else BF16_SENTINEL,
                       dtype=torch.float32 if self.epilogue == 0 else torch.bfloat16, device=self.dev)
        with _lib.diagnostic_library():
            ops.gemm_bf16_diag(self.a_d, self.b_d, c, kernel=kernel, b2=self.b2_d, ldc=self.ldc, bias=self.bias_d, add=self.add_d, **self.kw)
        torch.cuda.synchronize()
        self.c = c
        return c.float().cpu().numpy()

    def check(self, kernel, tag=""):
        bad = self.mismatches(kernel)
        assert not bad, f"{tag} kernel {kernel}: {bad}"

    def mismatches(self, kernel):
        """'' where the buffer equals the reference's bit for bit, else the count and the first few (plane, m, n, got, want)"""
        got = self.run(kernel)
        if np.array_equal(got, self.want):
            return ""
        idx = np.flatnonzero(~(got == self.want))
        body = self.planes * self.M * self.ldc if self.epilogue in (0, 1) else self.M * self.N
        first = []
        for i in idx[:6]:
            if i >= body:
                first.append(("past the end", int(i - body), float(got[i]), float(self.want[i])))
            elif self.epilogue in (0, 1):
                z, rem = divmod(int(i), self.M * self.ldc)
                first.append((z, rem // self.ldc, rem % self.ldc, float(got[i]), float(self.want[i])))
            else:
                first.append(("tile", int(i) // 1024, "element", int(i) % 1024, float(got[i]), float(self.want[i])))
        msg = f"{idx.size} of {got.size} elements differ, first (plane, m, n, got, want): {first}"
        print(f"M={self.M} N={self.N} K={self.K} {self.kw} kernel {kernel}: {msg}")
        return msg


def _fill(cus):
    """tile counts (4, n) of a 256 x 256 kernel that fill the machine without split-K"""
    return 4, -(-cus // 4) + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) kernel x layout
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_kmajor,b_kmajor", LAYOUTS)
def test_a_small_tile_kernel_all_layouts(nsd, dev, a_kmajor, b_kmajor):
    """2 x 2 tiles of 128 x 128, ragged in M, N (no multiples of 8 where the layout allows) and K; pinned, and as the launcher's choice"""
    p = Problem(dev, _ragged(197, a_kmajor), _ragged(141, b_kmajor), 136, a_kmajor=a_kmajor, b_kmajor=b_kmajor,
                ldc=_ragged(141, b_kmajor) + 5, seed=1)
    p.check(1)
    p.check(0)


@pytest.mark.parametrize("a_kmajor,b_kmajor", LAYOUTS)
def test_a_register_staged_big_kernel_all_layouts_pinned(nsd, dev, a_kmajor, b_kmajor):
    """2 x 2 tiles of 256 x 256; (False, False) is reachable only through the selector"""
    p = Problem(dev, _ragged(333, a_kmajor), _ragged(285, b_kmajor), 136, a_kmajor=a_kmajor, b_kmajor=b_kmajor,
                ldc=_ragged(285, b_kmajor) + 3, seed=2)
    p.check(2)


@pytest.mark.parametrize("a_kmajor,b_kmajor", LAYOUTS[1:])
def test_a_register_staged_big_kernel_by_shape(nsd, dev, cus, a_kmajor, b_kmajor):
    """the launcher's own choice where a k-major operand fills the machine: 4 tiles along N, ceil(cus / 4) + 1 along M"""
    tn, tm = _fill(cus)
    p = Problem(dev, _ragged((tm - 1) * 256 + 77, a_kmajor), _ragged((tn - 1) * 256 + 141, b_kmajor), 72, a_kmajor=a_kmajor,
                b_kmajor=b_kmajor, seed=3)
    assert -(-p.M // 256) * -(-p.N // 256) >= cus
    p.check(0)


@pytest.mark.parametrize("mode", DMA)
def test_a_dma_kernel_each_stage_mode_pinned_and_by_shape(nsd, dev, cus, mode):
    """LDS-DMA kernel: each stage mode pinned at 2 x 2 ragged tiles, and as the launcher chooses it by shape: M >= 4 N -> 32,
    N >= 4 M -> 23, neither -> 22 (tiles >= CUs each time)"""
    Problem(dev, 333, 285, 136, ldc=290, seed=4).check(mode, "pinned")
    few, many = _fill(cus)
    side = int(np.ceil(np.sqrt(cus)))
    tm, tn = {32: (many, few), 23: (few, many), 22: (side, side)}[mode]
    M, N = (tm - 1) * 256 + 77, (tn - 1) * 256 + 141
    assert tm * tn >= cus and (M >= 4 * N) == (mode == 32) and (N >= 4 * M) == (mode == 23)
    p = Problem(dev, M, N, 136, seed=5)
    p.check(0, "by shape")
    if mode != 22:
        p.check(mode, "pinned at the large shape")


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) K edges of the pipelines: 1..5 chunks of 64, with and without a tail
# ---------------------------------------------------------------------------------------------------------------------------------
K_EDGES = (8, 56, 64, 72, 128, 136, 192, 200, 264)


@pytest.mark.parametrize("kernel,a_kmajor,b_kmajor", [(22, False, False), (23, False, False), (32, False, False), (2, False, False),
                                                      (2, True, True), (1, False, False), (1, True, True)])
def test_b_k_edges(nsd, dev, kernel, a_kmajor, b_kmajor):
    """the counted vmcnt(4) pipeline of the 3-stage modes at 1, 2, 3 chunks, the double buffers at 1 and 2, every tail"""
    M, N = (197, 141) if kernel == 1 else (333, 285)
    bad = {}
    for K in K_EDGES:
        p = Problem(dev, _ragged(M, a_kmajor), _ragged(N, b_kmajor), K, a_kmajor=a_kmajor, b_kmajor=b_kmajor, seed=10 + K)
        msg = p.mismatches(kernel)
        if msg:
            bad[K] = msg
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) split-K: every partial against the reference's partial of that k range
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,a_kmajor,b_kmajor", [(1, False, False), (1, True, True), (2, True, True), (2, False, True), (22, False, False),
                                                      (23, False, False), (32, False, False)])
def test_c_split_k_partials_pinned(nsd, dev, kernel, a_kmajor, b_kmajor):
    """K = 328: five chunks and a tail of 8.  splits 1; 3 divides the six chunks; 6 leaves the last part the tail chunk alone; 4 and 8
    leave one and two parts empty: exact zeros over the sentinel"""
    M, N = (200, 136) if kernel == 1 else (336, 288)
    bad = {}
    for splits in (1, 3, 6, 4, 8):
        p = Problem(dev, M, N, 328, a_kmajor=a_kmajor, b_kmajor=b_kmajor, splits=splits, ldc=N + 4, seed=20 + splits)
        assert p.planes == splits and [hi - lo for lo, hi in gr.split_ranges(328, splits)][-1] == {1: 328, 3: 72, 6: 8, 4: 0, 8: 0}[splits]
        msg = p.mismatches(kernel)
        if msg:
            bad[splits] = msg
    assert not bad, bad


@pytest.mark.parametrize("a_kmajor,b_kmajor", [(False, False), (True, True)])
def test_c_split_k_fills_the_machine(nsd, dev, cus, a_kmajor, b_kmajor):
    """M = N = 512 with ceil(cus / 4) parts: the launcher's own choice of a 256 x 256 kernel through split-K (LDS-DMA 22 for two
    k-contiguous operands, register-staged for the weight gradients' layout); one chunk per part, the last one the tail"""
    splits = -(-cus // 4)
    K = 64 * (splits - 1) + 8
    p = Problem(dev, 512, 512, K, a_kmajor=a_kmajor, b_kmajor=b_kmajor, splits=splits, seed=30)
    assert 4 * splits >= cus and gr.split_ranges(K, splits)[-1] == (K - 8, K)
    p.check(0)


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) views
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("d", [0, 1])
def test_d_kmajor_column_block_and_wide_b(nsd, dev, kernel, d):
    """as weight_grads passes da: direction d's column block of [K][2 M], lda = 2 M; B with ldb > N; C with ldc > N"""
    M, N = (200, 136) if kernel == 1 else (328, 264)
    Problem(dev, M, N, 200, a_kmajor=True, b_kmajor=True, a_off=d * M, lda=2 * M, b_off=16, ldb=N + 24, ldc=N + 8, splits=2, seed=40 + d).check(kernel)


@pytest.mark.parametrize("kernel", [1, 2, 22, 23, 32])
@pytest.mark.parametrize("epilogue", [0, 1])
def test_d_row_major_views_and_ldc(nsd, dev, kernel, epilogue):
    """k-contiguous operands inside wider rows (lda, ldb > K, offsets) and ldc > N for the fp32 and the bf16 epilogue: the sentinel
    columns and the rows past M stay"""
    M, N = (197, 141) if kernel == 1 else (333, 285)
    Problem(dev, M, N, 200, a_off=24, lda=264, b_off=8, ldb=216, ldc=N + 11, epilogue=epilogue, seed=50).check(kernel)


# ---------------------------------------------------------------------------------------------------------------------------------
# (e) shift and period (the recurrent weight gradient: row k of da meets row k -+ 32 of h inside its batch tile's T * 32 rows)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_e_shift_with_period(nsd, dev, kernel, T):
    """three batch-tile blocks of T * 32 rows, shift -+32, with and without split-K (T = 5: part boundaries inside a block; T = 1:
    |shift| == period, the product is zero)"""
    M, N = (200, 136) if kernel == 1 else (264, 272)
    K = 3 * T * 32
    bad = {}
    for shift in (-32, 32):
        for splits in (1, 3):
            p = Problem(dev, M, N, K, a_kmajor=True, b_kmajor=True, b_shift=shift, b_period=T * 32, splits=splits, seed=60 + T)
            assert p.ref.any() == (T > 1)
            msg = p.mismatches(kernel)
            if msg:
                bad[(shift, splits)] = msg
    assert not bad, bad


@pytest.mark.parametrize("kernel", [1, 2])
def test_e_shift_without_period(nsd, dev, kernel):
    M, N = (200, 136) if kernel == 1 else (264, 272)
    bad = {}
    for shift in (-8, 8, -32, 32):
        p = Problem(dev, M, N, 200, a_kmajor=True, b_kmajor=True, b_shift=shift, splits=2, seed=70)
        msg = p.mismatches(kernel)
        if msg:
            bad[shift] = msg
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# (f) second source and the reductions behind it
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2])
def test_f_second_source_and_the_weight_gradient_reduction(nsd, dev, kernel):
    """weight_grads' fused call at H = 256: M = 4 H rows in unit-major order, columns [0, H) meet h shifted inside blocks of T * 32 rows,
    columns [H, H + Kin) the layer's input unshifted, ldc = N.  Then seq_reduce_dw_kernel on the partials: part + 0 with I = H, part + H
    with I < Kin -- sums of exact partials, exact again, in torch's row order g * H + u."""
    from nsd_amd import _lib, ops
    H, Kin, I, T, splits = 256, 104, 100, 5, 3
    M, N, K = 4 * H, H + Kin, 2 * T * 32
    bad = {}
    for shift in (-32, 32):
        p = Problem(dev, M, N, K, a_kmajor=True, b_kmajor=True, b_shift=shift, b_period=T * 32, n_split=H, b2_off=8, ldb2=Kin + 16,
                    splits=splits, seed=80)
        msg = p.mismatches(kernel)
        if msg:
            bad[shift] = msg
            continue
        parts = p.c[:splits * M * N]
        with _lib.diagnostic_library():
            w_hh = ops.reduce_dw_diag(parts, splits, H, N, H)
            w_ih = ops.reduce_dw_diag(parts, splits, H, N, I, part_off=H)
        total = p.ref.sum(0).reshape(H, 4, N).transpose(1, 0, 2).reshape(4 * H, N).astype(np.float32)      # row 4u + g -> g * H + u
        for name, got, want in (("w_hh", w_hh, total[:, :H]), ("w_ih", w_ih, total[:, H:H + I])):
            got = got.cpu().numpy()
            if not np.array_equal(got, want):
                at = np.argwhere(got != want)
                bad[(shift, name)] = f"{len(at)} differ, first (row, i, got, want): {[(int(r), int(i), float(got[r, i]), float(want[r, i])) for r, i in at[:6]]}"
    assert not bad, bad


@pytest.mark.parametrize("H,nparts", [(64, 1), (256, 5), (72, 3)])
def test_f_bias_gradient_reduction(nsd, dev, H, nparts):
    """seq_reduce_db_kernel: the per-tile rows of the backward scan summed, unit-major 4u + g -> torch's g * H + u, into both biases"""
    from nsd_amd import _lib, ops
    part = gr.exact_operands((nparts, 4 * H), 90 + H, quantum=0.25)
    with _lib.diagnostic_library():
        b_ih, b_hh = ops.reduce_db_diag(torch.from_numpy(part).to(dev), nparts, H)
    want = part.astype(np.float64).sum(0).reshape(H, 4).T.reshape(-1).astype(np.float32)
    assert np.array_equal(b_ih.cpu().numpy(), want) and np.array_equal(b_hh.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# (g) epilogues
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2, 22, 23, 32])
@pytest.mark.parametrize("epilogue", [1, 2, 3])
def test_g_bf16_epilogues_round_ties_to_even(nsd, dev, kernel, epilogue):
    """bf16 [M][ldc], accumulator tiles + bias, wave-major tiles + bias against the reference rounded to nearest even.  At K = 200 the
    sums spread over +-300: a quarter of those in [64, 256) lie exactly between two bf16 numbers, some exceed 256 (bf16 steps of 2)."""
    M, N = ((197, 141) if kernel == 1 else (333, 285)) if epilogue == 1 else ((160, 96) if kernel == 1 else (320, 288))
    p = Problem(dev, M, N, 200, epilogue=epilogue, bias=epilogue > 1, ldc=N + 3 if epilogue == 1 else None, seed=100 + epilogue)
    exact = gr.gemm_ref(p.A, p.B, M=M, N=N, K=200)[0]
    if p.bias is not None:
        exact = exact + p.bias[:, None]
    exact = exact.astype(np.float32)
    assert gr.bf16_ties(exact) >= 1000 and np.count_nonzero(np.abs(exact) > 256) >= 10, (gr.bf16_ties(exact), np.abs(exact).max())
    p.check(kernel)


@pytest.mark.parametrize("kernel", [1, 2, 22, 23, 32])
def test_g_addend_on_the_fp32_epilogue(nsd, dev, kernel):
    """C = A . B + add[m][n] with C's leading dimension: the residual route's input gradient"""
    M, N = (197, 141) if kernel == 1 else (333, 285)
    p = Problem(dev, M, N, 136, add=True, ldc=N + 7, seed=110)
    assert not np.array_equal(p.ref, gr.gemm_ref(p.A, p.B, M=M, N=N, K=136))
    p.check(kernel)


# ---------------------------------------------------------------------------------------------------------------------------------
# (h) tile order of the 256 x 256 kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles_m,tiles_n", [(3, 5), (3, 6), (8, 2), (9, 2), (17, 2), (16, 2), (2, 9)])
def test_h_tile_order_is_complete(nsd, dev, tiles_m, tiles_n):
    """The workgroup order is invisible in the result: every variant must simply be complete and exact.  15 tiles: natural order;
    18 and 34: >= 16 and no multiple of 8 -- a padded grid, whole workgroups leave; tiles_m < 8, = 8, = 16 (whole groups), = 9 and 17
    (a last group of one M tile)."""
    M, N = (tiles_m - 1) * 256 + 77, (tiles_n - 1) * 256 + 141
    p = Problem(dev, M, N, 72, seed=120 + tiles_m)
    p.check(22)
    p.check(2)
    Problem(dev, M - 5, N - 5, 72, a_kmajor=True, b_kmajor=True, seed=121 + tiles_m).check(2)
