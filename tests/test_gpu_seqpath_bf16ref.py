"""The bf16 sequence path (BASELINE cfg3 / cfg5) against a float64 emulation of the SAME operation (oracle/seq_bf16_ref.py): it
rounds to bf16 exactly where the kernels round, so what is left is fp32 accumulation order, transcendental ulps and the rare
bf16 rounding flip those cause.  Needs a real MI355X: run with `pytest -m gpu -s` (every comparison prints its worst errors).

The fp32-oracle comparisons in tests/test_gpu_seqpath.py check the path against the model (bounds of percents: the precision
gap); these check the arithmetic, at bounds about 1/10 of those and below.  The CPU tests (tests/test_seq_bf16_ref_cpu.py) pin
the emulation to the fp32 oracle with its rounding points off and show that each mutant in oracle.seq_bf16_ref.MUTANTS moves a
result at these shapes by several times the bounds below.

Synthetic parameters get fc.0.bias = +-4 (kink_safe): no fc.0 pre-activation lies near the RReLU kink, where a bf16-sized change
flips the slope -- a property of the data, not of the kernel -- and every test asserts that margin on the emulation's values.
Bounds, cases and the machinery of a comparison: tests/seq_bf16_harness.py.
"""
import numpy as np
import pytest

from tests.gpu_harness import dev, nsd  # noqa: F401  (fixtures)
from tests.seq_bf16_harness import CASES, CFG3_FULL, CFG5_LONG, SHORT_SHAPES, SHORT_T, case_inputs, check_case, compare, emulate, run_gpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", sorted(CASES))
def test_seq_path_matches_bf16_emulation(nsd, dev, tag):
    check_case(tag, CASES[tag], dev)


@pytest.mark.parametrize("T", SHORT_T)
@pytest.mark.parametrize("H,L", SHORT_SHAPES)
def test_very_short_sequences_match_bf16_emulation_twice(nsd, dev, H, L, T):
    """T = 1 .. 5, two rounds on ONE workspace (the second finds the first one's granules in the rings): each against the emulation,
    and bitwise equal to each other"""
    import torch
    case = (8, H, L, 3, 1, 150, T, None, "fused2" if L == 2 else "general", "short", False)
    flat, x, y, masks, rng = case_inputs(case)
    ref = emulate(case, flat, x, y, masks)
    ws, first = None, None
    for rep in range(2):
        out = run_gpu(case, flat, x, y, rng, dev, ws)
        ws = out["ws"]
        compare(f"H{H} L{L} T{T} round {rep}", case, out["logits"], out["grads"], ref, got_loss=out["loss"])
        compare(f"H{H} L{L} T{T} round {rep} infer", case, out["infer"], None, ref, got_probs=out["probs"])
        if first is None:
            first = out
        else:
            for k in ("logits", "grads", "infer"):
                assert np.array_equal(first[k], out[k]), k
    torch.cuda.synchronize()


@pytest.mark.timeout(900)
def test_cfg5_kernels_thousand_steps_match_bf16_emulation(nsd, dev):
    """cfg5's kernels (C = 64, H = 512, bidirectional) over T = 1000 steps at 192 trials: the emulation takes 63 s on 16 threads"""
    check_case("cfg5 T1000", CFG5_LONG, dev)


@pytest.mark.timeout(900)
def test_cfg3_full_size_matches_bf16_emulation(nsd, dev):
    """cfg3 at its full size, B = 1024 x T = 250, one direct comparison: the emulation takes 22 s on 16 threads"""
    check_case("cfg3 full", CFG3_FULL, dev)
