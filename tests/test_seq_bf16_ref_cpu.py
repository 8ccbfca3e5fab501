"""Host-only tests of the float64 bf16-path emulation (oracle/seq_bf16_ref.py), the checker of tests/test_gpu_seqpath_bf16ref.py:
its rounding helper, its agreement with the fp32 oracles when its rounding points are off, and that the GPU bounds resolve both the
roundings and a set of plausible kernel bugs (mutants) at the GPU tests' own shapes.  Nothing here launches a GPU kernel."""
import numpy as np
import pytest
import torch

from oracle import nsd_oracle as orc
from oracle import seq_bf16_ref as sr
from tests import seq_bf16_harness as gp
from tests.golden.make_goldens import BIDIR_CASES, synth_labels, synth_params, synth_x


def _worst(errs):
    return max((v, k) for k, v in errs.items() if k != "attn.bias")


# ---------------------------------------------------------------------------------------------------------------------------
def test_bf16_rounding_is_bit_identical_to_torch():
    rs = np.random.RandomState(0)
    vals = [rs.standard_normal(100000).astype(np.float32) * np.float32(10.0) ** rs.randint(-30, 30, 100000).astype(np.float32),
            rs.standard_normal(1000).astype(np.float32)]
    # exact ties (low 16 bits 0x8000, both parities of the kept bit), one ulp either side of a tie
    hi = (rs.randint(0, 0x7F7F, 4000).astype(np.uint32) << 16) | np.where(rs.rand(4000) < 0.5, 0x80000000, 0).astype(np.uint32)
    for low in (0x8000, 0x7FFF, 0x8001, 0x0000, 0xFFFF):
        vals.append((hi | np.uint32(low)).view(np.float32))
    vals.append(np.array([0.0, -0.0, np.inf, -np.inf, np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny,
                          1e-45, -1e-45, 3e-39, -3e-39, 3.3895314e38, 1.0, -1.0, 0.5, 65504.0], np.float32))
    a = torch.from_numpy(np.concatenate(vals))
    got = sr.bf16_round_f32(a)
    want = a.to(torch.bfloat16).to(torch.float32)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    nan = torch.tensor([float("nan"), -float("nan")], dtype=torch.float32)
    assert torch.isnan(sr.bf16_round_f32(nan)).all()


def test_param_layout_is_the_product_layout():
    from nsd_amd import ops
    for (C, H, L, K, D) in ((8, 64, 2, 5, 1), (24, 128, 3, 3, 2), (64, 512, 2, 5, 2)):
        spec = ops.ModelSpec(C=C, H=H, L=L, K=K, D=D)
        lo = sr.param_layout(C, H, L, K, 32, D)
        assert list(lo) == spec.names()
        assert {k: v[0] for k, v in lo.items()} == spec.offsets()
        assert sr.param_count(C, H, L, K, 32, D) == spec.param_count


# ---------------------------------------------------------------------------------------------------------------------------
# rounding points off: the fp64 model itself, against the fp32 C oracle / float64 torch / the bidirectional goldens
ORACLE_TOL = 5e-6          # of each tensor's largest element: the fp32 oracle's own error (measured <= 2.3e-6 at L = 3)


@pytest.mark.parametrize("C,H,L,streams", [(8, 64, 1, False), (8, 64, 2, False), (8, 64, 2, True), (40, 64, 2, False),
                                           (40, 128, 2, True), (8, 64, 3, False), (8, 64, 3, True), (40, 64, 1, False)])
def test_unrounded_emulation_equals_the_fp32_oracle(C, H, L, streams):
    K, B, T = 5, 19, 11
    d = orc.Dims(C=C, H=H, L=L, K=K)
    flat = orc.flatten_state(synth_params(C, H, L, K, seed=H + L + C), d)
    x, y = synth_x(B, T, C=C, seed=L), synth_labels(B, K, seed=L)
    kw = {}
    if streams:
        kw = dict(drop_lstm=orc.dropout_mask(11, 4, 0.4, (L - 1, B, T, H)), rrelu_slope=orc.rrelu_noise(11, 5, (B, 32)),
                  drop_head=orc.dropout_mask(11, 6, 0.4, (B, 32)))
    loss, g, fw = orc.loss_and_grads(flat, x, y, d, **kw)
    ev = orc.forward(flat, x, d)
    for route in (("fused2", "general") if L == 2 else ("general",)):
        r = sr.seq_bf16_ref(flat, x, y, C=C, H=H, L=L, K=K, route=route, rounding=False, **kw)
        assert np.abs(r["logits"] - fw["logits"]).max() < 1e-5
        assert np.abs(r["probs"] - fw["probs"]).max() < 1e-5 and abs(r["loss"] - loss) < 1e-5
        worst = _worst(sr.rel_errors(r["grads"], g, C, H, L, K))
        assert worst[0] < ORACLE_TOL, (route, worst)
        e = sr.seq_bf16_ref(flat, x, None, C=C, H=H, L=L, K=K, route=route, rounding=False)
        assert np.abs(e["logits"] - ev["logits"]).max() < 1e-5 and "grads" not in e


@pytest.mark.parametrize("tag", sorted(BIDIR_CASES))
def test_unrounded_bidirectional_emulation_equals_torch(golden, tag):
    """the bidirectional goldens (stock nn.LSTM, fp32) and a float64 torch composition with dropout / RReLU tensors"""
    from oracle.torch_ref import TorchRefEEG
    C, H, L, K, B, T = BIDIR_CASES[tag]
    ext = golden("extensions")
    st = synth_params(C, H, L, K, seed=70 + H, D=2)
    flat = np.concatenate([st[k].ravel() for k in sr.param_layout(C, H, L, K, 32, 2)])
    x, y = synth_x(B, T, C=C, seed=60), synth_labels(B, K=K, seed=60)
    r = sr.seq_bf16_ref(flat, x, y, C=C, H=H, L=L, K=K, D=2, route="general", rounding=False)
    assert np.abs(r["logits"] - ext[f"{tag}.logits"]).max() < 2e-5
    assert abs(r["loss"] - float(ext[f"{tag}.loss"])) < 2e-5
    g = sr.unflatten(r["grads"], C, H, L, K, 32, 2)
    for k in g:
        if f"{tag}.grad.{k}" in ext.files:
            ref = ext[f"{tag}.grad.{k}"]
            assert np.abs(g[k] - ref).max() <= 2e-5 * max(np.abs(ref).max(), 1e-6) + 1e-7, (tag, k)
    # float64 torch with the three stream tensors
    masks = dict(drop_lstm=orc.dropout_mask(5, 1, 0.4, (L - 1, B, T, 2 * H)) if L > 1 else None,
                 rrelu_slope=orc.rrelu_noise(5, 2, (B, 32)), drop_head=orc.dropout_mask(5, 3, 0.4, (B, 32)))
    m = TorchRefEEG(C, H, L, K, bidirectional=True).double()
    m.load_reference_state({k: torch.from_numpy(v).double() for k, v in st.items()})
    tm = {k: (torch.from_numpy(v).double() if v is not None else None) for k, v in masks.items()}
    lg = m(torch.from_numpy(x).double(), tm["drop_lstm"], tm["rrelu_slope"], tm["drop_head"])
    torch.nn.functional.cross_entropy(lg, torch.from_numpy(y.astype(np.int64))).backward()
    r = sr.seq_bf16_ref(flat, x, y, C=C, H=H, L=L, K=K, D=2, route="general", rounding=False, **masks)
    assert np.abs(r["logits"] - lg.detach().numpy()).max() < 1e-9
    g = sr.unflatten(r["grads"], C, H, L, K, 32, 2)
    for k, v in m.reference_named_grads().items():
        ref = v.numpy()
        assert np.abs(g[k] - ref).max() <= 1e-9 * max(np.abs(ref).max(), 1e-6), k


# ---------------------------------------------------------------------------------------------------------------------------
# the bounds resolve the roundings and the mutants, at the GPU tests' shapes
SMALL_CASES = [k for k in sorted(gp.CASES) if k not in ("cfg5_t64", "tiles64_h256")]


def _effect(case, ref, other):
    """(ratio to the GPU bounds, what): the larger of the worst gradient tensor's change over the gradient bound and the logit change
    over the logit bound"""
    C, H, L, K, D = case[:5]
    gw = _worst(sr.rel_errors(other["grads"], ref["grads"], C, H, L, K, 32, D))
    lw = float(np.abs(other["logits"] - ref["logits"]).max())
    gr, lr = gw[0] / gp.bound_of(case[9]), lw / gp.REF_LOGIT_TOL
    return (gr, gw[1]) if gr >= lr else (lr, "logits")


@pytest.mark.parametrize("tag", SMALL_CASES)
def test_rounding_effect_in_units_of_the_gpu_bounds(tag):
    """The emulation with its rounding points on against the fp64 model (the fp32 oracles' stand-in at the oracle's own level: test
    above), in units of the GPU bounds.  Measured: 0.8 .. 4.1x -- away from the RReLU kink the roundings move these shapes by about
    what the kernels' fp32-order noise moves them (0.1 %), so the bounds resolve the roundings as a whole, not 10x over; the wrong
    terms of the mutants below are what they do resolve.  Asserted: the roundings are on (>= 0.5x)."""
    case = gp.CASES[tag]
    flat, x, y, masks, _ = gp.case_inputs(case)
    C, H, L, K, D = case[:5]
    ref = sr.seq_bf16_ref(flat, x, y, C=C, H=H, L=L, K=K, D=D, route=case[8], **masks)
    unr = sr.seq_bf16_ref(flat, x, y, C=C, H=H, L=L, K=K, D=D, route=case[8], rounding=False, **masks)
    ratio, what = _effect(case, ref, unr)
    print(f"[{tag}] rounded vs unrounded: {ratio:.1f} x the bound ({what})")
    assert ratio >= ROUNDING_RESOLVED, (tag, ratio, what)


ROUNDING_RESOLVED = 0.5

# mutant -> the GPU case it is shown at (dropout / bidirectional where the mutant needs them)
MUTANT_CASES = {"dwhh_first_step": ["fused_h64", "general_l1", "bidir_h128"],
                "stale_member": ["fused_h128", "general_l1", "bidir_h128"],
                "forget_c_edge": ["fused_h64", "general_l3", "bidir_h128"],
                "reverse_init": ["bidir_h128"],
                "dscore_last": ["short_128_1_3"],      # (at T >= 20 the last step's score term is < 1x the bound)
                "keep_bit_lost": ["streams_h64", "general_l3", "bidir_h128"]}
MUTANT_TEETH = 3.0


def _case(tag):
    """a GPU case by name; short_<H>_<L>_<T>: the shapes of test_very_short_sequences_match_bf16_emulation_twice"""
    if tag.startswith("short_"):
        H, L, T = map(int, tag.split("_")[1:])
        return (8, H, L, 3, 1, 150, T, None, "fused2" if L == 2 else "general", "short", False)
    return gp.CASES[tag]


@pytest.mark.parametrize("mutant,tag", [(m, t) for m, ts in MUTANT_CASES.items() for t in ts])
def test_mutants_have_teeth(mutant, tag):
    case = _case(tag)
    flat, x, y, masks, _ = gp.case_inputs(case)
    C, H, L, K, D = case[:5]
    kw = dict(C=C, H=H, L=L, K=K, D=D, route=case[8], **masks)
    ref = sr.seq_bf16_ref(flat, x, y, **kw)
    mut = sr.seq_bf16_ref(flat, x, y, mutants=(mutant,), **kw)
    ratio, what = _effect(case, ref, mut)
    print(f"[{mutant} @ {tag}] {ratio:.1f} x the bound ({what})")
    assert ratio >= MUTANT_TEETH, (mutant, tag, ratio, what)


def test_rounding_point_sensitivity_table():
    """For the record: what removing / moving each rounding point does, in units of the GPU bounds, at two GPU shapes
    (fused streams, general bidirectional streams).  A point below 1 is invisible to the suite."""
    rows = []
    for tag in ("fused_l2_streams", "bidir_h128", "wide_c80"):
        case = gp.CASES[tag]
        flat, x, y, masks, _ = gp.case_inputs(case)
        C, H, L, K, D = case[:5]
        kw = dict(C=C, H=H, L=L, K=K, D=D, route=case[8], **masks)
        ref = sr.seq_bf16_ref(flat, x, y, **kw)
        for pt in sr.ROUNDING_POINTS:
            rows.append((tag, f"{pt} off", *_effect(case, ref, sr.seq_bf16_ref(flat, x, y, rounding_off=(pt,), **kw))))
        for mv in ("psum_once", "lk_unrounded_h"):
            rows.append((tag, mv, *_effect(case, ref, sr.seq_bf16_ref(flat, x, y, mutants=(mv,), **kw))))
    for r in rows:
        print(f"  {r[0]:18s} {r[1]:16s} {r[2]:8.2f} x bound  ({r[3]})")
    vis = {(r[0], r[1]): r[2] for r in rows}
    for tag in ("fused_l2_streams", "bidir_h128", "wide_c80"):
        assert vis[(tag, "w off")] > 1.0, tag                          # (measured 1.4 .. 2.3x; most single points sit below 1x)
