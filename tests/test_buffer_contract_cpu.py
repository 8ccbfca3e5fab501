"""tests/buffer_contract.py has teeth: on CPU tensors (no GPU) a write one element before or after a guarded payload is reported with its
side, a write inside it is not, payloads are 256-byte aligned, every fill has the bits it states, a stale payload keeps what the earlier
user left at the same address, and a one-bit flip of an input is seen."""
import numpy as np
import pytest
import torch

from tests import buffer_contract as bc

CPU = torch.device("cpu")
SHAPES = [((5, 3), torch.float32), ((7,), torch.float32), ((1,), torch.float32), ((3, 9, 5), torch.bfloat16), ((4099,), torch.uint8),
          ((2, 3000), torch.float32), ((6,), torch.int32)]


def _halves(t):
    return t.contiguous().view(-1).view(torch.uint8).numpy().view(np.uint16)


def _outside(g, nbytes_from_start):
    """the byte of the allocation at that offset from the payload's first byte"""
    return g.store[g.off + nbytes_from_start:g.off + nbytes_from_start + 1]


@pytest.mark.parametrize("shape,dtype", SHAPES)
def test_a_write_outside_the_payload_is_reported_with_its_side(shape, dtype):
    es = torch.empty(0, dtype=dtype).element_size()
    for side, at in (("before", -es), ("after", None)):
        g = bc.Guarded(shape, dtype, CPU, "zeros")
        assert g.violation() is None
        g.check()
        at = g.nbytes if at is None else at                # one element before the first / right after the last
        _outside(g, at).fill_(0)
        assert g.violation() == (side, at)
        with pytest.raises(AssertionError, match=f"{side} it"):
            g.check("probe")
    # the far ends of both guards are watched too
    for side, at in (("before", -g.guard), ("after", g.nbytes + g.guard - 1)):
        g = bc.Guarded(shape, dtype, CPU, "ones")
        _outside(g, at).fill_(0x5A)
        assert g.violation() == (side, at)


@pytest.mark.parametrize("shape,dtype", SHAPES)
def test_writes_inside_the_payload_are_not_reported(shape, dtype):
    payload, check = bc.guarded(shape, dtype, CPU, "nan32")
    assert tuple(payload.shape) == shape and payload.dtype == dtype and payload.is_contiguous()
    payload.view(-1)[0] = 1
    payload.view(-1)[-1] = 1
    payload.fill_(3)
    check()


@pytest.mark.parametrize("shape,dtype", SHAPES)
def test_payload_alignment_and_guard_size(shape, dtype):
    g = bc.Guarded(shape, dtype, CPU, "zeros")
    assert g.payload.data_ptr() % 256 == 0
    row = g.nbytes // shape[0]
    assert g.guard % 256 == 0 and g.guard >= max(4096, row) and g.guard < max(4096, row) + 256
    assert bool((g.store[g.off - g.guard:g.off] == 0xA5).all()) and bool((g.store[g.off + g.nbytes:g.off + g.nbytes + g.guard] == 0xA5).all())
    assert g.off - g.guard >= 0 and g.off + g.nbytes + g.guard <= g.store.numel()


def test_fills_have_the_stated_bits():
    n = 1024
    z = _halves(bc.guarded((n,), torch.float32, CPU, "zeros")[0])
    assert z.size == 2 * n and not z.any() and not (z & 0x4000).any()              # tag bit (bit 14) clear in every half
    one = bc.guarded((n,), torch.float32, CPU, "ones")[0]
    h = _halves(one)
    assert (h == 0xFFFF).all() and (h & 0x4000).all()
    assert bool(torch.isnan(one).all()) and bool(torch.isnan(one.view(torch.bfloat16)).all())
    nan = bc.guarded((n,), torch.float32, CPU, "nan32")[0]
    h = _halves(nan)
    assert (nan.view(torch.int32) == 0x7FC00000).all() and bool(torch.isnan(nan).all())
    lo, hi = h[0::2], h[1::2]                                                     # little-endian: the low half comes first
    assert (lo == 0).all() and (hi == 0x7FC0).all() and (hi & 0x4000).all()
    halves = nan.view(torch.bfloat16)
    assert bool(torch.isnan(halves[1::2]).all()) and bool((halves[0::2] == 0).all())
    odd = bc.guarded((3, 7), torch.bfloat16, CPU, "nan32")[0]                     # 42 bytes: ten words and the first two bytes of one
    assert (_halves(odd)[0::2] == 0).all() and (_halves(odd)[1::2] == 0x7FC0).all()
    with pytest.raises(ValueError):
        bc.guarded((4,), torch.float32, CPU, "fives")
    with pytest.raises(ValueError):
        bc.guarded((4,), torch.float32, CPU, "stale")                             # stale content needs an earlier user


def test_stale_takes_over_the_allocation_of_a_larger_evaluation():
    big = bc.Arena(CPU, "zeros")
    b = big.buf("logits", (8, 5))
    b.copy_(torch.arange(40, dtype=torch.float32).view(8, 5))
    assert big.buf("logits", (8, 5)) is b                                          # a second request: the same buffer, untouched
    small = bc.Arena(CPU, "stale", prior=big)
    s = small.buf("logits", (5, 5))
    assert s.data_ptr() == b.data_ptr() and torch.equal(s.view(-1), torch.arange(25, dtype=torch.float32))
    g = small.bufs["logits"]
    assert bool((g.store[g.off + g.nbytes:g.off + g.nbytes + g.guard] == 0xA5).all())   # the larger payload's tail is guard now
    small.check()
    b[5, 0] = 1.0                                                                 # row 5 of the larger shape: past the smaller payload
    with pytest.raises(AssertionError, match="logits.*after it"):
        small.check()
    with pytest.raises(ValueError, match="does not fit"):
        bc.Guarded((64, 5), torch.float32, CPU, "stale", within=big.bufs["logits"])
    with pytest.raises(KeyError):
        small.buf("grads", (3,))


def test_unchanged_sees_a_one_bit_flip():
    x = torch.randn(3, 4, 5)
    y = torch.arange(7, dtype=torch.int32)
    w = torch.randn(6).to(torch.bfloat16)
    snap = bc.snapshot(x, None, y, w)
    assert snap.unchanged() and snap.changed() == []
    x.view(torch.int32)[1, 2, 3] ^= 1                                              # the lowest mantissa bit of one element
    assert not snap.unchanged() and snap.changed() == [0]
    x.view(torch.int32)[1, 2, 3] ^= 1
    assert snap.unchanged()
    y[6] ^= 1 << 30
    w.view(torch.int16)[0] ^= 1
    assert snap.changed() == [1, 2]
    z = torch.zeros(4)
    s0 = bc.snapshot(z)
    z[2] = -0.0                                                                    # equal as a number, another bit pattern
    assert not s0.unchanged()


def test_exact_sizes_are_the_librarys_own():
    import ctypes as C
    import nsd_amd
    from nsd_amd import _lib, ops
    L = nsd_amd.load_library()
    spec = ops.ModelSpec(C=8, H=48, L=2, K=5, F=24)
    d, w = spec.dims(5, 9), _lib.WsLayout()
    assert bc.workspace_bytes(spec, 5, 9) == L.nsd_workspace_bytes(C.byref(d), C.byref(w)) == 4 * w.total
    assert bc.multi_workspace_bytes(spec, 3, 5, 9) == L.nsd_multi_workspace_bytes(C.byref(d), 3, C.byref(w)) == 4 * w.total
    assert bc.infer_scratch_bytes(spec, 5, 9) == L.nsd_infer_scratch_bytes(C.byref(d))
    assert bc.multi_infer_scratch_bytes(spec, 3, 5, 9) == L.nsd_multi_infer_scratch_bytes(C.byref(d), 3)
    seq = ops.ModelSpec(C=8, H=64, L=2, K=5)
    ds = seq.dims(33, 2)
    assert bc.seq_workspace_bytes(seq, 33, 2) == L.nsd_seq_workspace_bytes(C.byref(ds), 0) > 0
    assert spec.param_count == 31398 and ops.ModelSpec(C=8, H=48, L=2, K=4, F=24).param_count == 31373   # the GPU file's model-batched heads
