"""Any-loss backward and input gradients on the bf16 sequence path (nsd_seq_train_fwd_logits, nsd_seq_head_bwd,
nsd_seq_train_bwd_dx) without a GPU: symbols, refusals before any launch, an unchanged workspace size, the profile kinds."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nsd_seq_train_fwd_logits", "nsd_seq_head_bwd", "nsd_seq_train_bwd_dx"]
FAKE = 4096                     # never dereferenced: every call below is refused before anything is launched
E_INVALID, E_WS = -1, -3
BIDIR, RESIDUAL = 8, 1

# nsd_seq_workspace_bytes of the tree before these entry points: ((B, T, C, H, L, K, F), flags, bytes).  The new calls need
# no workspace of their own, so existing callers' workspaces keep working.
PINNED_WS = [
    ((48, 20, 8, 64, 2, 5, 32), 0, 80341760), ((48, 20, 8, 64, 2, 5, 32), 8, 83931904),
    ((48, 20, 8, 64, 2, 5, 32), 1, 80341760), ((48, 20, 8, 64, 2, 5, 32), 9, 85242624),
    ((48, 20, 8, 64, 2, 5, 32), 2, 80341760),
    ((33, 7, 8, 256, 2, 5, 32), 0, 85889280), ((33, 7, 8, 256, 2, 5, 32), 8, 96489728),
    ((33, 7, 8, 256, 2, 5, 32), 1, 85889280), ((33, 7, 8, 256, 2, 5, 32), 9, 98324736),
    ((33, 7, 8, 256, 2, 5, 32), 2, 85889280),
    ((1030, 3, 8, 256, 2, 5, 32), 0, 136161536), ((1030, 3, 8, 256, 2, 5, 32), 8, 198334720),
    ((1030, 3, 8, 256, 2, 5, 32), 1, 142846208), ((1030, 3, 8, 256, 2, 5, 32), 9, 211704064),
    ((1030, 3, 8, 256, 2, 5, 32), 2, 136161536),
    ((1024, 250, 8, 256, 2, 5, 32), 0, 3516363264), ((1024, 250, 8, 256, 2, 5, 32), 8, 5899686400),
    ((1024, 250, 8, 256, 2, 5, 32), 1, 3516363264), ((1024, 250, 8, 256, 2, 5, 32), 9, 6948262400),
    ((1024, 250, 8, 256, 2, 5, 32), 2, 3516363264),
    ((64, 1, 40, 128, 1, 3, 32), 0, 76683520), ((64, 1, 40, 128, 1, 3, 32), 8, 77836544),
    ((64, 1, 40, 128, 1, 3, 32), 1, 76749056), ((64, 1, 40, 128, 1, 3, 32), 9, 77967616),
    ((64, 1, 40, 128, 1, 3, 32), 2, 76683520),
    ((40, 5, 40, 64, 3, 4, 32), 0, 77404416), ((40, 5, 40, 64, 3, 4, 32), 8, 79516928),
    ((40, 5, 40, 64, 3, 4, 32), 1, 77568256), ((40, 5, 40, 64, 3, 4, 32), 9, 79844608),
    ((40, 5, 40, 64, 3, 4, 32), 2, 77404416),
    ((576, 64, 64, 512, 2, 5, 32), 0, 959587072), ((576, 64, 64, 512, 2, 5, 32), 8, 1846735616),
    ((576, 64, 64, 512, 2, 5, 32), 1, 1110582016), ((576, 64, 64, 512, 2, 5, 32), 9, 2148725504),
    ((576, 64, 64, 512, 2, 5, 32), 2, 959587072),
    ((512, 1000, 64, 512, 2, 5, 32), 0, 11724261888), ((512, 1000, 64, 512, 2, 5, 32), 8, 23311174144),
    ((512, 1000, 64, 512, 2, 5, 32), 1, 13821413888), ((512, 1000, 64, 512, 2, 5, 32), 9, 27505478144),
    ((512, 1000, 64, 512, 2, 5, 32), 2, 11724261888),
    ((32, 9, 100, 256, 3, 3, 16), 0, 85934848), ((32, 9, 100, 256, 3, 3, 16), 8, 100485888),
    ((32, 9, 100, 256, 3, 3, 16), 1, 86524672), ((32, 9, 100, 256, 3, 3, 16), 9, 101665536),
    ((32, 9, 100, 256, 3, 3, 16), 2, 85934848),
]


@pytest.fixture(scope="module")
def L():
    import nsd_amd
    nsd_amd.build_library()
    from nsd_amd import _lib
    return _lib


def test_new_symbols_are_declared_bound_and_exported(L):
    hdr = open(os.path.join(ROOT, "include", "nsd.h")).read()
    assert re.search(r"#define NSD_VERSION 301\b", hdr)
    lib = L.lib()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, hdr), s
        assert s in L.SYMBOLS, s
        assert hasattr(lib, s), s
    # the header documents both call sequences
    assert "nsd_seq_train_fwd -> nsd_seq_train_bwd[_dx]" in hdr
    assert "nsd_seq_train_fwd_logits -> (the caller forms dL/dlogits) -> nsd_seq_head_bwd -> nsd_seq_train_bwd[_dx]" in hdr


@pytest.mark.parametrize("dims,flags,nbytes", PINNED_WS)
def test_workspace_bytes_unchanged(L, dims, flags, nbytes):
    d = L.Dims(*dims)
    assert L.lib().nsd_seq_workspace_bytes(C.byref(d), flags) == nbytes


@pytest.mark.parametrize("flags", [0, BIDIR, RESIDUAL, BIDIR | RESIDUAL])
def test_refusals_before_any_launch(L, flags):
    lib = L.lib()
    d = L.Dims(33, 7, 40, 64, 3, 4, 32)
    need = lib.nsd_seq_workspace_bytes(C.byref(d), flags)
    assert need > 0
    ok_rng, bad_rng = L.Rng(1, 4, 0.5, 0.5), L.Rng(1, 4, 1.5, 0.5)
    # nsd_seq_train_fwd_logits(d, params, x, rng, flags, ws, bytes, logits, stream)
    fwd = lambda params=FAKE, x=FAKE, rng=None, fl=flags, ws=FAKE, nb=need, logits=FAKE: lib.nsd_seq_train_fwd_logits(
        C.byref(d), params, x, rng, fl, ws, nb, logits, None)
    assert fwd(x=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert fwd(logits=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert fwd(params=None) == E_INVALID
    assert fwd(ws=None) == E_INVALID
    assert fwd(fl=flags | (1 << 20)) == E_INVALID and b"unknown flag" in lib.nsd_last_error()
    assert fwd(nb=need - 256) == E_WS
    assert fwd(rng=C.byref(bad_rng)) == E_INVALID
    # nsd_seq_head_bwd(d, params, rng, dlogits, flags, ws, bytes, stream)
    hb = lambda params=FAKE, rng=None, dl=FAKE, fl=flags, ws=FAKE, nb=need: lib.nsd_seq_head_bwd(C.byref(d), params, rng, dl, fl, ws, nb, None)
    assert hb(dl=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert hb(params=None) == E_INVALID
    assert hb(fl=flags | (1 << 20)) == E_INVALID
    assert hb(nb=need - 256) == E_WS
    assert hb(rng=C.byref(bad_rng)) == E_INVALID
    # nsd_seq_train_bwd_dx(d, params, rng, flags, ws, bytes, grads, dx, stream)
    bw = lambda params=FAKE, rng=None, fl=flags, ws=FAKE, nb=need, grads=FAKE, dx=FAKE: lib.nsd_seq_train_bwd_dx(
        C.byref(d), params, rng, fl, ws, nb, grads, dx, None)
    assert bw(grads=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert bw(params=None) == E_INVALID
    assert bw(ws=None) == E_INVALID
    assert bw(fl=flags | (1 << 20)) == E_INVALID
    assert bw(nb=need - 256) == E_WS and b"smaller than nsd_seq_workspace_bytes" in lib.nsd_last_error()
    assert bw(nb=need - 256, dx=None) == E_WS
    assert bw(rng=C.byref(bad_rng)) == E_INVALID
    # nsd_seq_infer(d, params, x, flags, logits, probs, ws, bytes, stream)
    inf = lambda params=FAKE, x=FAKE, fl=flags, logits=FAKE, ws=FAKE, nb=need: lib.nsd_seq_infer(
        C.byref(d), params, x, fl, logits, None, ws, nb, None)
    assert inf(x=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert inf(logits=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert inf(params=None) == E_INVALID
    assert inf(ws=None) == E_INVALID
    assert inf(fl=flags | (1 << 20)) == E_INVALID and b"unknown flag" in lib.nsd_last_error()
    assert inf(nb=need - 256) == E_WS and b"smaller than nsd_seq_workspace_bytes" in lib.nsd_last_error()
    # nsd_seq_train_fwd(d, params, x, rng, labels, scale, flags, ws, bytes, logits, stream)
    tf = lambda params=FAKE, x=FAKE, rng=None, labels=FAKE, fl=flags, ws=FAKE, nb=need, logits=FAKE: lib.nsd_seq_train_fwd(
        C.byref(d), params, x, rng, labels, 1.0, fl, ws, nb, logits, None)
    assert tf(x=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert tf(logits=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert tf(labels=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert tf(params=None) == E_INVALID
    assert tf(ws=None) == E_INVALID
    assert tf(fl=flags | (1 << 20)) == E_INVALID and b"unknown flag" in lib.nsd_last_error()
    assert tf(nb=need - 256) == E_WS
    assert tf(rng=C.byref(bad_rng)) == E_INVALID and b"rng" in lib.nsd_last_error()
    # nsd_seq_train_bwd(d, params, rng, flags, ws, bytes, grads, stream)
    tb = lambda params=FAKE, rng=None, fl=flags, ws=FAKE, nb=need, grads=FAKE: lib.nsd_seq_train_bwd(
        C.byref(d), params, rng, fl, ws, nb, grads, None)
    assert tb(grads=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert tb(params=None) == E_INVALID
    assert tb(ws=None) == E_INVALID
    assert tb(fl=flags | (1 << 20)) == E_INVALID and b"unknown flag" in lib.nsd_last_error()
    assert tb(nb=need - 256) == E_WS
    assert tb(rng=C.byref(bad_rng)) == E_INVALID and b"rng" in lib.nsd_last_error()
    # nsd_seq_loss_sum(d, flags, ws, bytes, out, stream)
    ls = lambda fl=flags, ws=FAKE, nb=need, out=FAKE: lib.nsd_seq_loss_sum(C.byref(d), fl, ws, nb, out, None)
    assert ls(ws=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert ls(out=None) == E_INVALID and b"null" in lib.nsd_last_error()
    assert ls(fl=flags | (1 << 20)) == E_INVALID and b"unknown flag" in lib.nsd_last_error()
    assert ls(nb=need - 256) == E_WS
    # when two things are wrong at once, the earlier check answers: dims and flags, null workspace / params, workspace size, the
    # entry's own pointers, (empty batch), rng
    assert inf(nb=need - 256, x=None) == E_WS
    assert tf(nb=need - 256, labels=None, rng=C.byref(bad_rng)) == E_WS
    assert tb(nb=need - 256, grads=None) == E_WS
    assert ls(nb=need - 256, out=None) == E_INVALID         # (no parameters: its `out` is refused where the others' params are)
    assert tf(x=None, rng=C.byref(bad_rng)) == E_INVALID and b"null" in lib.nsd_last_error()
    assert tb(grads=None, rng=C.byref(bad_rng)) == E_INVALID and b"null" in lib.nsd_last_error()
    # an empty batch is a no-op that launches nothing: it returns before the rng is looked at
    d0 = L.Dims(0, 7, 40, 64, 3, 4, 32)
    need0 = lib.nsd_seq_workspace_bytes(C.byref(d0), flags)
    assert lib.nsd_seq_train_fwd_logits(C.byref(d0), FAKE, FAKE, C.byref(ok_rng), flags, FAKE, need0, FAKE, None) == 0
    assert lib.nsd_seq_head_bwd(C.byref(d0), FAKE, None, FAKE, flags, FAKE, need0, None) == 0
    assert lib.nsd_seq_train_bwd_dx(C.byref(d0), FAKE, None, flags, FAKE, need0, FAKE, FAKE, None) == 0
    assert lib.nsd_seq_infer(C.byref(d0), FAKE, FAKE, flags, FAKE, None, FAKE, need0, None) == 0
    assert lib.nsd_seq_train_fwd(C.byref(d0), FAKE, FAKE, C.byref(bad_rng), FAKE, 1.0, flags, FAKE, need0, FAKE, None) == 0
    assert lib.nsd_seq_train_bwd(C.byref(d0), FAKE, C.byref(bad_rng), flags, FAKE, need0, FAKE, None) == 0
    assert lib.nsd_seq_train_fwd_logits(C.byref(d0), FAKE, FAKE, C.byref(bad_rng), flags, FAKE, need0, FAKE, None) == 0
    assert lib.nsd_seq_head_bwd(C.byref(d0), FAKE, C.byref(bad_rng), FAKE, flags, FAKE, need0, None) == 0
    assert lib.nsd_seq_train_bwd_dx(C.byref(d0), FAKE, C.byref(bad_rng), flags, FAKE, need0, FAKE, FAKE, None) == 0


def test_profile_kinds_of_the_new_launches(L):
    """The dx contraction and the head backward from dlogits have timing kinds of their own in the diagnostic build."""
    from nsd_amd import ops
    assert ops.SEQ_PROFILE_KINDS[8:] == ("gemm_dx", "head_bwd")
    with L.diagnostic_library() as DL:
        ms, n = C.c_float(-1.0), C.c_int32(-1)
        for kind in (8, 9):
            assert DL.nsd_seq_profile_read(kind, C.byref(ms), C.byref(n)) == 0 and n.value == 0
        assert DL.nsd_seq_profile_read(10, C.byref(ms), C.byref(n)) == E_INVALID

