"""CPU-side checks of the ABI 32 additions for triplet attention at 65 <= N <= 128: the workspace query, the refusal
above 128, the ctypes mirror, and the numpy restatement of the dropout pattern (tests/triplet_kb_util.py)."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import triplet_kb_util as ku


def _args(B=2, N=80, H=4, D=16, dtype=1, flags=3):
    from tgt_amd import _lib
    a = _lib.TripletAttentionArgs()
    a.B, a.N, a.H, a.D, a.dtype, a.flags = B, N, H, D, dtype, flags
    return a


def _ws(bwd=1, **kw):
    from tgt_amd import _lib
    return _lib.lib().tgt_triplet_attention_workspace_bytes(C.byref(_args(**kw)), bwd)


def test_workspace_query():
    assert _ws(N=64) == 0 and _ws(N=64, bwd=0) == 0 and _ws(N=1) == 0
    for N in (65, 80, 128):
        n = _ws(N=N)
        assert n > 0 and n % 16 == 0, (N, n)
        assert _ws(N=N, bwd=0) >= 0 and _ws(N=N, bwd=0) % 16 == 0
        for dtype in (0, 1, 2):
            assert _ws(N=N, dtype=dtype) > 0
        assert _ws(N=N, B=3) > _ws(N=N, B=2) > _ws(N=N, B=1)
        assert _ws(N=N, H=8) > _ws(N=N, H=4) > _ws(N=N, H=3)
    assert _ws(N=128) >= _ws(N=65)
    assert _ws(N=129) < 0
    assert _ws(N=80, D=8) < 0
    assert _ws(N=1000, bwd=0) < 0


def test_refusal_above_128_names_the_limit():
    from tgt_amd import _lib
    L = _lib.lib()
    a = _args(N=129)
    assert L.tgt_triplet_attention_fwd(C.byref(a), None) == 2          # TGT_ERR_UNSUPPORTED, before any tensor is looked at
    assert b'128' in L.tgt_last_error()
    assert L.tgt_triplet_attention_bwd(C.byref(a), None) == 2
    assert b'128' in L.tgt_last_error()


def test_binding_mirrors_the_new_fields():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32
    assert _lib.lib().tgt_abi_version() == 32
    names = [f[0] for f in _lib.TripletAttentionArgs._fields_]
    assert names[-2:] == ['workspace', 'workspace_bytes']
    TA = _lib.TripletAttentionArgs
    assert TA.workspace.offset + 16 == C.sizeof(TA) and TA.workspace_bytes.size == 8


@pytest.mark.parametrize('N', [1, 7, 32, 48, 64])
def test_dropout_restatement_matches_the_existing_one_up_to_64(N):
    units = np.array([0, 3, 1000, 2 ** 20 + 5])
    for p in (0.1, 0.3):
        want, s0 = gu.triplet_dropout_keep(0x1234567890ABCDEF, p, units, N)
        got, s1 = ku.triplet_dropout_keep(0x1234567890ABCDEF, p, units, N)
        assert s0 == s1 and np.array_equal(got, want)


@pytest.mark.parametrize('N', [65, 80, 128])
def test_dropout_fields_do_not_alias_above_64(N):
    f = ku.dropout_field_index(N)
    assert np.unique(f).size == N * N                       # every (i, k) of a unit draws from its own 16-bit field
    old = ((np.arange(N)[:, None] * 64 + np.arange(N)[None, :]) >> 1) * 2 + (np.arange(N)[None, :] & 1)
    assert np.unique(old).size < N * N                      # (the stride of 64 is what aliased)
    keep, _ = ku.triplet_dropout_keep(7, 0.3, np.arange(8), N)
    assert abs(keep.mean() - 0.7) < 0.02
