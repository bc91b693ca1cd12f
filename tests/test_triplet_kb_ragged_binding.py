"""CPU-side checks of TGT_TRI_COUNTS_KB (include/tgt_hip.h: the key-blocked triplet attention kernels for 65..128 nodes use the
per-graph node counts): the flag constant and the TGT_TRI_RAGGED_KB knob exist and agree with the header; with the bit set the
entry points refuse what they refuse without it, in the same order and with the same codes, before anything is launched; the
workspace size does not depend on the bit.  And the premise the skip rests on, on the float64 oracle: a padded ROW is as safe
to skip as a padded column."""
import ctypes as C
import os
import re

import pytest
import torch

import golden_util as gu
from oracle import core

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'tgt_hip.h')


def test_flag_and_knob_exist_and_agree_with_the_header():
    from tgt_amd import _lib, knobs, ops
    with open(HEADER) as fh:
        text = fh.read()
    flags = {k: int(v) for k, v in re.findall(r'^\s*(TGT_TRI_\w+)\s*=\s*(\d+),', text, re.M)}
    assert flags['TGT_TRI_COUNTS_KB'] == _lib.TRI_COUNTS_KB == 16
    assert flags['TGT_TRI_NO_QKV_STORE'] == _lib.TRI_NO_QKV_STORE == 8
    assert sorted(flags.values()) == [1, 2, 4, 8, 16]                   # one bit each
    assert knobs._SPEC['tri_ragged_kb'][:3] == ('TGT_TRI_RAGGED_KB', False, 'flag')
    assert knobs._read('TGT_TRI_RAGGED_KB_never_set', False, 'flag') is False
    assert ops._TRI_RAGGED_KB == knobs.K.tri_ragged_kb
    assert _lib.ABI_VERSION == 32 and C.sizeof(_lib.TripletAttentionArgs) == 312        # ABI number and argument struct unchanged


def _args(flags=3, **kw):
    from tgt_amd import _lib
    a = _lib.TripletAttentionArgs()
    a.B, a.N, a.H, a.D, a.dtype, a.flags, a.scale = 2, 72, 4, 16, _lib.TGT_BF16, flags, 0.25
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _fill(a, n=16):
    """every tensor pointer set to an aligned HOST address: enough to pass the null / alignment checks -- a launch would fault
    on it, so every block below must be refused before one"""
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 15) & ~15
    a._keep = buf
    a.qkv[0] = a.qkv[1] = a.eg[0] = a.eg[1] = a.mask = a.out = p
    a.d_out = a.d_qkv[0] = a.d_qkv[1] = a.d_eg[0] = a.d_eg[1] = p
    a.ld_qkv[0] = a.ld_qkv[1] = a.ld_eg[0] = a.ld_eg[1] = 400
    a.ld_out = 128
    return a


def _refusals():
    """argument blocks the entry points refuse, in the order the checks come: (what, block, backward only)"""
    from tgt_amd import _lib
    p8 = C.cast((C.c_float * 16)(), C.c_void_p)
    return [
        ('bad sizes', _args(H=0), False),
        ('more than 128 nodes', _args(N=129), False),
        ('dropout_p', _args(dropout_p=1.5), False),
        ('null tensors', _args(), False),
        ('head width', _fill(_args(D=8)), False),
        ('column sums', _fill(_args(d_qkv_colsum=(C.c_void_p * 2)(p8.value, p8.value), d_eg_colsum=(C.c_void_p * 2)(p8.value, p8.value))), True),
        ('no workspace', _fill(_args()), True),
        ('workspace too small', _fill(_args(workspace=p8.value & ~15, workspace_bytes=64)), True),
    ]


def test_refusals_do_not_depend_on_the_bit():
    """same code and same message with TGT_TRI_COUNTS_KB set and clear, with and without a counts pointer (a host address that is
    never looked at); nothing is launched"""
    from tgt_amd import _lib
    L = _lib.lib()
    counts = C.cast((C.c_int32 * 4)(), C.c_void_p)
    null = C.POINTER(_lib.TripletAttentionArgs)()
    for fn in (L.tgt_triplet_attention_fwd_counts, L.tgt_triplet_attention_bwd_counts):
        assert fn(null, counts, None) == 1 and b'null args' in L.tgt_last_error()
    seen = []
    for what, a, bwd_only in _refusals():
        for name in ('tgt_triplet_attention_fwd_counts', 'tgt_triplet_attention_bwd_counts'):
            if bwd_only and 'fwd' in name:
                continue
            got = []
            for bit in (0, _lib.TRI_COUNTS_KB):
                for nc in (None, counts):
                    base = a.flags
                    a.flags = base | bit
                    code = getattr(L, name)(C.byref(a), nc, None)
                    got.append((code, L.tgt_last_error()))
                    a.flags = base
            assert got[0][0] in (1, 2), (what, name, got[0])            # TGT_ERR_INVALID / TGT_ERR_UNSUPPORTED: refused
            assert all(g == got[0] for g in got), (what, name, got)
            seen.append((what, name, got[0][0]))
    codes = {(w, n[-10:]): c for w, n, c in seen}
    assert codes[('more than 128 nodes', 'fwd_counts')] == 2 and codes[('head width', 'fwd_counts')] == 2
    assert codes[('column sums', 'bwd_counts')] == 2 and codes[('no workspace', 'bwd_counts')] == 1


def test_workspace_bytes_do_not_depend_on_the_bit():
    from tgt_amd import _lib
    L = _lib.lib()
    for N in (64, 65, 72, 100, 128, 129):
        for bwd in (0, 1):
            want = L.tgt_triplet_attention_workspace_bytes(C.byref(_args(N=N)), bwd)
            assert L.tgt_triplet_attention_workspace_bytes(C.byref(_args(N=N, flags=3 | _lib.TRI_COUNTS_KB)), bwd) == want
    assert L.tgt_triplet_attention_workspace_bytes(C.byref(_args(N=72, flags=3 | _lib.TRI_COUNTS_KB)), 1) == 2 * 2 * 4 * 72 * 3 * 96 * 4


@pytest.mark.parametrize('variant', ['gated', 'ungated', 'axial'])
def test_padded_rows_are_as_safe_to_skip_as_padded_columns(variant):
    """float64 oracle, N = 9, counts [9, 4, 1], prefix masks: with a cotangent that is zero at every padded row and column,
    other finite values at every padded position of the inputs leave the real block of the output and every gradient on it
    bit-equal, and the gradient at every padded position is exactly 0"""
    N, counts, C_, H = 9, [9, 4, 1], 8, 2
    B = len(counts)
    gated, biased = variant == 'gated', variant != 'axial'
    g = torch.Generator().manual_seed(9)
    mask = gu.additive_mask(counts, N, torch.float64)
    nm = torch.arange(N)[None, :] < torch.tensor(counts)[:, None]
    real = (nm[:, :, None] & nm[:, None, :]).unsqueeze(-1)                # (B,N,N,1)
    widths = [3 * C_, (2 if gated else 1) * H, 3 * C_, (2 if gated else 1) * H]
    base = [torch.randn(B, N, N, w, generator=g, dtype=torch.float64) for w in widths]
    other = [torch.where(real, t, 3.0 * torch.randn(B, N, N, t.shape[-1], generator=g, dtype=torch.float64) + 1.0) for t in base]
    d_out = torch.randn(B, N, N, 2 * C_, generator=g, dtype=torch.float64) * real

    def run(ins):
        ins = [t.clone().requires_grad_(True) for t in ins]
        out = core.triplet_attention_core(ins[0], ins[1] if biased else None, ins[2], ins[3] if biased else None, mask, H, gated, biased)
        out.backward(d_out)
        return out.detach(), [t.grad for t in (ins if biased else (ins[0], ins[2]))]
    out0, grads0 = run(base)
    out1, grads1 = run(other)
    assert not torch.equal(out0, out1)                                    # (the padded positions did change)
    assert torch.equal(torch.where(real, out0, 0.0), torch.where(real, out1, 0.0))
    for g0, g1 in zip(grads0, grads1):
        assert torch.equal(g0 * real, g1 * real)
        assert float((g0 * ~real).abs().max()) == 0 and float((g1 * ~real).abs().max()) == 0
