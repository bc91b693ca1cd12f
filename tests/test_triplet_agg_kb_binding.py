"""CPU-side checks of the triplet aggregate entry points at 65 <= N <= 128 (csrc/triplet_aggregate_kb.hip): the order of the
refusals (sizes, N > 128, D at N > 64, then the tensors), with null tensors so that nothing is launched."""
import ctypes as C

import pytest


def _args(B=2, N=80, H=4, D=16, dtype=1, flags=3):
    from tgt_amd import _lib
    a = _lib.TripletAggregateArgs()
    a.B, a.N, a.H, a.D, a.dtype, a.flags = B, N, H, D, dtype, flags
    return a


def _entries():
    from tgt_amd import _lib
    L = _lib.lib()
    return L, (L.tgt_triplet_aggregate_fwd, L.tgt_triplet_aggregate_bwd)


def test_refusal_above_128_names_the_limit():
    L, fns = _entries()
    for fn in fns:
        assert fn(C.byref(_args(N=129)), None) == 2            # TGT_ERR_UNSUPPORTED, before any tensor is looked at
        assert b'128' in L.tgt_last_error()


def test_refusal_of_other_head_widths_above_64_names_d():
    L, fns = _entries()
    for fn in fns:
        assert fn(C.byref(_args(N=80, D=8)), None) == 2
        assert b'D=8' in L.tgt_last_error()
        assert fn(C.byref(_args(N=128, D=32)), None) == 2
        assert b'D=32' in L.tgt_last_error()


@pytest.mark.parametrize('N', [65, 80, 128])
@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_shapes_up_to_128_reach_the_tensor_check(N, dtype):
    L, fns = _entries()
    for fn in fns:
        assert fn(C.byref(_args(N=N, D=16, H=4, dtype=dtype)), None) == 1      # TGT_ERR_INVALID: the shape is accepted
        assert b'null tensor' in L.tgt_last_error()
        assert fn(C.byref(_args(N=N, D=16, H=3, dtype=dtype)), None) == 1      # H not a multiple of 4


@pytest.mark.parametrize('N', [1, 64])
def test_small_shapes_still_reach_the_tensor_check(N):
    L, fns = _entries()
    for D in (8, 16, 32):
        for fn in fns:
            assert fn(C.byref(_args(N=N, D=D)), None) == 1


def test_bad_sizes_come_first():
    L, fns = _entries()
    for fn in fns:
        assert fn(C.byref(_args(N=129, H=0)), None) == 1
        assert fn(C.byref(_args(N=-1)), None) == 1
        assert fn(C.byref(_args(N=0)), None) == 0


def test_abi_and_struct_are_unchanged():
    from tgt_amd import _lib
    assert _lib.ABI_VERSION == 32 and _lib.lib().tgt_abi_version() == 32
    AA = _lib.TripletAggregateArgs
    assert C.sizeof(AA) == 200
    assert [f[0] for f in AA._fields_][-3:] == ['dropout_p', '_pad1', 'dropout_seed']
    assert AA.dropout_seed.offset == 192
