"""Inputs and per-element float64 bars for the plain activations of the FFN block (relu / silu / elu: csrc/act.hpp), after
tests/row_hard_inputs.py, whose sweep and helpers this module imports.  tests/test_act_hard_inputs.py pins the bars on the CPU,
tests/test_hip_act.py runs the HIP kernels against them.

The sweep: every finite bf16 / fp16 bit pattern once (row_hard_inputs.finite_patterns, as a (256, 256) tensor) as x, crossed with
CYCLE = (1, -0.75, 3) over the flat index as the upstream gradient dy; in float32 storage the wider set of
row_hard_inputs.activation_sweep.  Left out: what sweep_valid leaves out (non-finite, below the smallest normal float32).

Every bar is

    |new - ref|  <=  h + F * s     (+ 2^-126 where |ref| < 2^-126: the result may be flushed)

  ref  the float64 value of F.relu / F.silu / F.elu (and of its autograd gradient) on the input AS STORED
  h    one rounding of ref into the storage type (row_hard_inputs.storage_h): derived from the format
  s    the natural scale of the element (SCALE below)
  F    a floor: a COUNT of float32 roundings (unit roundoff U32 = 2^-24 each), written out at FLOOR below.  The counts follow from
       the formulas of csrc/act.hpp = the operations any float32 evaluation needs; they are not fitted to a kernel's result.

Plain helper: numpy and torch only, no pytest hooks or settings."""
import numpy as np
import torch
import torch.nn.functional as F

import golden_util as gu
import row_hard_inputs as rh
from row_hard_inputs import U32, FMIN, CYCLE, finite_patterns, activation_sweep, sweep_valid, cycle, storage_h      # noqa: F401

KINDS = ('relu', 'silu', 'elu')
FN = {'relu': F.relu, 'silu': F.silu, 'elu': F.elu}
ELU_SERIES_BELOW = 0.5            # act.hpp: expm1 by its Taylor polynomial for |x| < 1/2, exp(x) - 1 from there on

# ---------------------------------------------------------------------------------------------------------------
# the floors F, relative to the scale s
# ---------------------------------------------------------------------------------------------------------------
# exp(x) for x <= 0 in float32: the argument scaling x log2(e) (one rounding of a number of magnitude 1.44 |x|, which moves e^x by
# |x| e^x U32) and the 1-ulp hardware exp2 (2 e^x U32): together (|x| + 2) e^x U32 <= 2 U32, the maximum at x = 0.  Counted as 2.
_F_EXP = 2 * U32
# expm1(x), x <= 0, relative to s = min(|x|, 1).
#   |x| >= 1/2, as exp(x) - 1: exp's absolute error (|x| + 2) e^x U32, largest at the switch point (2.5 e^-1/2 = 1.52 U32), plus the
#   subtraction's rounding of a number below 1 (1 U32): 2.52 U32 against s = 1/2 -> 5.04; at |x| = 1 it is 2.1.  Counted as 6.
#   |x| < 1/2, Horner form x (1 + x (1/2 + x (1/6 + ...))) up to x^8 / 8!: every partial sum lies in [0.6, 1], so the rounding of
#   step j reaches the result times |x|^j: at most 1 / (1 - 1/2) = 2 roundings in all, the closing product (1) and the first
#   dropped term (x^8 / 9! <= 0.18 U32): 3.2.  exp(x) - 1 itself would fail here: its error is U32 / |x| relative (2^-12 at
#   x = -2^-12, where a float16 result is held to 2^-11), which is what the pinning test's negative control shows.
F_EXPM1 = 6 * U32
# sigmoid: row_hard_inputs._F_SIG (exp 2, the sum 1, the reciprocal 1, one spare for the 1-ulp reciprocal = 5)
_F_SIG = rh._F_SIG
FLOOR = {
    # relu: the comparison is exact; y = x k and dx = dy 1 k carry the dropout / DropPath factor k (1) and, dx, the product with the
    # 0 / 1 derivative (exact, counted as 1)
    ('relu', 'y'): 1 * U32,
    ('relu', 'dx'): 2 * U32,
    # silu: y = x sigma k: sigma + two products
    ('silu', 'y'): _F_SIG + 2 * U32,
    # dx = dy sigma (1 + x (1 - sigma)) k: the swiglu gate of row_hard_inputs.FLOOR[('swiglu', 'd_g')] without the linear half:
    # sigma twice, 1 - ., x ., 1 + ., sigma . (4), and the two products with dy and k (2)
    ('silu', 'dx'): 2 * _F_SIG + 4 * U32 + 2 * U32,
    # elu: y = x k (x > 0) or expm1(x) k
    ('elu', 'y'): F_EXPM1 + 1 * U32,
    # dx = dy k (x > 0) or dy exp(x) k: exp and two products
    ('elu', 'dx'): _F_EXP + 2 * U32,
}


def scales(kind, x, dy):
    """name -> s (float64): y relative to |x| (elu below zero: to min(|x|, 1), the magnitude of expm1 up to a factor 1.6); dx relative
    to |dy| (silu: |dy| (1 + |x|), the bound of |d act' / d sigma| that carries sigma's error into the derivative)"""
    a, d = x.double().abs(), dy.double().abs()
    if kind == 'relu':
        return {'y': a, 'dx': d}
    if kind == 'silu':
        return {'y': a, 'dx': d * (1 + a)}
    return {'y': torch.where(x.double() > 0, a, a.clamp_max(1.0)), 'dx': d}


def act_case(x, dy, kind):
    """x, dy: stored tensors of one shape.  name -> (eager float32, float64 reference, scale s) for y = act(x), dx = dy act'(x)"""
    out = {}
    for tag, dt in (('e', torch.float32), ('r', torch.float64)):
        xx = x.detach().to(dt).clone().requires_grad_(True)
        y = FN[kind](xx)
        y.backward(dy.to(dt))
        out[tag] = (y.detach(), xx.grad)
    s = scales(kind, x, dy)
    return {'y': (out['e'][0], out['r'][0], s['y']), 'dx': (out['e'][1], out['r'][1], s['dx'])}


def act_ratio(name, new, ref, s, dtype, floor, valid):
    """largest err / bar over the tested elements for the bar of the module docstring; asserts finite outputs"""
    ref, new64, s = ref.double(), new.double(), s.double().to(ref.device)
    valid = valid.to(ref.device)
    assert float(ref.abs()[valid].max()) <= torch.finfo(dtype).max, (name, 'the reference leaves the storage type')
    assert torch.isfinite(new64[valid]).all(), (name, 'non-finite output')
    bar = storage_h(ref, dtype) + floor * s + (ref.abs() < FMIN) * FMIN
    err = (new64 - ref).abs()
    ratio = err[valid] / bar[valid].clamp_min(1e-300)
    ratio = torch.where((bar[valid] == 0) & (err[valid] == 0), torch.zeros_like(ratio), ratio)
    i = int(torch.argmax(ratio))
    print(f'{name}: floor {floor:.3e} worst ratio {float(ratio[i]):.3f} (err {float(err[valid][i]):.3e} ref {float(ref[valid][i]):.3e})')
    return float(ratio[i])


# ---------------------------------------------------------------------------------------------------------------
# float32 numpy restatement of csrc/act.hpp (act_fwd / act_grad), operation by operation
# ---------------------------------------------------------------------------------------------------------------
_f32 = np.float32


def _fma(a, b, c):
    """one rounding of a b + c (the product of two float32 is exact in float64)"""
    return (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(_f32)


def _sigmoid32(x):
    with np.errstate(over='ignore'):
        return (_f32(1) / (_f32(1) + np.exp(-x))).astype(_f32)


def expm1_neg32(x, series_below=ELU_SERIES_BELOW):
    """act_expm1_neg: series for x > -series_below, exp(x) - 1 otherwise (series_below = 0: the cancelling form everywhere)"""
    p = np.full_like(x, _f32(1.0 / 40320.0))
    for c in (1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0):
        p = _fma(p, x, _f32(c))
    return np.where(x > _f32(-series_below), p * x, np.exp(x).astype(_f32) - _f32(1)).astype(_f32)


def act_fwd32(x, kind, series_below=ELU_SERIES_BELOW):
    x = np.asarray(x, dtype=_f32)
    if kind == 'relu':
        return np.where(x < 0, _f32(0), x).astype(_f32)
    if kind == 'silu':
        return (x * _sigmoid32(x)).astype(_f32)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.where(x > 0, x, expm1_neg32(np.minimum(x, _f32(0)), series_below)).astype(_f32)


def act_grad32(x, kind):
    x = np.asarray(x, dtype=_f32)
    if kind == 'relu':
        return (x > 0).astype(_f32)
    if kind == 'silu':
        s = _sigmoid32(x)
        with np.errstate(over='ignore', invalid='ignore'):
            return (s * (_f32(1) + x * (_f32(1) - s))).astype(_f32)
    return np.where(x > 0, _f32(1), np.exp(np.minimum(x, _f32(0)))).astype(_f32)


# ---------------------------------------------------------------------------------------------------------------
# the counter-based drop pattern of the activation kernels (csrc/common.hpp keep_vector on golden_util's hash restatement)
# ---------------------------------------------------------------------------------------------------------------
def drop_thresh(p):
    return 0 if p <= 0 else int(min(65535, max(1, np.rint(np.float32(p) * np.float32(65536.0)))))


def keep_pattern_np(n, elem_size, p, seed, counter=None):
    """(n,) bool: keep flags of a flat tensor of n elements of `elem_size` bytes (n a multiple of the 16-byte vector).  One hash of
    (seed, vector index), then one 32-bit word per two elements, 16 bits each; kept where the 16 bits reach the threshold.
    counter: the device step counter mixed into the seed (tgt_set_seed_counter), or None."""
    V = 16 // elem_size
    assert n % V == 0
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if counter is not None:
        seed = (seed + int(counter) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    vec = np.arange(n // V, dtype=np.uint64)
    lo, hi = vec & np.uint64(0xFFFFFFFF), vec >> np.uint64(32)
    base = gu._mix32(lo ^ np.uint64(seed & 0xFFFFFFFF)) ^ gu._mix32((hi + np.uint64(seed >> 32) + np.uint64(0x9e3779b9)) & np.uint64(0xFFFFFFFF))
    keep = np.empty((n // V, V), dtype=bool)
    t = drop_thresh(p)
    for w in range(V // 2):
        r = gu._mix32((base + np.uint64(((w + 1) * 0x9e3779b9) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF))
        keep[:, 2 * w] = (r & np.uint64(0xFFFF)) >= t
        keep[:, 2 * w + 1] = (r >> np.uint64(16)) >= t
    return keep.reshape(-1)
