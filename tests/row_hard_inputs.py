"""Inputs and per-element / per-row float64 bars for the activation, normalisation and loss row kernels
(tests/test_row_hard_inputs.py pins both on the CPU, tests/test_hip_row_hard_inputs.py runs the HIP kernels against them).

Every bar has the three-term form of tests/test_hip_glu.py,

    err_new  <=  h  +  2 * E_eager  +  F

  h        one rounding of the output into its storage type (storage_h): DERIVED from the format.
  E_eager  the error of torch's own composition, evaluated in FLOAT32 on the same stored inputs (upcast), against float64; taken
           at run time; for an elementwise function normalised by the natural scale `s` of the element and maximised over the
           sweep (so a tail counts as much as the bulk), for a row quantity the norm over that row.  The factor two: another
           summation / rounding order (tests/test_hip_glu.py).
  F        a floor: a COUNT of float32 roundings (unit roundoff U32 = 2^-24 each) times the operand magnitude, plus the documented
           1.5e-7 bound of the erf approximation (Abramowitz & Stegun 7.1.26) where erf is used.  The counts are written out at
           FLOOR below; they count the operations any float32 evaluation of the formula needs and are not fitted to a kernel.

Left out of a sweep: non-finite inputs and inputs below the smallest normal float32 (sweep_valid asserts that this is under 0.5 %
of the sweep).  A REFERENCE below the smallest normal float32 is not left out: its bar gets one more 2^-126 (the result may be
flushed), so the kernel still has to return (nearly) nothing there.  A reference beyond the largest finite value of the storage
type (3 * gelu(3.4e38)) has no finite rounding: there the output must be the largest finite value or the infinity of the right
sign, and everywhere else it must be finite.

Plain helper: numpy and torch only, no pytest hooks or settings."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                  # unit roundoff of float32: the largest relative error of one correctly rounded operation
FMIN = 2.0 ** -126                # smallest normal float32
ERF = 1.5e-7                      # |erf error| of Abramowitz & Stegun 7.1.26
CYCLE = (1.0, -0.75, 3.0)         # the linear half / upstream gradient of the activation sweeps
KINDS = ('geglu', 'glu', 'swiglu')
GATE = {'geglu': F.gelu, 'glu': torch.sigmoid, 'swiglu': F.silu}

# ---------------------------------------------------------------------------------------------------------------
# the floors F, relative to the scale `s` of the function (SCALE below)
# ---------------------------------------------------------------------------------------------------------------
# Phi(v) = 0.5 (1 + erf(v / sqrt 2)) in float32, every intermediate at most 1.5 in magnitude, so every rounding moves Phi by at
# most U32:  v/sqrt2 (1), 1 + p a (2), reciprocal (1), a*a (1), exp (2: argument scaling and the 1-ulp hardware exp2), the degree-5
# Horner form (5 mul + 4 add = 9), 0.5 * poly * e (2), 0.5 - . (1), 0.5 +- . (1)  =  20, plus the erf bound itself.
F_PHI = ERF + 20 * U32
# x phi(x) with phi = exp(-x^2/2) / sqrt(2 pi): exp (2) + its squared argument (1) + two products (2), relative to 0.4 |x| <= (1 + |x|)
_F_XPDF = 5 * U32
# sigmoid(g) = 1 / (1 + exp(-g)): exp (2: the argument rounding moves sigma by |g| sigma (1 - sigma) U32 <= 0.23 U32, counted as
# one, and the hardware exp2), the sum (1), the reciprocal (1), and one spare for the 1-ulp reciprocal = 5
_F_SIG = 5 * U32
FLOOR = {
    # y = x Phi(x) k: Phi, the product, the dropout / DropPath factor k
    ('gelu', 'y'): F_PHI + 2 * U32,
    # dx = dy (Phi + x phi) k: Phi, x phi, the sum, two products
    ('gelu', 'dx'): F_PHI + _F_XPDF + 3 * U32,
    # y = e act(g) k
    ('geglu', 'y'): F_PHI + 3 * U32,                 # g Phi(g): Phi + 1; e . (1); k (1)
    ('glu', 'y'): _F_SIG + 2 * U32,
    ('swiglu', 'y'): _F_SIG + 3 * U32,
    # d_e = dy act(g) k: the same operation count as y
    ('geglu', 'd_e'): F_PHI + 3 * U32,
    ('glu', 'd_e'): _F_SIG + 2 * U32,
    ('swiglu', 'd_e'): _F_SIG + 3 * U32,
    # d_g = dy e act'(g) k: three products on top of act'
    ('geglu', 'd_g'): F_PHI + _F_XPDF + 1 * U32 + 3 * U32,              # act' = Phi + g phi
    ('glu', 'd_g'): 2 * _F_SIG + 2 * U32 + 3 * U32,                     # act' = sigma (1 - sigma): sigma twice, 1 - . , the product
    ('swiglu', 'd_g'): 2 * _F_SIG + 4 * U32 + 3 * U32,                  # act' = sigma (1 + g (1 - sigma))
}


def storage_h(ref, dtype):
    """one rounding of `ref` (float64) into dtype, as stated: bf16 2^-8 |ref|; fp16 2^-11 |ref| and at least 2^-25 (half the
    spacing of the fp16 subnormals); fp32 2^-24 |ref|"""
    a = ref.abs()
    if dtype == torch.bfloat16:
        return a * 2.0 ** -8
    if dtype == torch.float16:
        return (a * 2.0 ** -11).clamp_min(2.0 ** -25)
    assert dtype == torch.float32, dtype
    return a * U32


# ---------------------------------------------------------------------------------------------------------------
# A. the activation sweep
# ---------------------------------------------------------------------------------------------------------------
def finite_patterns(dtype):
    """(65536,) in a 16-bit dtype: every bit pattern once, in a fixed shuffled order (so that neighbouring lanes, the two halves of
    a packed pair and the rows of one tile hold unrelated magnitudes); the non-finite patterns (256 in bf16, 2048 in fp16) hold +0
    instead, so that every FINITE pattern appears exactly once and an identity GEMM over a row stays finite."""
    assert dtype in (torch.bfloat16, torch.float16)
    bits = np.random.default_rng(65536).permutation(65536).astype(np.uint16)
    x = torch.from_numpy(bits.view(np.int16).copy()).view(dtype)
    return torch.where(torch.isfinite(x), x, torch.zeros((), dtype=dtype))


def activation_sweep(dtype):
    """(rows, 256) in dtype.  16-bit: finite_patterns, (256, 256).  fp32: the bf16 set upcast, a linear grid on [-8, 8] with step
    2^-10, and 2^16 log-uniform magnitudes in [2^-20, 2^4] with both signs; padded with +0 to whole rows of 256 (833 rows)."""
    if dtype != torch.float32:
        return finite_patterns(dtype).view(256, 256)
    grid = torch.arange(-8 * 1024, 8 * 1024 + 1, dtype=torch.float64) / 1024
    mag = torch.exp2(-20 + 24 * (torch.arange(65536, dtype=torch.float64) + 0.5) / 65536)
    x = torch.cat([finite_patterns(torch.bfloat16).double(), grid, mag, -mag]).float()
    pad = -x.numel() % 256
    return torch.cat([x, torch.zeros(pad)]).view(-1, 256)


def sweep_valid(x):
    """bool mask of the elements of a sweep that are tested: finite, and zero or at least the smallest normal float32 in magnitude"""
    a = x.double().abs()
    valid = torch.isfinite(a) & ((a == 0) | (a >= FMIN))
    assert float((~valid).double().mean()) < 0.005, float((~valid).double().mean())
    return valid


def cycle(shape, shift=0, by_column=False, dtype=torch.float64):
    """CYCLE over the flat index (or over the column index), starting at CYCLE[shift]"""
    n = int(np.prod(shape))
    idx = torch.arange(n).view(shape)
    if by_column:
        idx = torch.arange(shape[-1]).expand(shape)
    return torch.tensor(CYCLE, dtype=torch.float64)[(idx + shift) % 3].to(dtype)


def gelu_case(x, dy):
    """x, dy: stored tensors of one shape.  name -> (eager float32, float64 reference, scale s) for y = gelu(x), dx = dy gelu'(x)"""
    out = {}
    for tag, dt in (('e', torch.float32), ('r', torch.float64)):
        xx = x.detach().to(dt).clone().requires_grad_(True)
        y = F.gelu(xx)
        y.backward(dy.to(dt))
        out[tag] = (y.detach(), xx.grad)
    a, d = x.double().abs(), dy.double().abs()
    return {'y': (out['e'][0], out['r'][0], a), 'dx': (out['e'][1], out['r'][1], d * (1 + a))}


def glu_case(g, e, dy, kind):
    """name -> (eager float32, float64 reference, scale s) for y = e act(g), d_g, d_e (the table of the issue)"""
    out = {}
    for tag, dt in (('e', torch.float32), ('r', torch.float64)):
        gg, ee = (t.detach().to(dt).clone().requires_grad_(True) for t in (g, e))
        y = ee * GATE[kind](gg)
        y.backward(dy.to(dt))
        out[tag] = (y.detach(), gg.grad, ee.grad)
    ga, ea, da = g.double().abs(), e.double().abs(), dy.double().abs()
    s_y = ea if kind == 'glu' else ea * ga.clamp_min(1.0)
    s = {'y': s_y, 'd_g': da * ea * (1 + ga), 'd_e': da * ga.clamp_min(1.0)}
    return {n: (out['e'][i], out['r'][i], s[n]) for i, n in enumerate(('y', 'd_g', 'd_e'))}


def elementwise_ratio(name, new, eager32, ref, s, dtype, floor, valid, signed_zero=False):
    """The bar of the module docstring for one tensor; returns (largest err / bar over the tested elements, E_new): E_new is
    the error of `new` measured as E_eager is, the largest err / s (in a 16-bit type mostly the storage rounding).
    Asserts what no ratio expresses: finite outputs, saturated outputs, signed zeros, and that E_eager is itself within the floor
    (torch's float32 composition is a float32 evaluation: were it outside, the count behind the floor would be wrong and twice
    E_eager could hide anything)."""
    ref, new64, s = ref.double(), new.double(), s.double()
    fmax = torch.finfo(dtype).max
    sat = ref.abs() > fmax                                    # beyond the largest finite value of the storage type
    ok = valid & ~sat
    assert torch.isfinite(new64[ok]).all(), (name, 'non-finite output')
    if bool(sat.any()):
        got, want = new64[valid & sat], ref[valid & sat]
        assert torch.all((got.abs() >= fmax) & (torch.signbit(got) == torch.signbit(want))), (name, 'saturated outputs')
    # (torch's float32 GELU forms x (1 + erf) before it halves and overflows in the top binade: such elements cannot enter E_eager;
    # they stay in the test)
    e_fin = torch.isfinite(eager32)
    assert float((ok & ~e_fin).double().mean()) < 0.005, (name, 'eager float32 is non-finite too often')
    e_ok = ok & e_fin & (ref.abs() >= FMIN) & (s > 0)
    E = float(((eager32.double() - ref).abs()[e_ok] / s[e_ok]).max()) if bool(e_ok.any()) else 0.0
    assert E <= floor, (name, 'E_eager outside the floor', E, floor)
    bar = storage_h(ref, dtype) + (2 * E + floor) * s + (ref.abs() < FMIN) * FMIN
    err = (new64 - ref).abs()
    ratio = err[ok] / bar[ok]
    i = int(torch.argmax(ratio))
    E_new = float((err[e_ok] / s[e_ok]).max()) if bool(e_ok.any()) else 0.0
    print(f'{name}: E_eager {E:.3e} E_new {E_new:.3e} floor {floor:.3e} worst ratio {float(ratio[i]):.3f} '
          f'(err {float(err[ok][i]):.3e} ref {float(ref[ok][i]):.3e})')
    if signed_zero:
        z = ok & (ref == 0) & (new64 == 0)
        assert torch.all(torch.signbit(new64[z]) == torch.signbit(ref[z])), (name, 'signed zero')
    return float(ratio[i]), E_new


# ---------------------------------------------------------------------------------------------------------------
# B. LayerNorm rows with structure
# ---------------------------------------------------------------------------------------------------------------
OFFSETS = [(m, s) for m in (0.0, 30.0, -30.0, 1000.0, -1000.0) for s in (1e-2, 1.0, 30.0)]


def row_kinds(dtype):
    kinds = [('offset', m, s) for m, s in OFFSETS]
    kinds += [('const', 3.0), ('const', -1000.0), ('zero',), ('outlier',), ('alternating',)]
    if dtype == torch.float16:
        kinds += [('edge', 6e4), ('edge', -6e4)]
    return kinds


def structured_rows(M, C, dtype, seed=0):
    """(M, C) in dtype; row r is of kind row_kinds(dtype)[r % len]: 20 kinds (22 in fp16) against tiles of 32 rows, so every tile
    holds every kind next to rows whose mean and spread differ by orders of magnitude.
      offset       m + s z, m in {0, +-30, +-1000}, s in {1e-2, 1, 30}   (in a 16-bit type m = 1000 swallows s = 1e-2: constant rows)
      const, zero  no variance: rstd = eps^-1/2
      outlier      N(0,1) with one channel at 1e4
      alternating  +big, -big, ...  (big = 1e15; 3e4 in fp16): rstd ~ 1 / big
      edge         fp16 only: +-(6e4 + 32 k), |k| <= 8, next to the largest finite value 65504"""
    rng = np.random.default_rng(1000 * M + C + seed)
    kinds = row_kinds(dtype)
    x = np.zeros((M, C))
    for r in range(M):
        kind = kinds[r % len(kinds)]
        z = rng.standard_normal(C)
        if kind[0] == 'offset':
            x[r] = kind[1] + kind[2] * z
        elif kind[0] == 'const':
            x[r] = kind[1]
        elif kind[0] == 'outlier':
            x[r] = z
            x[r, rng.integers(C)] = 1e4
        elif kind[0] == 'alternating':
            x[r] = (3e4 if dtype == torch.float16 else 1e15) * (1 - 2 * (np.arange(C) % 2))
        elif kind[0] == 'edge':
            x[r] = kind[1] + 32.0 * rng.integers(-8, 9, C)
    return torch.from_numpy(x).to(dtype)


def ln_params(C, device='cpu', seed=0):
    g = torch.Generator().manual_seed(C + seed)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).float()
    beta = (0.1 * torch.randn(C, generator=g)).float()
    return gamma.to(device), beta.to(device)


def ln_reference(x, gamma, beta, eps, dy=None, dt=torch.float64):
    """LayerNorm of the stored rows x in `dt` by the textbook formulas: dict y, mean, rstd and, with dy, dx, dgamma_terms = dy xhat,
    g = dy gamma.  (float32: torch's own ops, see ln_eager32.)"""
    x, gamma, beta = x.to(dt), gamma.to(dt), beta.to(dt)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    out = dict(y=xh * gamma + beta, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1), xhat=xh)
    if dy is not None:
        g = dy.to(dt) * gamma
        out['g'] = g
        out['dx'] = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
        out['dgamma'] = (dy.to(dt) * xh).sum(0)
        out['dbeta'] = dy.to(dt).sum(0)
    return out


def ln_eager32(x, gamma, beta, eps, dy=None):
    """torch's own float32 LayerNorm (native_layer_norm and its autograd) on the stored rows, upcast"""
    C = x.shape[-1]
    xx, gg, bb = x.detach().float().clone().requires_grad_(True), gamma.float().clone().requires_grad_(True), beta.float().clone().requires_grad_(True)
    y, mean, rstd = torch.native_layer_norm(xx, (C,), gg, bb, eps)
    out = dict(y=y.detach(), mean=mean.detach().reshape(-1), rstd=rstd.detach().reshape(-1))
    if dy is not None:
        y.backward(dy.float())
        out.update(dx=xx.grad, dgamma=gg.grad, dbeta=bb.grad)
    return out


def ln_delta(x, given_stats=False):
    """error of the row mean a float32 kernel may make: a C-term sum is log2 C roundings deep, times 1/C and the final rounding,
    each relative to max |x_row|  ->  (log2 C + 2) U32 max|x_row|.  given_stats: the mean was handed in as the float32 rounding of
    the exact one: U32 max|x_row|."""
    C = x.shape[-1]
    return (1.0 if given_stats else math.log2(C) + 2) * U32 * x.double().abs().amax(-1)


def _row_tol(ref, dtype):
    """one storage rounding of a row: tol ||ref|| (fp16: plus 2^-25 per element for the subnormal spacing)"""
    tol = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: U32}[dtype]
    extra = 2.0 ** -25 * math.sqrt(ref.shape[-1]) if dtype == torch.float16 else 0.0
    return tol * ref.norm(dim=-1) + extra


def _worst(name, err, bar):
    """largest err / bar; a zero bar asks for a zero error"""
    err, bar = err.detach(), bar.detach()
    assert torch.isfinite(bar).all(), (name, 'non-finite bar')
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(err), ratio, torch.full_like(err, math.inf))        # a non-finite output misses every bar
    i = int(torch.argmax(ratio))
    print(f'{name}: worst ratio {float(ratio[i]):.3f} at {i} (err {float(err[i]):.3e} bar {float(bar[i]):.3e})')
    return float(ratio[i])


def ln_forward_ratios(name, x, gamma, new, ref, eager, dtype, given_stats=False):
    """per ROW, the worst row returned: name -> ratio for y, mean, rstd.
      y     ||err|| <= 2 ||err_eager32|| + tol ||ref|| + (log2 C + 2) U32 max|x_row| rstd_row ||gamma||       (the issue's bar: the
            last term is the row's conditioning, one float32 rounding of the mean seen through rstd)
      mean  |err| <= 2 |err_eager32| + delta,  delta = ln_delta
      rstd  |err| <= 2 |err_eager32| + rstd ((log2 C + 4) U32 + (delta rstd)^2): the mean's error enters the variance only in
            second order (sum of (x - m) vanishes), the sum of squares is log2 C + 1 roundings deep, + eps, rsqrt, storing."""
    C = x.shape[-1]
    delta = ln_delta(x, given_stats)
    rstd = ref['rstd']
    out = {}
    cond = delta * rstd * float(gamma.double().norm())
    out['y'] = _worst(f'{name} y', (new['y'].double() - ref['y']).norm(dim=-1),
                      2 * (eager['y'].double() - ref['y']).norm(dim=-1) + _row_tol(ref['y'], dtype) + cond)
    if 'mean' in new:
        out['mean'] = _worst(f'{name} mean', (new['mean'].double() - ref['mean']).abs(),
                             2 * (eager['mean'].double() - ref['mean']).abs() + delta)
        out['rstd'] = _worst(f'{name} rstd', (new['rstd'].double() - rstd).abs(),
                             2 * (eager['rstd'].double() - rstd).abs() + rstd * ((math.log2(C) + 4) * U32 + (delta * rstd) ** 2))
    return out


def ln_backward_row_bar(x, ref, eager_dx, dtype, given_stats=False, roundings=1, factor=1.0):
    """(M,) bar on ||dx_new - dx_ref|| per row for dx = rstd (g - mean g - xhat mean(g xhat)), g = dy gamma:
        2 ||err_eager32|| + roundings * tol ||ref||
        + 2 c (1 + c) rstd ||g||            c = delta rstd: xhat is off by the constant c along the row; term by term the change of
                                            xhat mean(g xhat) has norm <= 2 c ||g|| (+ c^2 ||g||) since ||xhat|| <= sqrt C
        + 2 er rstd ||g||                   er = (log2 C + 4) U32 + c^2: the relative error of the saved rstd, which scales both dx
                                            and xhat
        + (log2 C + 6) U32 rstd ||g||       the two row means (log2 C roundings deep, relative to sum |terms| <= sqrt C ||g||) and
                                            the six elementwise operations
    `roundings`: how often the value was rounded to the storage type on its way (2 for a gradient that is the stored product of a
    stored gradient and the per-graph factor); `factor`: that per-row factor, which scales the derived terms as it scales dx."""
    C = x.shape[-1]
    c = ln_delta(x, given_stats) * ref['rstd']
    er = (math.log2(C) + 4) * U32 + c ** 2
    rg = ref['rstd'] * ref['g'].norm(dim=-1)
    return 2 * (eager_dx.double() - ref['dx']).norm(dim=-1) + roundings * _row_tol(ref['dx'], dtype) + \
        (2 * c * (1 + c) + 2 * er + (math.log2(C) + 6) * U32) * rg * factor


def column_sum_bar(terms, eager_err=None, extra=None):
    """(C,) bar of a float32 column sum over M rows against float64, relative to sum |terms| of the column as tests/test_hip_ops.py::
    test_sum_planes: (log2 M + 8) U32 sum_m |term_mc| (a sum log2 M deep in the best order, eight spare for partial rows and the
    term's own arithmetic) + 2 |err_eager32| + `extra` (the conditioning of the terms, summed with absolute values)."""
    M = terms.shape[0]
    bar = (math.log2(M) + 8) * U32 * terms.double().abs().sum(0)
    if eager_err is not None:
        bar = bar + 2 * eager_err.double().abs()
    if extra is not None:
        bar = bar + extra
    return bar


def ln_dgamma_extra(x, dy, ref, given_stats=False):
    """conditioning of the dgamma terms dy xhat: xhat is off by c_m along row m and by the relative error er_m of rstd"""
    C = x.shape[-1]
    c = ln_delta(x, given_stats) * ref['rstd']
    er = (math.log2(C) + 4) * U32 + c ** 2
    return (dy.double().abs() * (c[:, None] + er[:, None] * ref['xhat'].abs())).sum(0)


# ---------------------------------------------------------------------------------------------------------------
# C. cross entropy rows and the Gaussian basis
# ---------------------------------------------------------------------------------------------------------------
XENT_SHAPES = [(37, 1024), (513, 40), (64, 2048), (800, 512)]
XENT_OFFSET = {torch.float16: 3e4, torch.bfloat16: 1e4, torch.float32: 1e4}


def xent_rows(rows, C, dtype, seed=0):
    """(logits (rows, C) in dtype, target (rows,) int64, weight (rows,) float32 with exact zeros = masked rows).  Row r is of kind
    r % 7:  0 3 z;  1 one logit 60 above z, the target on it;  2 the same, the target off it;  3 all logits equal (target 0 / C - 1
    in turn);  4 z + offset;  5 z - offset (3e4 in fp16, 1e4 in bf16 / fp32);  6 z with an eighth of the entries at the most
    negative finite value.  target[0] = 0, target[-1] = C - 1."""
    rng = np.random.default_rng(rows * 4096 + C + seed)
    x = rng.standard_normal((rows, C))
    target = rng.integers(0, C, rows)
    lo = float(torch.finfo(dtype).min)
    for r in range(rows):
        k = r % 7
        if k == 0:
            x[r] *= 3
        elif k in (1, 2):
            peak = int(rng.integers(C))
            x[r, peak] = x[r].max() + 60
            target[r] = peak if k == 1 else (peak + 1 + int(rng.integers(C - 1))) % C
        elif k == 3:
            x[r] = 0.5
            target[r] = 0 if (r // 7) % 2 == 0 else C - 1
        elif k in (4, 5):
            x[r] += XENT_OFFSET[dtype] * (1 if k == 4 else -1)
        else:
            x[r, rng.random(C) < 0.125] = lo
            x[r, target[r]] = 0.25                     # the target's logit is an ordinary one
            x[r, (target[r] + 1) % C] = lo
    target[0], target[-1] = 0, C - 1
    w = (0.5 + 1.5 * rng.random(rows)) * (rng.random(rows) < 0.7)
    return torch.from_numpy(x).to(dtype), torch.from_numpy(target), torch.from_numpy(w).float()


def xent_case(logits, target, w):
    """float64 reference and float32 eager of lse, xent and the gradient of sum(w * xent)"""
    out = {}
    for tag, dt in (('eager', torch.float32), ('ref', torch.float64)):
        x = logits.detach().to(dt).clone().requires_grad_(True)
        xent = F.cross_entropy(x, target, reduction='none')
        (xent * w.to(dt)).sum().backward()
        out[tag] = dict(xent=xent.detach(), lse=torch.logsumexp(x.detach(), -1), grad=x.grad)
    return out


def xent_magnitude(logits):
    """max(1, max |x_row|) over the entries that can reach the float32 result at all: those within 104 of the row maximum
    (exp(-104) < 2^-149 adds exactly nothing to a float32 sum); an entry at the most negative finite value does not set the scale"""
    x = logits.double()
    live = x >= x.amax(-1, keepdim=True) - 104
    return torch.where(live, x.abs(), torch.zeros_like(x)).amax(-1).clamp_min(1.0)


def xent_ratios(name, logits, w, new, case, dtype):
    """xent, lse per row: h + 2 E_eager + 4 U32 max(1, max|x_row|), h the float32 rounding of the result itself (the first term of
    the common form: lse = 0.5 + log 2048 = 8.1 cannot be stored closer than 4.8e-7, whatever the logits' magnitude);  gradient per
    element: h + 2 E_eager + 4 U32 |w_row| (E_eager: the largest eager error of the row);  masked rows exactly zero."""
    ref, eager = case['ref'], case['eager']
    mag = xent_magnitude(logits)
    out = {}
    for k in ('xent', 'lse'):
        out[k] = _worst(f'{name} {k}', (new[k].double() - ref[k]).abs(), storage_h(ref[k], torch.float32) + 2 * (eager[k].double() - ref[k]).abs() + 4 * U32 * mag)
    g = ref['grad']
    E = (eager['grad'].double() - g).abs().amax(-1, keepdim=True)
    bar = storage_h(g, dtype) + 2 * E + 4 * U32 * w.double().abs()[:, None] + (g.abs() < FMIN) * FMIN
    live = w != 0
    assert torch.all(new['grad'][~live] == 0), (name, 'masked rows')
    out['grad'] = _worst(f'{name} grad', (new['grad'].double() - g).abs()[live].reshape(-1), bar[live].reshape(-1))
    return out


GAUSS_SHAPE = (2, 48, 48)          # 4608 pairs: a grid capped at 1024 workgroups of four waves makes a second trip
GAUSS_KS = (2, 130, 512)
GAUSS_NORM = (2 * 3.14159) ** 0.5


def gaussian_inputs(K, seed=0):
    """x, mul, bias (float32, GAUSS_SHAPE [+ (1,)]), means, stds (1, K): t = mul x + bias spreads over [-2, 40] (exp underflows
    long before), stds hold an exact 0, negatives and |std| from 3 down to 1e-6."""
    rng = np.random.default_rng(K + seed)
    x = rng.uniform(0.0, 6.0, GAUSS_SHAPE)
    x[rng.random(GAUSS_SHAPE) < 0.1] *= 3.0
    mul = 1.0 + 0.2 * rng.standard_normal(GAUSS_SHAPE + (1,))
    mul[rng.random(GAUSS_SHAPE + (1,)) < 0.05] = 2.2
    bias = 0.2 * rng.standard_normal(GAUSS_SHAPE + (1,))
    x[0, 0, 0], mul[0, 0, 0, 0], bias[0, 0, 0, 0] = 18.2, 2.2, 0.0           # t = 40.04
    x[1, 47, 47], mul[1, 47, 47, 0], bias[1, 47, 47, 0] = 0.0, 1.0, -2.0     # t = -2
    means = rng.uniform(0.0, 3.0, (1, K))
    stds = rng.uniform(-3.0, 3.0, (1, K))
    stds[0, 0] = 0.0
    stds[0, 1] = -1e-3
    if K > 4:
        stds[0, 2], stds[0, 3], stds[0, K - 1] = 1e-6, -0.0, 1e-2
    f = [torch.from_numpy(a).float() for a in (x, mul, bias, means, stds)]
    assert float((f[1].squeeze(-1) * f[0] + f[2].squeeze(-1)).max()) >= 39.0
    return f


def gaussian_case(x, mul, bias, means, stds, gy, dt):
    """the reference's composition (lib/models/pcqm/layers.py:129-157) in `dt` with autograd: y and the four gradients, plus (float64
    only) the per-term tensors the bars are relative to"""
    leaves = [t.detach().to(dt).clone().requires_grad_(True) for t in (mul, bias, means, stds)]
    t = leaves[0] * x.to(dt).unsqueeze(-1) + leaves[1]
    sg = leaves[3].view(-1).abs() + 1e-2
    y = torch.exp(-0.5 * (((t - leaves[2].view(-1)) / sg) ** 2)) / (GAUSS_NORM * sg)
    (y * gy.to(dt)).sum().backward()
    out = dict(y=y.detach(), dmul=leaves[0].grad, dbias=leaves[1].grad, dmeans=leaves[2].grad, dstds=leaves[3].grad)
    if dt == torch.float64:
        with torch.no_grad():
            z = (t - leaves[2].view(-1)) / sg
            gyy = gy.double() * y
            tmag = 2 * U32 * ((leaves[0] * x.double().unsqueeze(-1)).abs() + t.abs())        # two roundings of t = mul x + bias
            out.update(coef=1 / (GAUSS_NORM * sg), sg=sg, z=z, tmag=tmag,
                       t_dt=gyy * z / sg, t_dmean=gyy * z / sg, t_dstd=gyy * (z * z - 1) / sg,
                       # |d term / d t| tmag: what the rounding of t alone does to each term
                       c_y=(y * z / sg).abs() * tmag, c_dt=(gyy * (1 - z * z) / sg ** 2).abs() * tmag,
                       c_dstd=(gyy * (3 * z - z ** 3) / sg ** 2).abs() * tmag)
            # the exponential is a float32 number of its own: below 2^-126 it may be flushed, whatever coef (up to 40) and z / sigma
            # (up to 1e5) make of it afterwards
            fl = FMIN / (GAUSS_NORM * sg)
            out.update(f_y=fl + 0 * y, f_dt=fl * (gy.double() * z / sg).abs(), f_dstd=fl * (gy.double() * (z * z - 1) / sg).abs())
    return out


def gaussian_ratios(name, new, ref, eager, dtype, x):
    """y per element: h + 2 E_k coef_k + 2^-22 coef_k + c_y  (E_k: eager's largest error of basis function k over coef_k; c_y: the
    two float32 roundings of t seen through dy/dt = y z / sigma -- with sigma = 0.01 a rounding of t = 40 moves z by 2e-4).
    dbias, dmul per pair and dmeans, dstds per k: 2 |err_eager32| + (log2 n + 8) U32 sum |terms| + the same conditioning summed.
    Every bar also carries the flush of the exponential (gaussian_case: f_y, f_dt, f_dstd), 1e-36 and less."""
    out = {}
    K = ref['y'].shape[-1]
    coef = ref['coef']
    E = ((eager['y'].double() - ref['y']).abs() / coef).reshape(-1, K).amax(0)
    bar = storage_h(ref['y'], dtype) + (2 * E + 2.0 ** -22) * coef + ref['c_y'] + ref['f_y']
    out['y'] = _worst(f'{name} y', (new['y'].double() - ref['y']).abs().reshape(-1), bar.reshape(-1))
    fl_k, P = (math.log2(K) + 8) * U32, ref['y'].numel() // K
    fl_p = (math.log2(P) + 8) * U32
    dt_bar = fl_k * ref['t_dt'].abs().sum(-1, keepdim=True) + (ref['c_dt'] + ref['f_dt']).sum(-1, keepdim=True)
    xa = x.double().abs().unsqueeze(-1)
    for k, scale in (('dbias', 1.0), ('dmul', xa)):              # dmul = dbias x: one more rounding
        bar = 2 * (eager[k].double() - ref[k]).abs() + dt_bar * scale + U32 * ref[k].abs()
        out[k] = _worst(f'{name} {k}', (new[k].double() - ref[k]).abs().reshape(-1), bar.reshape(-1))
    for k, terms, c, f in (('dmeans', 't_dmean', 'c_dt', 'f_dt'), ('dstds', 't_dstd', 'c_dstd', 'f_dstd')):
        bar = 2 * (eager[k].double() - ref[k]).abs().reshape(-1) + fl_p * ref[terms].abs().reshape(-1, K).sum(0) + \
            (ref[c] + ref[f]).reshape(-1, K).sum(0)
        out[k] = _worst(f'{name} {k}', (new[k].double() - ref[k]).abs().reshape(-1), bar)
    return out
