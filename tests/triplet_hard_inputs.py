"""Inputs on which the triplet kernels can be wrong without a prefix mask and unit-variance logits noticing
(tests/test_triplet_hard_inputs.py pins their properties on the CPU, tests/test_hip_triplet_hard_inputs.py runs the kernels on them):

  pair_mask     a per-pair additive mask that is NOT symmetric, with scattered closed pairs and whole LEADING key blocks closed for
                some queries, in both directions (inward the key is the 2nd index of M, outward the 1st) -- the construction of
                tests/test_hip_ops.py::test_node_attention_arbitrary_mask_and_large_logits, made two-sided and confined to the real
                block of a ragged batch.  Values are 0 or finfo(float32).min, the contract of include/tgt_hip.h (never -inf).
  hard_logits   third-arm columns whose softmax is peaked and whose row maximum moves by tens of units from one key block to the
                next (E * 6, +12 on the keys of the upper half), gates that saturate (G * 4).

Plain helper: numpy and torch only, no pytest hooks or settings."""
import numpy as np
import torch

LO = torch.finfo(torch.float32).min

# B, N, num_nodes, C, H -- the smallest shapes that still reach each kernel family
CASES = {
    'S8': (2, 20, [20, 13], 128, 8),       # N <= 32, one 8-head group
    'S1': (2, 11, [11, 7], 48, 3),         # one-head workgroups, odd N
    'M': (2, 40, [40, 33], 64, 4),         # 33..64 nodes: the 16-wide kernels (16-bit), the two-tile 32-wide kernels (fp32)
    'K80': (2, 80, [80, 71], 64, 4),       # key-blocked, ragged
    'K128': (1, 128, [128], 32, 2),        # the upper limit: three leading key blocks closed, the maximum in the last
}
TRIANGULAR_CASES = {'T20': (2, 20, [20, 13], 16), 'T40': (1, 40, [33], 3)}      # B, N, num_nodes, H

# (first row, row step, width of the closed leading key block, smallest N it applies above)
LEADING_BLOCKS = [(1, 3, 16, 0), (2, 5, 32, 0), (3, 7, 64, 64), (4, 11, 96, 96)]


def leading_blocks(N):
    return [(s, st, w) for s, st, w, above in LEADING_BLOCKS if N > above]


def prefix_mask(num_nodes, N):
    """(B,N,N) float32: golden_util.additive_mask without its trailing axis -- 0 where both nodes are real, finfo.min elsewhere"""
    nm = torch.arange(N)[None, :] < torch.as_tensor(num_nodes)[:, None]
    em = (nm[:, :, None] & nm[:, None, :]).float()
    return (1 - em) * LO


def pair_mask(num_nodes, N, rng):
    """(B,N,N) float32 in {0, finfo.min}.  rng: a numpy Generator."""
    B = len(num_nodes)
    m = torch.zeros(B, N, N)
    m[torch.from_numpy(rng.random((B, N, N)) < 0.2)] = LO           # 1. a random fifth of the pairs
    for start, step, width in leading_blocks(N):                    # 2. inward: the key is the 2nd index
        m[:, start::step, :width] = LO
    for start, step, width in leading_blocks(N):                    # 3. outward: the key is the 1st index
        m[:, :width, start::step] = LO
    d = torch.arange(N)
    m[:, d, d] = 0.0                                                # 4. every real row / column keeps a live key
    return torch.minimum(m, prefix_mask(num_nodes, N))              # 5. padded rows and columns wholly closed, as the model builds them


def hard_logits(eg, H, N, gated):
    """eg: (B,N,N,2*nb) third-arm columns [E_in | G_in | E_out | G_out] (gated) or [E_in | E_out], BEFORE the cast to the test
    dtype.  Returns a new tensor: E * 6, +12 where the KEY index is >= N // 2, G * 4."""
    eg = eg.clone()
    nb = (2 if gated else 1) * H
    assert eg.shape[-1] == 2 * nb, (eg.shape, nb)
    for d in (0, 1):
        e = eg[..., d * nb: d * nb + H]
        e *= 6.0
        if d == 0:
            e[:, :, N // 2:] += 12.0          # inward: the key is the 2nd index
        else:
            e[:, N // 2:] += 12.0             # outward: the 1st
        if gated:
            eg[..., d * nb + H: (d + 1) * nb] *= 4.0
    return eg


def _seed(*key):
    """the same on every host and in every process (hash() of a string is not)"""
    return sum((i + 1) * sum(str(k).encode()) for i, k in enumerate(key)) % (2 ** 31)


def _rnd(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape))


def _width(used):
    return -(-used // 8) * 8           # rows of the fused projections are padded to 16 bytes (ops.TripletLayout / AggregateLayout)


def attention_inputs(case, dtype, variant, hard=True):
    """(fused (B,N,N,width) in dtype, d_out (B,N,N,2C) in dtype, mask (B,N,N) float32, used) in the row layout of
    ops.TripletLayout: [Q_in|K_in|V_in|Q_out|K_out|V_out|E_in|G_in|E_out|G_out|pad].  hard=False: the same shape with
    standard-normal columns and the prefix mask."""
    B, N, nn_, C, H = case
    gated, biased = variant == 'gated', variant != 'axial'
    nb = ((2 if gated else 1) * H) if biased else 0
    used = 6 * C + 2 * nb
    rng = np.random.default_rng(_seed('attention', B, N, C, H, variant))
    fused = _rnd(rng, B, N, N, _width(used))
    d_out = _rnd(rng, B, N, N, 2 * C)
    mask = pair_mask(nn_, N, rng)
    if hard and biased:
        fused[..., 6 * C:used] = hard_logits(fused[..., 6 * C:used], H, N, gated)
    return fused.to(dtype), d_out.to(dtype), (mask if hard else prefix_mask(nn_, N)), used


def aggregate_inputs(case, dtype, gated, hard=True):
    """as attention_inputs, in the row layout of ops.AggregateLayout: [V_in|V_out|E_in|G_in|E_out|G_out|pad] / [V_in|V_out|E_in|E_out|pad]"""
    B, N, nn_, C, H = case
    used = 2 * C + (4 if gated else 2) * H
    rng = np.random.default_rng(_seed('aggregate', B, N, C, H, gated))
    fused = _rnd(rng, B, N, N, _width(used))
    d_out = _rnd(rng, B, N, N, 2 * C)
    mask = pair_mask(nn_, N, rng)
    if hard:
        fused[..., 2 * C:used] = hard_logits(fused[..., 2 * C:used], H, N, gated)
    return fused.to(dtype), d_out.to(dtype), (mask if hard else prefix_mask(nn_, N)), used


def triangular_inputs(case, dtype, hard=True):
    """(e4, v4 (B,N,N,4H) in dtype: chunks [in_gate | in_lin | out_gate | out_lin]; d_out (B,N,N,2H); mask (B,N,N)); hard: the
    gate chunks * 4"""
    B, N, nn_, H = case
    rng = np.random.default_rng(_seed('triangular', B, N, H))
    e4, v4 = _rnd(rng, B, N, N, 4 * H), _rnd(rng, B, N, N, 4 * H)
    d_out = _rnd(rng, B, N, N, 2 * H)
    mask = pair_mask(nn_, N, rng)
    if hard:
        for t in (e4, v4):
            t[..., :H] *= 4.0
            t[..., 2 * H:3 * H] *= 4.0
    return e4.to(dtype), v4.to(dtype), d_out.to(dtype), (mask if hard else prefix_mask(nn_, N))
