"""Kernel-level A/B of the live tile lists (tgt_edge_linear_live): the persistent edge row kernels at the ragged
benchmark shape (B 256, N 32, node counts U{16..32}) without a list, with a list whose tiles are all live (what the walk itself
costs) and with the ragged list.  HIP events around 30 back-to-back launches, best of 3 rounds, bf16.
    python tools/edge_live_bench.py"""
import math
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tgt_amd import _lib, ops
torch.manual_seed(0)
B, N = 256, 32
M = B * N * N
dt = torch.bfloat16
counts = torch.randint(16, 33, (B,), dtype=torch.int32).cuda()
live = ops.edge_live_tiles(counts, N)
full = ops.edge_live_tiles(torch.full((B,), N, dtype=torch.int32).cuda(), N)
print('live tiles', int(live.tiles[0]), 'of', live.tiles.numel() - 1, flush=True)
def mk(K, Nn):
    return torch.randn(M, K, device='cuda').to(dt), (torch.randn(Nn, K, device='cuda') / math.sqrt(K)).to(dt), torch.randn(Nn, device='cuda').to(dt)
res = torch.randn(M, 256, device='cuda').to(dt)
ds = torch.randn(M, 256, device='cuda').to(dt)
gamma, beta = torch.rand(256, device='cuda') + 0.5, torch.randn(256, device='cuda')
mean, rstd = torch.zeros(M, device='cuda'), torch.ones(M, device='cuda')
sc = torch.ones(B, device='cuda')
o1, o2, y = (torch.empty(M, 256, dtype=dt, device='cuda') for _ in range(3))
o512 = torch.empty(M, 512, dtype=dt, device='cuda')
L = _lib.lib()
a256, w256, b256 = mk(256, 256)
a512, w512, b512 = mk(512, 256)
aw, ww, bw = mk(256, 512)
cs1 = torch.empty(L.tgt_edge_linear_parts(M, 256), 256, device='cuda')
cs3 = torch.empty(L.tgt_edge_linear_parts(M, 256), 768, device='cuda')
cases = {
    'resid+LN K=256': lambda lv: ops.edge_linear_raw(a256, w256, b256, _lib.EPI_RESID, out=o1, res=res, row_scale=sc, rows_per_sample=N * N, ln=(gamma, beta, 1e-5), stats=(mean, rstd), y=y, live=lv),
    'gelu K=256': lambda lv: ops.edge_linear_raw(a256, w256, b256, _lib.EPI_GELU, out=o1, out2=o2, dropout=(0.1, 7), row_scale=sc, rows_per_sample=N * N, live=lv),
    'gelu_bwd': lambda lv: ops.edge_linear_raw(a256, w256, None, _lib.EPI_GELU_BWD, out=o1, res=res, dropout=(0.1, 7), colsum_partial=cs1, live=lv),
    'ln_bwd K=256': lambda lv: ops.edge_linear_raw(a256, w256, None, _lib.EPI_LN_BWD, ln=(gamma, None, 1e-5), stats=(mean, rstd), res=res, ds_in=ds, out=o1, out2=o2, row_scale=sc, rows_per_sample=N * N, colsum_partial=cs3, live=lv),
    'resid+LN K=512': lambda lv: ops.edge_linear_raw(a512, w512, b512, _lib.EPI_RESID, out=o1, res=res, row_scale=sc, rows_per_sample=N * N, ln=(gamma, beta, 1e-5), stats=(mean, rstd), y=y, live=lv),
    'wide 256->512': lambda lv: ops.edge_linear_raw(aw, ww, bw, out=o512, live=lv),
}
def t(fn, lv, n=30):
    for _ in range(5): fn(lv)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn(lv)
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n
for name, fn in cases.items():
    r = []
    for rnd in range(3):
        r.append((t(fn, None), t(fn, full), t(fn, live)))
    best = [min(x[i] for x in r) for i in range(3)]
    print('%-16s no list %.4f ms | list, all live %.4f | list, ragged %.4f  (%.1f %% of no list)' % (name, *best, 100 * best[2] / best[0]), flush=True)
