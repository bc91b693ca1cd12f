#!/usr/bin/env python
"""Secondary benchmark lines: forward-only graphs/s of the two inference configurations of BASELINE.json
on one MI355X.  One JSON line per configuration.

  cfg1  TGT-Agx2 12x2 distance predictor (256 bins), PCQM4Mv2-like val mini-batch of 8 ragged graphs (N <= 32), eval
        forward -- the reference's CPU-runnable case, here on the GPU in fp32 (and bf16 autocast)
  cfg5  TGT-Agx2 two-stage end-to-end inference, fp16 autocast, batch 512, N = 32: S stochastic forwards (dropout ON,
        predict_in_train) of TGT_Distance -> argmax bins of the symmetrised softmax -> bins2dist on the device ->
        S stochastic forwards of TGT_Gap, one per bins sample (tgt_amd/pcqm/predict.py::two_stage_predict)

  mc    (opt-in: --only mc)  MC-dropout prediction of one small batch: train mode (predict_in_train), bf16 autocast, --mc-graphs
        graphs of --nodes nodes, predict_bins with --samples stochastic forwards per batch, on TGT-At 24L and TGT-Agx2 12x2 distance
        predictors: the eager loop against one graph replay per sample (pcqm/graphed.py::GraphedSampler), alternating in one
        process, --reps repetitions each; median and spread (min..max) of the time per batch

python tools/infer_bench.py [--samples 4] [--batch 512] [--steps 3] [--nodes 32]
python tools/infer_bench.py --only mc --samples 10 [--mc-graphs 8] [--nodes 32] [--reps 7]
(--nodes: the padded node count of cfg5's batch; above 32 the aggregate forward is tgt_triplet_aggregate_proj64_fwd,
TGT_AGG_PROJ64_INFER=0 is the A/B knob and `knobs` in the line says which side ran.  --only tgt_at honours --nodes and --batch
too: above 32 nodes its triplet forward is tgt_triplet_attention_proj64_fwd, TGT_TRI_PROJ64_INFER=0 is the A/B knob)
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tgt_amd import knobs, ops                                       # noqa: E402
from tgt_amd.pcqm import TGT_Distance, TGT_Gap, predict as pp        # noqa: E402
from tgt_amd.training import configs, gemm_tuning                   # noqa: E402
from tgt_amd.training.synthetic import make_batch                    # noqa: E402


def device_batch(graphs, nodes, seed, ragged):
    b = {k: v.cuda() for k, v in make_batch(graphs, nodes, seed, ragged=ragged).items()}
    nm = b['node_mask']
    b['edge_mask'] = nm.unsqueeze(-1) * nm.unsqueeze(-2)
    c = b['dft_coords']
    b['dist_input'] = torch.norm(c.unsqueeze(-2) - c.unsqueeze(-3), dim=-1)
    return b


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=4, help='MC samples per stage of cfg5 (the shipped configs use 50)')
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--nodes', type=int, default=32, help='padded node count of the cfg5 batch (the BASELINE shape is 32)')
    ap.add_argument('--only', default='')
    ap.add_argument('--mc-graphs', type=int, default=8, help='graphs of the mc batch')
    ap.add_argument('--reps', type=int, default=7, help='repetitions per side of the mc comparison')
    a = ap.parse_args()
    gemm_tuning.enable_gemm_tuning(online=True)
    torch.manual_seed(0)

    if not a.only or 'cfg1' in a.only.split(','):
        kw = configs.tgt_agx2_12x2(num_dist_bins=256, embed_3d_type='none')       # coords_input: none (tgt_agx2_dp_nordkit.yaml)
        model = TGT_Distance(**kw).cuda().eval()
        batch = device_batch(8, 32, 11, ragged=True)
        for prec in ('fp32', 'bf16'):
            ctx = torch.autocast('cuda', dtype=torch.bfloat16) if prec == 'bf16' else torch.autocast('cuda', enabled=False)

            def fwd():
                with torch.no_grad(), ctx:
                    model(batch)
            dt = timed(fwd, 3, 20)
            line = dict(metric='graphs/sec forward, TGT-Agx2 12x2 dist-predictor, 8-graph ragged val mini-batch (cfg 1)',
                        value=round(8 / dt, 1), unit='graphs/s', ms_per_forward=round(dt * 1e3, 3), dtype=prec, n_gpus=1,
                        data='synthetic', launch='eager')
            print(json.dumps(line), flush=True)
            from tgt_amd.pcqm.graphed import GraphedForward
            gf = GraphedForward(model, batch, autocast_dtype=torch.bfloat16 if prec == 'bf16' else None)
            with torch.no_grad(), ctx:
                want = model(batch)
            same = bool(torch.equal(gf(batch), want))
            dt = timed(lambda: gf(batch), 3, 50)
            line.update(value=round(8 / dt, 1), ms_per_forward=round(dt * 1e3, 3), launch='hipGraph replay', bit_identical_to_eager=same)
            print(json.dumps(line), flush=True)
        del model

    if not a.only or 'cfg5' in a.only.split(','):
        S, B = a.samples, a.batch
        dk = configs.tgt_agx2_12x2(num_dist_bins=256, embed_3d_type='none')
        gk = configs.tgt_agx2_12x2(num_dist_bins=256, embed_3d_type='gaussian')
        gk.pop('num_dist_bins')
        dist_model = TGT_Distance(**dk).cuda().train()                                # predict_in_train: dropout ON
        gap_model = TGT_Gap(**gk).cuda().train()
        batch = device_batch(B, a.nodes, 12, ragged=False)
        batch['num_nodes'] = batch['node_mask'].sum(-1).long()
        # (events only around the attention kernels, one launch in three: an event pair around every launch slows the host AND the queue,
        #  DESIGN.md 5.2)
        prof = ops.profile_kernels(True, only=('tgt_triplet_aggregate_fwd', 'tgt_triplet_aggregate_proj_fwd', 'tgt_triplet_aggregate_proj64_fwd', 'tgt_node_attention_fwd', 'tgt_node_attention_fwd(logits)'), stride=3)

        def run():
            return pp.two_stage_predict(dist_model, gap_model, batch, S, 256, 8, autocast_dtype=torch.float16)
        dt = timed(run, 1, a.steps)
        ops.profile_kernels(False)
        bins, gap = run()
        kt = {k: round(sum(v) / len(v), 4) for k, v in ops.kernel_times_ms(prof).items()}
        print(json.dumps(dict(metric=f'graphs/sec end-to-end two-stage inference, TGT-Agx2 12x2 (dist+gap), fp16, batch {B} (cfg 5)',
                              value=round(B / dt, 1), unit='graphs/s', ms_per_batch=round(dt * 1e3, 2), dtype='fp16',
                              mc_samples_per_stage=S, stochastic_forwards_per_batch=2 * S,
                              graph_forwards_per_s=round(2 * S * B / dt, 1), n_gpus=1, data='synthetic',
                              gap_finite=bool(torch.isfinite(gap).all()), kernel_ms=kt, batch=B, nodes=a.nodes,
                              knobs=knobs.K.non_default())), flush=True)

    if 'tgt_at' in a.only:
        # (opt-in: --only tgt_at)  TGT-At 24L, the training benchmark's model, as a forward without autograd: eval mode, bf16
        # autocast, 256 graphs of 32 nodes -- the forward whose triplet kernel leaves its Q/K/V stores out
        # (TGT_TRI_PROJ_INFER=0 is the A/B knob; `knobs` in the line says which side ran)
        from tgt_amd.knobs import K
        from tgt_amd.pcqm import TGT_Multi
        # --nodes / --batch: the padded node count and the graphs of the batch (--batch is capped at 256, the benchmark's batch).  33..64
        # nodes: the forward is tgt_triplet_attention_proj64_fwd; TGT_TRI_PROJ64_INFER=0 (GEMMs + tgt_triplet_attention_fwd) is the A/B knob
        B, Nn = min(a.batch, 256), a.nodes
        model = TGT_Multi(**configs.tgt_at_24l(dropouts=False)).cuda().eval()
        batch = device_batch(B, Nn, 13, ragged=False)
        prof = ops.profile_kernels(True, only=('tgt_triplet_attention_proj_fwd', 'tgt_triplet_attention_proj64_fwd', 'tgt_triplet_attention_fwd'), stride=3)

        def fwd_at():
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                model(batch)
        dt = timed(fwd_at, 3, max(a.steps, 10))
        ops.profile_kernels(False)
        kt = {k: round(sum(v) / len(v), 4) for k, v in ops.kernel_times_ms(prof).items()}
        print(json.dumps(dict(metric=f'graphs/sec forward, TGT-At 24L, bf16, batch {B}, N = {Nn}, no autograd', value=round(B / dt, 1),
                              unit='graphs/s', ms_per_forward=round(dt * 1e3, 3), dtype='bf16', n_gpus=1, data='synthetic',
                              launch='eager', kernel_ms=kt, batch=B, nodes=Nn, knobs=K.non_default())), flush=True)

    if 'mc' in a.only.split(','):
        import statistics
        from tgt_amd.pcqm.graphed import GraphedSampler
        S, B, Nn = a.samples, a.mc_graphs, a.nodes
        for name, kw in (('TGT-At 24L', configs.tgt_at_24l(num_dist_bins=256)), ('TGT-Agx2 12x2', configs.tgt_agx2_12x2(num_dist_bins=256))):
            model = TGT_Distance(**kw).cuda().train()                                 # predict_in_train: every dropout ON
            batch = device_batch(B, Nn, 14, ragged=True)

            def eager():
                with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                    return pp.predict_bins(model, batch, S)
            eager()                                                                   # GEMM plans, allocator
            times = dict(eager=[], graphed=[])
            with GraphedSampler(model, batch, S, 'bins', autocast_dtype=torch.bfloat16) as gs:
                def graphed():
                    return pp.predict_bins(model, batch, S, graphed=gs)
                bins = graphed()
                distinct = len({bins[:, s].cpu().numpy().tobytes() for s in range(S)})
                for _ in range(max(1, a.reps)):                                       # alternating: both sides see the same clocks
                    times['graphed'].append(timed(graphed, 1, a.steps))
                    # the eager side as it runs without a sampler: host seeds, pooled DropPath draws (a replay keeps the counter it
                    # captured, so the mode can be lent out between replays)
                    ops.set_seed_counter(None)
                    ops.graph_safe_rng(False)
                    try:
                        times['eager'].append(timed(eager, 1, a.steps))
                    finally:
                        ops.graph_safe_rng(True)
                        ops.set_seed_counter(gs.counter)
            med = {k: statistics.median(v) for k, v in times.items()}
            print(json.dumps(dict(metric=f'ms per MC-dropout predict_bins batch, {name} distance predictor, train mode, bf16, {B} graphs, '
                                         f'N = {Nn}, {S} samples', unit='ms', dtype='bf16', n_gpus=1, data='synthetic', graphs=B, nodes=Nn,
                                  samples=S, reps=len(times['eager']), batches_per_rep=a.steps,
                                  eager_ms=dict(median=round(med['eager'] * 1e3, 3), min=round(min(times['eager']) * 1e3, 3),
                                                max=round(max(times['eager']) * 1e3, 3)),
                                  graphed_ms=dict(median=round(med['graphed'] * 1e3, 3), min=round(min(times['graphed']) * 1e3, 3),
                                                  max=round(max(times['graphed']) * 1e3, 3)),
                                  speedup=round(med['eager'] / med['graphed'], 3), distinct_samples=distinct,
                                  samples_per_s_graphed=round(S * B / med['graphed'], 1), knobs=knobs.K.non_default())), flush=True)
            del model


if __name__ == '__main__':
    main()
