"""hipGraph replay of an inference forward.

A small-batch forward of a 24-layer TGT model is launch-bound: ~2400 kernels of a few microseconds each behind a Python
dispatch of 5-10 us per launch (BASELINE config 1: 8 graphs).  `GraphedForward` captures ONE forward of a task model
into a HIP graph through torch.cuda.CUDAGraph and replays it on new inputs of the same shapes: one graph launch instead of
thousands of kernel launches.  The kernels are the same libtgt_hip.so kernels on the same stream order; outputs are bit-identical
to the eager forward (tests/test_hip_predict.py).  The reference has no counterpart (its forward is eager PyTorch); this is the
MI355X form of its `prediction_loop` inner call for small batches (lib/training/training.py:700-722).

Dropout.  By default the dropout kernels take seeds the host draws at capture time, so a replayed train-mode forward repeats the
captured drop pattern: such a model is refused (`allow_frozen_dropout=True` is for probes).  `stochastic=True` is the mode for
MC-dropout prediction (prediction_loop(predict_in_train=True), the schemes' default: S stochastic forwards of one batch): the
object takes the process's graph-safe random mode the way training/graphed.py does -- host seeds become a function of the call's
position inside the forward (ops.graph_safe_rng), a device counter the graph bumps first enters every kernel's seed
(ops.set_seed_counter; the triplet attention dropout included), DropPath factors and source-dropout masks are drawn by torch's
capture-aware generator -- so every replay draws new patterns in every dropout of the model.  `load(batch)` copies the inputs,
`sample()` only replays: the S samples of one batch need one input copy.  An eager
`counter.add_(1); ops.begin_step(); model(batch)` in that mode (eager_graph_safe_forward) computes exactly what a replay computes
(tests/test_hip_graphed_mc.py).

`GraphedSampler` puts one complete TRY of the MC prediction steps of pcqm/predict.py into the graph: the forward plus the
sample's device-side bookkeeping (accept / skip of a non-finite sample included), on accumulators allocated before the capture.
"""
import weakref

import torch

from .. import ops


def _stochastic(model):
    """does any sub-module carry a positive dropout / drop-path rate?"""
    for m in model.modules():
        for name in ('p', 'drop_prob', 'drop_path', 'source_dropout', 'act_dropout', 'attention_dropout', 'triplet_dropout'):
            v = getattr(m, name, 0)
            if isinstance(v, (int, float)) and not isinstance(v, bool) and v > 0:
                return True
    return False


def _leave_graph_mode(counter):
    """back to eager: host seeds and pooled DropPath draws.  Shared by close(), by the failure path of a capture and by the
    finalizer of an owner dropped without close().  `counter` is the ownership token (as training/graphed.py): the mode is only
    given back while the registered seed counter is still this owner's."""
    if ops._seed_counter[0] is not counter:
        return
    ops.set_seed_counter(None)
    ops.graph_safe_rng(False)


def eager_graph_safe_forward(model, counter, batch):
    """one eager forward in graph-safe mode -- exactly what a replay of a GraphedForward(stochastic=True) computes.  The caller
    holds the mode (ops.graph_safe_rng(True), ops.set_seed_counter(counter)), no_grad and the autocast."""
    counter.add_(1)
    ops.begin_step()
    return model(batch)


class GraphedForward:
    """stochastic=True: see the module docstring.  counter: the device counter of ANOTHER open stochastic owner whose mode this
    object shares without owning it (the two models of two_stage_predict); that owner is closed last."""

    def __init__(self, model, example_batch, autocast_dtype=None, warmup=3, allow_frozen_dropout=False, stochastic=False,
                 counter=None):
        if model.training and not allow_frozen_dropout and not stochastic and _stochastic(model):
            # the dropout kernels take host-drawn seeds: a captured train-mode forward replays ONE drop pattern, so S
            # "Monte-Carlo samples" through it would be S copies of the same sample (prediction_loop(predict_in_train=True))
            raise RuntimeError('GraphedForward: the model is in train mode with dropout / drop_path > 0 -- a replay would repeat '
                               'the captured dropout pattern.  Capture in eval mode, pass stochastic=True (fresh patterns per '
                               'replay), or pass allow_frozen_dropout=True.')
        if counter is not None and not stochastic:
            raise RuntimeError('GraphedForward: counter= belongs to stochastic=True')
        self.model, self.autocast_dtype, self.stochastic = model, autocast_dtype, bool(stochastic)
        self.static_in = {k: v.clone() for k, v in example_batch.items()}
        self.counter, self._finalizer, self._closed = None, None, False
        if stochastic:
            held = ops._seed_counter[0]
            if counter is None:
                if held is not None or ops._GRAPH_SAFE[0]:
                    raise RuntimeError('GraphedForward(stochastic=True): the graph-safe random mode already has an owner (a '
                                       'registered seed counter); close it first, or share its counter (counter=)')
                dev = next(iter(self.static_in.values())).device
                self.counter = torch.zeros(1, dtype=torch.int64, device=dev)
                ops.graph_safe_rng(True)
                ops.set_seed_counter(self.counter)
                # an owner dropped without close() must not leave the process in graph-safe mode
                self._finalizer = weakref.finalize(self, _leave_graph_mode, self.counter)
            else:
                if held is not counter or not ops._GRAPH_SAFE[0]:
                    raise RuntimeError('GraphedForward(stochastic=True, counter=...): that counter is not the registered one')
                self.counter = counter
        try:
            self._allocate()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(warmup):                 # allocator, TunableOp decisions, lazy attribute memos: before capture
                    self._body()
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_out = self._body()
        except BaseException:
            # warm-up or capture failed: give the mode back before the error travels on
            self._closed = True
            self.graph = self.static_out = None
            if self._finalizer is not None:
                self._finalizer()
            raise

    def _allocate(self):
        """static tensors of the captured body besides the inputs (before the warm-up; GraphedSampler's accumulators)"""

    # what the graph holds
    def _body(self):
        if self.stochastic:
            self.counter.add_(1)
            ops.begin_step()            # host side, at trace time: the per-call seed positions of an eager forward
        return self._forward()

    def _forward(self):
        ctx = (torch.autocast('cuda', dtype=self.autocast_dtype) if self.autocast_dtype is not None
               else torch.autocast('cuda', enabled=False))
        with torch.no_grad(), ctx:
            return self._run()

    def _run(self):
        return self.model(self.static_in)

    def load(self, batch):
        """copy `batch` (same keys, shapes and dtypes as the example) into the static inputs; nothing is launched besides"""
        if self._closed:
            raise RuntimeError('GraphedForward is closed')
        if batch.keys() != self.static_in.keys():          # a missing key would silently replay the example's data
            raise RuntimeError(f'GraphedForward: batch keys {sorted(batch)} differ from the captured {sorted(self.static_in)}')
        for k, v in batch.items():
            dst = self.static_in[k]
            if dst.shape != v.shape or dst.dtype != v.dtype:
                raise RuntimeError(f'GraphedForward: input {k} is {tuple(v.shape)} {v.dtype}, captured {tuple(dst.shape)} {dst.dtype}')
            dst.copy_(v, non_blocking=True)

    def sample(self):
        """one replay on the loaded inputs (stochastic: a new draw of every dropout); returns the graph's static outputs"""
        if self._closed:
            raise RuntimeError('GraphedForward is closed')
        self.graph.replay()
        return self.static_out

    def __call__(self, batch):
        """the model's output for `batch` (same keys, shapes and dtypes as the example); the returned tensors are the graph's
        static outputs: clone them if they must survive the next call"""
        self.load(batch)
        return self.sample()

    def close(self):
        """drop the graph; a stochastic owner hands the mode back (host seeds, pooled draws)"""
        if not self._closed:
            self._closed = True
            if self._finalizer is not None:
                self._finalizer()            # runs _leave_graph_mode once; a later garbage collection does nothing
            self.graph = self.static_out = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class GraphedSampler(GraphedForward):
    """One complete try of an MC prediction step as one graph replay: the stochastic forward AND the sample's device-side
    bookkeeping, for predict_bins ('bins'), predict_probs ('probs') and gap_prediction_step ('gap') of pcqm/predict.py, which take
    it through their `graphed=` keyword.  One capture per (model, batch shape, kind, nb_samples).

    Nothing in a try reads device state on the host: the accept / skip decision of a sample, the sample's slot in the output and
    the gap predictor's `valid % num_dist_inputs` input choice are functions of the state vector `state` {valid, nonfinite,
    tries, -} evaluated by the kernels (tgt_sample_commit, tgt_gap_commit) and by an index_select on a device index.  The host
    reads state[0] where predict._sample_loop always did: once after the S tries it certainly needs, then after each further try.

    The accumulators (`out` -- bins (B,S,N,N) / gap predictions (B,S) --, `acc`, `state`) are allocated before the capture and are
    static: reset() zeroes them for the next batch, and the predict functions return CLONES of the results."""

    def __init__(self, model, example_batch, nb_samples, kind, autocast_dtype=None, warmup=3, counter=None):
        if kind not in ('bins', 'probs', 'gap'):
            raise ValueError(f"GraphedSampler: kind {kind!r}; 'bins', 'probs' or 'gap'")
        self.kind, self.nb_samples = kind, int(nb_samples)
        self.out = self.acc = self.state = None
        warmup = max(1, warmup)                          # (the first forward sizes the accumulators: before the capture)
        if kind == 'gap' and example_batch['dist_input'].ndim != 4:
            raise RuntimeError('GraphedSampler: a gap sampler takes dist_input (B, num_dist_inputs, N, N)')
        super().__init__(model, example_batch, autocast_dtype=autocast_dtype, warmup=warmup, stochastic=True, counter=counter)
        self.reset()                                     # (the warm-up tries committed samples)

    def _allocate(self):
        dev = next(iter(self.static_in.values())).device
        self.state = torch.zeros(4, dtype=torch.int32, device=dev)
        if self.kind == 'gap':
            self._gap_batch = dict(self.static_in)
            self.out = torch.zeros(self.static_in['dist_input'].shape[0], self.nb_samples, dtype=torch.float32, device=dev)

    def _run(self):
        from . import predict
        if self.kind == 'gap':
            return predict._gap_try(self.model, self._gap_batch, self.static_in['dist_input'], self.out, self.state,
                                    self.nb_samples)
        logits = self.model(self.static_in)
        if self.kind == 'bins':
            if self.out is None:                         # first warm-up forward: the logits' shape is known now
                B, N, _, NB = logits.shape
                self.out = torch.empty(B, self.nb_samples, N, N, dtype=predict.bins_dtype(NB), device=logits.device)
            predict._bins_try(logits, self.out, self.state, self.nb_samples)
        else:
            if self.acc is None:
                self.acc = torch.zeros(logits.shape, dtype=torch.float32, device=logits.device)
            predict._probs_try(logits, self.acc, self.state, self.nb_samples)
        return logits

    def reset(self):
        """empty accumulators for the next batch (device-side fills; the counter and torch's generator go on)"""
        self.state.zero_()
        if self.acc is not None:
            self.acc.zero_()
        if self.kind == 'gap':
            self.out.zero_()

    def check(self, model, nb_samples, kind):
        if self._closed:
            raise RuntimeError('GraphedSampler is closed')
        if model is not self.model or int(nb_samples) != self.nb_samples or kind != self.kind:
            raise RuntimeError(f'GraphedSampler: captured for kind {self.kind!r}, nb_samples {self.nb_samples} and its own model; '
                               f'asked for {kind!r}, {nb_samples}' + ('' if model is self.model else ' and another model'))

    def close(self):
        super().close()
        self.out = self.acc = self.state = None
