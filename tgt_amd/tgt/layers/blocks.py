"""The blocks of one TGT layer on the HIP kernels: node attention with edge bias/gate,
logits-only edge update, FFN, DropPath and the layer wiring.  Class names, constructor
keywords and state_dict keys follow the reference (lib/tgt/layers/layers.py,
lib/tgt/layers/activations.py); the arithmetic is libtgt_hip.so plus library GEMMs."""
import contextlib

import torch
from torch import nn
import torch.nn.functional as F

from ... import ops
from ...knobs import K
from .triplet import get_triplet_layer


_CHAIN_NODE_STREAM = K.node_chain      # A/B knob (tgt_amd/knobs.py)
_TRI_SKIP = K.tri_skip != 0      # A/B knob: triplet kernels skip DropPath-dropped graphs


def _keep(module, **kw):
    """constructor keywords stay readable as attributes, as on the reference modules"""
    for k, v in kw.items():
        setattr(module, k, v)


class LayerNorm(nn.LayerNorm):
    """nn.LayerNorm parameters / state_dict keys, HIP forward+backward: reads the
    residual stream in its storage dtype and emits the consuming GEMM's dtype."""

    def forward(self, x):
        return ops.layer_norm(x, self.weight, self.bias, self.eps)


class Linear(nn.Linear):
    """nn.Linear parameters / state_dict keys; GEMMs through ops.linear (split-M weight gradient)."""

    def forward(self, x):
        return ops.linear(x, self.weight, self.bias)


class PendingResidual:
    """`res + DropPath(lin(x))` not yet computed: the edge residual that closes a layer is handed to the
    next layer un-added, together with the Linear (lin_W2 of the edge FFN) that feeds it, so that Linear,
    residual add and the LayerNorm that opens the next layer are ONE launch (ops.linear_residual_layer_norm).
    Only TGT_Encoder asks layers for this (defer_edge=True) and resolves the last one."""

    def __init__(self, x, lin, res, scale, prescaled=False):
        self.x, self.lin, self.res, self.scale = x, lin, res, scale
        self.prescaled = prescaled and scale is not None      # x already carries the DropPath factor (FFN.hidden(sample_scale=))

    def materialize(self):
        if self.prescaled:                                    # res + x' W^T + scale * b
            z = ops.linear(self.x, self.lin.weight, None)
            if self.lin.bias is not None:
                z = z + self.scale.view([-1] + [1] * (z.ndim - 1)).to(z.dtype) * self.lin.bias.to(z.dtype)
            return z.add_(self.res)
        return ops.scaled_add_(self.lin(self.x), self.res, self.scale)

    def enter(self, ln):
        """(res + lin(x)*scale, LayerNorm of it)"""
        return ops.linear_residual_layer_norm(self.x, self.lin.weight, self.lin.bias, self.res, self.scale,
                                              ln.weight, ln.bias, ln.eps, prescaled=self.prescaled)


class EGT_Attention(nn.Module):
    """Node attention biased and gated by edge channels.
    Reference lib/tgt/layers/layers.py:15-84."""

    def __init__(self, node_width, edge_width, num_heads, source_dropout=0,
                 scale_degree=True, edge_update=True):
        super().__init__()
        _keep(self, node_width=node_width, edge_width=edge_width, num_heads=num_heads,
              source_dropout=source_dropout, scale_degree=scale_degree, edge_update=edge_update)
        self._dot_dim, rem = divmod(node_width, num_heads)
        assert rem == 0, 'node_width must be divisible by num_heads'
        self._scale_factor = self._dot_dim ** -0.5

        self.mha_ln_h = LayerNorm(node_width)
        self.mha_ln_e = LayerNorm(edge_width)
        self.lin_QKV = Linear(node_width, node_width * 3)
        self.lin_EG = Linear(edge_width, num_heads * 2)
        self.lin_O_h = Linear(node_width, node_width)
        if edge_update:
            self.lin_O_e = Linear(num_heads, edge_width)

    def forward(self, h, e, mask):
        return self.forward_normed(h, self.mha_ln_e(e), mask, e)

    def project_nodes(self, h):
        """the node half of the block's input: lin_QKV(mha_ln_h(h)) (TGT_Layer runs it on the
        node stream, right behind the previous layer's node FFN)"""
        return self.lin_QKV(self.mha_ln_h(h))

    def forward_normed(self, h, e_hat, mask, e=None, qkv=None):
        """the block with mha_ln_e already applied (TGT_Layer fuses that LayerNorm with the
        residual add that closed the previous layer); e: returned as is without edge_update;
        qkv: project_nodes(h) when the caller already has it"""
        v_att, e = self.attend(h, e_hat, mask, e, qkv)
        return self.lin_O_h(v_att), e

    def attend(self, h, e_hat, mask, e=None, qkv=None, project_edges=True, hhat_scale=None, node_counts=None):
        """(V_att before lin_O_h, updated edge channels): forward_normed without the node output
        projection, which TGT_Layer runs on the node stream together with the node FFN.
        project_edges=False: return H_hat itself; the caller fuses lin_O_e with what follows it (hhat_scale: H_hat
        comes back multiplied by that per-graph factor, the DropPath of the branch it feeds)
        node_counts (B,) int32: ragged batches (ops.node_attention) -- every pair with a node >= node_counts[b] must be closed by
        the mask"""
        B, N = h.shape[0], h.shape[1]
        if qkv is None:
            qkv = self.project_nodes(h)
        eg = self.lin_EG(e_hat)
        mask3 = ops.as_mask3(mask, B, N)
        if self.source_dropout > 0 and self.training:
            # per-key-node drop shared by all queries/heads (layers.py:55-59); the
            # caller's mask is left untouched (the triplet module sees it un-dropped)
            mask3 = mask3 + ops.source_drop_mask(B, N, self.source_dropout, torch.finfo(mask.dtype).min, h.device)
        v_att, h_hat = ops.node_attention(qkv, eg, mask3, self.num_heads,
                                          self.scale_degree, self.edge_update, hhat_scale=hhat_scale, node_counts=node_counts)
        if self.edge_update:
            e = self.lin_O_e(h_hat) if project_edges else h_hat
        return v_att, e


class EdgeUpdate(nn.Module):
    """Edge channels from node dot products only.  Reference layers.py:87-130."""

    def __init__(self, node_width, edge_width, num_heads):
        super().__init__()
        _keep(self, node_width=node_width, edge_width=edge_width, num_heads=num_heads)
        self._dot_dim, rem = divmod(node_width, num_heads)
        assert rem == 0, 'node_width must be divisible by num_heads'
        self._scale_factor = self._dot_dim ** -0.5
        self.mha_ln_h = LayerNorm(node_width)
        self.mha_ln_e = LayerNorm(edge_width)
        self.lin_QK = Linear(node_width, node_width * 2)
        self.lin_E = Linear(edge_width, num_heads)
        self.lin_O_e = Linear(num_heads, edge_width)

    def forward(self, h, e, mask):
        return self.forward_normed(h, self.mha_ln_e(e), mask, e)

    def project_nodes(self, h):
        return self.lin_QK(self.mha_ln_h(h))

    def forward_normed(self, h, e_hat, mask, e=None, qkv=None):
        qk = self.project_nodes(h) if qkv is None else qkv
        bias = self.lin_E(e_hat)
        return h, self.lin_O_e(ops.edge_logits(qk, bias, self.num_heads))


_GLU_GATES = {            # name -> gate nonlinearity g(.) of  lin * g(gate)  (reference activations.py:4-17)
    'geglu': F.gelu,
    'glu': torch.sigmoid,
    'swiglu': F.silu,
}


def get_activation(activation):
    """(callable, width multiplier of lin_W1): GLU-family names split the projection into
    (gate, linear) halves, anything else is looked up in torch.nn.functional
    (reference lib/tgt/layers/activations.py:21-25)."""
    gate_fn = _GLU_GATES.get(activation)
    if gate_fn is None:
        return getattr(F, activation), 1

    def gated(x):
        gate, lin = x.chunk(2, dim=-1)
        return lin * gate_fn(gate)
    return gated, 2


class FFN(nn.Module):
    """Pre-norm MLP block: ffn_ln -> lin_W1 -> activation -> dropout -> lin_W2
    (reference lib/tgt/layers/layers.py:134-160)."""

    def __init__(self, width, multiplier=1., act_dropout=0., activation='gelu'):
        super().__init__()
        _keep(self, width=width, multiplier=multiplier, act_dropout=act_dropout, activation=activation)
        self.ffn_fn, self.act_mul = get_activation(activation)
        hidden = round(width * multiplier)
        self.ffn_ln = LayerNorm(width)
        self.lin_W1 = Linear(width, hidden * self.act_mul)
        self.lin_W2 = Linear(hidden, width)
        self.dropout = nn.Dropout(act_dropout)

    def forward(self, x):
        return self.forward_normed(self.ffn_ln(x))

    def forward_normed(self, x):
        """the block after ffn_ln (TGT_Layer fuses that LayerNorm with the residual add before it)"""
        return self.lin_W2(self.hidden(x))

    def hidden(self, x, sample_scale=None):
        """activation(lin_W1(x)) with dropout: the input of lin_W2 (TGT_Layer fuses lin_W2 with the residual add and
        the next LayerNorm).  sample_scale (B,): the result times that per-graph factor (the branch's DropPath, folded in)"""
        if self.activation == 'gelu' and ops.linear_gelu_dropout_ok(x, self.lin_W1.weight, sample_scale):
            return ops.linear_gelu_dropout(x, self.lin_W1.weight, self.lin_W1.bias, self.act_dropout, self.training, sample_scale)
        if self.activation in ops.GLU_KINDS:
            # gated activations: lin_W1 + activation + dropout as one launch on the edge rows (256 -> 512, 16-bit); any other
            # width, the node channel and fp32 take the library GEMM and one streaming pass each way
            if ops.linear_glu_dropout_ok(x, self.lin_W1.weight, sample_scale):
                return ops.linear_glu_dropout(x, self.lin_W1.weight, self.lin_W1.bias, self.activation, self.act_dropout,
                                              self.training, sample_scale)
            return ops.glu_dropout(self.lin_W1(x), self.activation, self.act_dropout, self.training, sample_scale)
        if self.activation in ops.ACT_KINDS:
            # relu / silu / elu: the same two forms -- one launch on the edge rows (K in {64,128,256} -> 256, 16-bit), else the library
            # GEMM and one streaming pass each way (the node FFN of width 768, fp32); the drop pattern is the kernels' own
            if ops.linear_act_dropout_ok(x, self.lin_W1.weight, sample_scale):
                return ops.linear_act_dropout(x, self.lin_W1.weight, self.lin_W1.bias, self.activation, self.act_dropout,
                                              self.training, sample_scale)
            return ops.act_dropout(self.lin_W1(x), self.activation, self.act_dropout, self.training, sample_scale)
        x = self.lin_W1(x)
        if self.activation == 'gelu' and x.dtype in (torch.float32, torch.bfloat16, torch.float16):
            return ops.gelu_dropout(x, self.act_dropout, self.training, sample_scale)      # one pass each way, no mask tensor
        x = self.dropout(self.ffn_fn(x))
        return x if sample_scale is None else x * sample_scale.view([-1] + [1] * (x.ndim - 1)).to(x.dtype)

    def can_fold_scale(self):
        return self.activation == 'gelu' or self.activation in ops.GLU_KINDS


class DropPath(nn.Module):
    """Stochastic depth per graph of the batch (reference lib/tgt/layers/layers.py:163-177).
    Inside TGT_Layer the factor is folded into the fused residual kernels
    (`ops.drop_path_scale`); this module form exists for API parity."""

    def __init__(self, drop_path=0.):
        super().__init__()
        self.drop_path = drop_path
        self._keep_prob = 1 - drop_path

    def forward(self, x):
        scale = ops.drop_path_scale(x, self.drop_path, self.training)
        if scale is None:
            return x
        return x * scale.view(-1, *([1] * (x.ndim - 1))).to(x.dtype)

    def extra_repr(self):
        return f'drop_path={self.drop_path}'


class TGT_Layer(nn.Module):
    """Reference lib/tgt/layers/layers.py:180-302."""

    def __init__(self, node_width, edge_width, num_heads, activation='gelu',
                 scale_degree=True, node_update=True, edge_update=True,
                 triplet_heads=0, triplet_type='aggregate', triplet_dropout=0,
                 node_ffn_multiplier=1., edge_ffn_multiplier=1., source_dropout=0,
                 drop_path=0, node_act_dropout=0, edge_act_dropout=0):
        super().__init__()
        _keep(self, node_width=node_width, edge_width=edge_width, num_heads=num_heads, activation=activation,
              scale_degree=scale_degree, node_update=node_update, edge_update=edge_update,
              triplet_heads=triplet_heads, triplet_type=triplet_type, triplet_dropout=triplet_dropout,
              node_ffn_multiplier=node_ffn_multiplier, edge_ffn_multiplier=edge_ffn_multiplier,
              source_dropout=source_dropout, node_act_dropout=node_act_dropout, edge_act_dropout=edge_act_dropout)
        self._triplet_update = triplet_heads > 0
        if not (node_update or edge_update):
            raise ValueError('At least one of node_update and edge_update must be True')

        if node_update:
            self.update = EGT_Attention(node_width=node_width, edge_width=edge_width,
                                        num_heads=num_heads, source_dropout=source_dropout,
                                        scale_degree=scale_degree, edge_update=edge_update)
            self.node_ffn = FFN(width=node_width, multiplier=node_ffn_multiplier,
                                act_dropout=node_act_dropout, activation=activation)
        else:                       # last layer of an edge-ended model: logits-only edge update
            self.update = EdgeUpdate(node_width=node_width, edge_width=edge_width, num_heads=num_heads)
        if edge_update:
            if self._triplet_update:
                self.tria = get_triplet_layer(triplet_type)(edge_width=edge_width,
                                                            num_heads=triplet_heads,
                                                            attention_dropout=triplet_dropout)
            self.edge_ffn = FFN(width=edge_width, multiplier=edge_ffn_multiplier,
                                act_dropout=edge_act_dropout, activation=activation)
        self.drop_path = DropPath(drop_path)

    def forward(self, g, defer_edge=False):
        """defer_edge (TGT_Encoder only): leave the closing edge residual un-added in g.e (a
        PendingResidual) for the next layer's opening LayerNorm, and leave the node stream
        un-joined (g.node_side) so that the next layer's node projection follows this layer's node
        FFN on it; TGT_Encoder resolves both after the last layer."""
        h, e, mask = g.h, g.e, g.mask
        side = g.get('node_side')            # h was produced on the node stream and is not joined yet
        qkv = None
        if side is not None:
            with side.resume():
                qkv = self.update.project_nodes(h)
        if isinstance(e, PendingResidual):
            e, e_hat = e.enter(self.update.mha_ln_e)
        else:
            e_hat = self.update.mha_ln_e(e)
        if side is not None:
            side.join(h, qkv)
        h_in, e_in = h, e
        fuse_oe = self.node_update and self.edge_update          # lin_O_e joins the entry of the next edge sub-block
        dp, tr = self.drop_path.drop_path, self.training
        # DropPath folded into the branch's PRODUCER where that is free (H_hat out of the node attention kernel, the FFN's
        # activation): the factor is drawn before the branch runs and the closing Linear + residual add then need no scaled
        # copy of the stream gradient in the backward (ops.linear_residual_layer_norm(prescaled=True))
        cd = torch.get_autocast_dtype('cuda') if (e_hat.is_cuda and torch.is_autocast_enabled('cuda')) else e_hat.dtype
        pair_rows = e_hat.numel() // e_hat.shape[-1]
        sc_oe = ops.drop_path_scale(e_hat, dp, tr) if fuse_oe else None      # (drawn here whether it is folded or not)
        fold_oe = sc_oe is not None and ops.can_prescale(pair_rows, self.update.num_heads, e_hat.shape[-1], cd)
        if self.node_update:
            # (ragged batches under TGT_NODE_RAGGED: TGT_Encoder marks the graph when the counts bound rows and columns of the mask)
            v_att, e = self.update.attend(h, e_hat, mask, e, qkv, project_edges=not fuse_oe,
                                          hhat_scale=sc_oe if fold_oe else None,   # lin_O_h follows on the node stream
                                          node_counts=g.get('node_counts') if g.get('node_ragged') else None)
        else:
            h, e = self.update.forward_normed(h, e_hat, mask, e, qkv)
        # Each residual add is fused with the LayerNorm that opens the next sub-block
        # (s = res + DropPath(x); y = LN(s) in one pass, and one pass in the backward).

        def enter(x, res, ln, lin=None, scale=None, folded=False):
            """(s, LayerNorm(s)) with s = res + DropPath(x), or res + DropPath(lin(x)) in one launch
            (scale: the factor when it was drawn earlier; folded: x already carries it)"""
            if lin is not None:
                sc = scale if scale is not None else ops.drop_path_scale(x, dp, tr)
                return ops.linear_residual_layer_norm(x, lin.weight, lin.bias, res, sc, ln.weight, ln.bias, ln.eps,
                                                      prescaled=folded)
            return ops.add_layer_norm(x, res, scale if scale is not None else ops.drop_path_scale(x, dp, tr), ln.weight, ln.bias, ln.eps)

        node_side = None
        if self.node_update:
            # the node FFN (a dozen latency-bound launches on 8192 rows) runs under the edge
            # kernels of this layer on a second stream; joined before the layer returns
            node_side = ops.side_stream(v_att, h_in) if self.edge_update else None
            with (node_side if node_side is not None else contextlib.nullcontext()):
                h = self.update.lin_O_h(v_att)
                h, x = enter(h, h_in, self.node_ffn.ffn_ln)
                h = ops.drop_path_add_(self.node_ffn.forward_normed(x), h, dp, tr)
        if self.edge_update:
            lin_oe = self.update.lin_O_e if fuse_oe else None        # then `e` is still H_hat
            if self._triplet_update:
                e, x = enter(e, e_in, self.tria.tri_ln_e, lin_oe, sc_oe, fold_oe)
                # the triplet branch's DropPath factor is drawn BEFORE the branch runs: the attention kernels skip the
                # graphs it drops (zeros out, zero gradients -- what the multiplication at the residual add gives anyway)
                sc_tri = ops.drop_path_scale(x, dp, tr) if (_TRI_SKIP and getattr(self.tria, 'takes_graph_scale', False)) else None
                tri_kw = {} if sc_tri is None else {'graph_scale': sc_tri}
                # ragged batches (TGT_TRI_RAGGED, TGT_Encoder): per-graph node counts -- the attention kernels skip the padded nodes
                if g.get('node_counts') is not None and getattr(self.tria, 'takes_node_counts', False):
                    tri_kw['node_counts'] = g['node_counts']
                if hasattr(self.tria, 'out_proj_residual_ln'):
                    # lin_O + DropPath + residual + the edge FFN's LayerNorm as one launch (K = 512 row kernel; the same two-step
                    # composition where the shape does not qualify)
                    va = self.tria.attend(x, mask, **tri_kw)
                    e, x = self.tria.out_proj_residual_ln(va, e, sc_tri if sc_tri is not None else ops.drop_path_scale(va, dp, tr),
                                                          self.edge_ffn.ffn_ln)
                else:
                    e, x = enter(self.tria.forward_normed(x, mask, **tri_kw), e, self.edge_ffn.ffn_ln, scale=sc_tri)
            else:
                e, x = enter(e, e_in, self.edge_ffn.ffn_ln, lin_oe, sc_oe, fold_oe)
            sc_ffn = ops.drop_path_scale(x, dp, tr)
            fold = (sc_ffn is not None and self.edge_ffn.can_fold_scale() and
                    ops.can_prescale(pair_rows, self.edge_ffn.lin_W2.weight.shape[1], self.edge_ffn.lin_W2.weight.shape[0], cd))
            closing = PendingResidual(self.edge_ffn.hidden(x, sc_ffn if fold else None), self.edge_ffn.lin_W2, e, sc_ffn, prescaled=fold)
            e = closing if defer_edge else closing.materialize()
        g = g.copy()
        g.pop('node_side', None)
        if node_side is not None:
            if defer_edge and _CHAIN_NODE_STREAM:
                g['node_side'] = node_side       # joined by the next layer (or TGT_Encoder)
            else:
                node_side.join(h)
        g.h, g.e = h, e
        return g

    def extra_repr(self):
        return f'activation={self.activation}, source_dropout={self.source_dropout}'
