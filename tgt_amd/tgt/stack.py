"""The layer stack (`TGT_Encoder`) and the attribute-style batch container (`Graph`).
Same public behaviour and state_dict prefixes (`TGT_layers.{i}.`) as the reference's
lib/tgt/encoder.py."""
import torch
from torch import nn

from .. import ops
from ..knobs import K
from .layers import TGT_Layer
from .layers.blocks import PendingResidual


_DEFER_EDGE = K.defer_edge      # A/B knob (tgt_amd/knobs.py)
_TRI_RAGGED = K.tri_ragged      # triplet attention skips the padded nodes of every graph (default off)
_EDGE_RAGGED = K.edge_ragged    # the edge row kernels skip the tiles of padded rows (default off; needs _TRI_RAGGED)
_NODE_RAGGED = K.node_ragged    # node attention skips the padded nodes too (default off; needs _TRI_RAGGED)


class Graph(dict):
    """A dict whose keys read and write as attributes (g.h, g.e, g.mask, ...)."""

    def __getattr__(self, name):
        if name in self:
            return self[name]
        raise AttributeError('No such attribute: ' + name)

    __setattr__ = dict.__setitem__

    def __dir__(self):
        return [*super().__dir__(), *self]

    def copy(self):
        return type(self)(self)


class TGT_Encoder(nn.Module):
    """`model_height` TGT layers, each applied `layer_multiplier` times in a row with shared
    weights.  Per-layer keyword handling follows reference encoder.py:52-78: `IndivConfig`
    lists give one value per layer, `drop_path` ramps linearly with depth, and the last layer
    drops its node (edge) half when the model is not node (edge) ended."""

    class IndivConfig(list):
        pass

    def __init__(self, model_height=4, layer_multiplier=1, node_ended=True,
                 edge_ended=True, egt_simple=False, **layer_configs):
        super().__init__()
        if not (node_ended or edge_ended):
            raise AssertionError('At least one of node_ended and edge_ended must be True')
        vars(self).update(model_height=model_height, layer_multiplier=layer_multiplier,
                          node_ended=node_ended, edge_ended=edge_ended, egt_simple=egt_simple,
                          layer_configs=layer_configs, **layer_configs)
        self.TGT_layers = nn.ModuleList(TGT_Layer(**self.get_layer_kwargs(i)) for i in range(model_height))

    def _value_for_layer(self, key, value, depth):
        if isinstance(value, self.IndivConfig):
            return value[depth]
        if key == 'drop_path':                       # 0 at the first layer ... `value` at the last
            return value * depth / (self.model_height - 1)
        return value

    def get_layer_kwargs(self, i):
        kwargs = {k: self._value_for_layer(k, v, i) for k, v in self.layer_configs.items()}
        last = i == self.model_height - 1
        kwargs.update(node_update=self.node_ended or not last,
                      edge_update=not self.egt_simple and (self.edge_ended or not last))
        return kwargs

    def apply_layer(self, layer_idx, graph, defer_edge=False):
        for _ in range(self.layer_multiplier):
            graph = self.TGT_layers[layer_idx](graph, defer_edge=defer_edge)
        return graph

    def _edge_ragged_ok(self):
        """may the edge row kernels leave the padded rows out?  Only when no layer lets a padded row reach a real one: a triplet
        module must take the node counts (the attention family: every key of a padded node is masked; TriangularUpdate: every
        operand of a pair with a padded node is gated to an exact zero).  The aggregate family's
        gated outward direction is unmasked (quirk Q2), so its padded rows DO reach real outputs: such a model computes everything."""
        return self._padding_is_unread('edge_ragged', 'TGT_EDGE_RAGGED has no effect on this model: a triplet module that does not take '
                                       'node counts (the aggregate family) reads padded rows; every edge row is computed')

    def _padding_is_unread(self, key, notice):
        """does every triplet module take the node counts?  (one predicate for every switch that changes padded rows of the edge
        stream; `notice` is said once, under `key`, when it does not hold)"""
        ok = all(getattr(layer.tria, 'takes_node_counts', False) for layer in self.TGT_layers if hasattr(layer, 'tria'))
        if not ok:
            ops._slow_path_notice(key, notice)
        return ok

    def _counts_bound_rows(self):
        """does some triplet module need counts that bound the rows of the mask as well as its columns?"""
        return any(getattr(layer.tria, 'node_counts_bound_rows', False) for layer in self.TGT_layers if hasattr(layer, 'tria'))

    def _node_ragged_ok(self):
        """may node attention leave the padded nodes out?  Its H_hat is then zero at padded pairs instead of a finite value, which
        is the edge stream's padded rows: the gate of _edge_ragged_ok, for the same reason (an aggregate-family model reads them)."""
        return self._padding_is_unread('node_ragged', 'TGT_NODE_RAGGED has no effect on this model: a triplet module that does not take '
                                       'node counts (the aggregate family) reads padded rows; node attention computes every node')

    def forward(self, inputs):
        graph = Graph(inputs)
        # ragged batches: the per-graph node counts the triplet attention kernels skip behind, once per forward from the mask
        # (one launch, nothing read on the host); a caller that knows num_nodes may put its own int32 `node_counts` in the inputs
        own_counts = _TRI_RAGGED and graph.get('node_counts') is None and graph.mask.is_cuda
        # ... which node attention honours too under TGT_NODE_RAGGED; its count must bound the ROWS of the mask as well as the columns
        # (tgt_mask_node_counts guarantees the column half only): the larger of the counts of the mask and of its transpose -- two
        # small launches more, still nothing on the host.  The triplet modules get the same, larger, count: always safe.
        node_ragged = bool(_NODE_RAGGED and _TRI_RAGGED and graph.mask.is_cuda and self._node_ragged_ok())
        if own_counts:
            mask3 = ops.as_mask3(graph.mask, graph.e.shape[0], graph.e.shape[1])
            graph['node_counts'] = ops.mask_node_counts(mask3)
            # (a triplet module whose operands are gated by the mask of their own pair -- TriangularUpdate -- needs the row half too)
            if node_ragged or self._counts_bound_rows():
                graph['node_counts'] = torch.maximum(graph['node_counts'], ops.mask_node_counts(mask3.transpose(1, 2).contiguous()))
        if node_ragged and graph.get('node_counts') is not None:
            graph['node_ragged'] = True
        # ... and the live tile list the persistent edge row kernels walk (TGT_EDGE_RAGGED): one more launch per forward, carried
        # by an ops context around the layer loop; the padded rows of the edge stream are then zeros in whole dead tiles
        live = None
        if _EDGE_RAGGED and _TRI_RAGGED and graph.get('node_counts') is not None and graph.e.is_cuda and self._edge_ragged_ok():
            live = ops.edge_live_tiles(graph['node_counts'], graph.e.shape[1])
        with ops.edge_live(live):
            for idx in range(self.model_height):
                # between layers the closing edge residual travels un-added (layers.PendingResidual)
                graph = self.apply_layer(idx, graph, defer_edge=_DEFER_EDGE)
            if isinstance(graph.e, PendingResidual):
                graph.e = graph.e.materialize()
        side = graph.pop('node_side', None)
        if side is not None:
            side.join(graph.h)
        if own_counts:
            graph.pop('node_counts', None)
        graph.pop('node_ragged', None)
        return graph
