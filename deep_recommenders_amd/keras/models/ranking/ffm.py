"""FFM (Juan et al., RecSys 2016, "Field-aware Factorization Machines for CTR Prediction").  The reference's README lists FFM among its
ranking models and ships no code for it; the model here follows the paper and is built like afm.py: one EmbeddingSlab for the tables and
the linear term, and the field-aware interaction as one fused kernel each way (csrc/ffm.hip).  A feature holds one latent k-vector per
field, so its table row is F * k wide; for single-valued fields the interaction is computed straight from the table rows
(dr_ffm_gather_fwd) and the gathered rows are never written."""
import math
from typing import Dict

import torch
from torch import nn

from deep_recommenders_amd import feature_column as fc
from deep_recommenders_amd import layers as L
from deep_recommenders_amd import losses
from deep_recommenders_amd import ops


class FieldAwareInteraction(nn.Module):
    """FieldAwareInteraction()(rows) -> [B]

    rows [B, F, F, k] or [B, F, F * k]: rows[b, i, j] is the factor of example b's feature of field i towards field j.  Output
    sum_{j < i} <rows[b, i, j], rows[b, j, i]>.  The diagonal blocks rows[b, i, i] take no part: they are never read and their gradient
    is exactly 0.  No [B, F, F, k] product is built."""

    def __init__(self, **kwargs):
        super().__init__()
        self._kwargs = kwargs

    def call(self, rows, **kwargs):
        rows = torch.as_tensor(rows, dtype=torch.float32)
        if rows.dim() not in (3, 4):
            raise ValueError("`rows` dim should be 3 or 4. Got `rows` dim = {}".format(rows.dim()))
        F = int(rows.shape[1])
        if rows.dim() == 4:
            if rows.shape[2] != F:
                raise ValueError("`rows` should be [B, F, F, k]. Got `rows` shape = {}".format(tuple(rows.shape)))
            k = int(rows.shape[3])
        else:
            if F == 0 or rows.shape[2] % F != 0 or rows.shape[2] == 0:
                raise ValueError("`rows` should be [B, F, F * k]. Got `rows` shape = {}".format(tuple(rows.shape)))
            k = int(rows.shape[2]) // F
        ops.ffm_row_width(F, k)                                # the kernel's domain, checked before anything moves to the device
        return L.ffm_interaction(rows.cuda(), F, k)

    forward = call

    def get_config(self):
        return dict(self._kwargs)


class FFM(nn.Module):
    """FFM(indicator_columns, embedding_columns).call(inputs) -> prob = sigmoid(linear(indicator) + sum_{j < i} <v_{i -> j}, v_{j -> i}>).

    Each embedding column's `dimension` is the latent size k (all equal).  The fields are numbered in the order of `embedding_columns`
    (= `model.slab.keys`), never in the order of `inputs`: block j of a row means "towards field j".  One EmbeddingSlab holds the rows,
    F * k wide (truncated normal with sigma = 1 / sqrt(k) unless the column brings its own initializer, which then sees the [n, F * k]
    rows), the linear term and the output bias.  Multi-valued fields are mean-pooled by the slab and the pooled row is the field's row; a
    missing id is a row of zeros.  `model.slab.sparse_lr = lr` applies fused SGD to the looked-up rows on both paths."""

    ROW_LIMIT = 256                                            # the slab's widest row

    def __init__(self, indicator_columns, embedding_columns, device="cuda", **kwargs):
        super().__init__()
        if indicator_columns is None or len(indicator_columns) == 0:
            raise ValueError("FFM needs the indicator columns of its linear term")
        F = len(embedding_columns)
        if F < 2:
            raise ValueError("FFM pairs fields: at least 2 embedding columns are required, got {}".format(F))
        dims = sorted({int(c.dimension) for c in embedding_columns})
        if len(dims) != 1:
            raise ValueError("FFM needs one latent size k for all fields: all dimensions must be equal, got {}".format(dims))
        k = dims[0]
        if k % 4 != 0:
            raise ValueError("FFM's latent size k (the columns' dimension) must be a multiple of 4, got {}".format(k))
        if F * k > self.ROW_LIMIT:
            raise ValueError("FFM keeps one k-vector per field in every row: F * k = {} * {} = {} exceeds the slab's limit of {} floats "
                             "per row".format(F, k, F * k, self.ROW_LIMIT))
        self._indicator_columns = indicator_columns
        self._embedding_columns = embedding_columns
        self._kwargs = kwargs
        self.F, self.k = F, k
        std = 1.0 / math.sqrt(k)
        wide = [fc.embedding_column(c.categorical_column, F * k, combiner=c.combiner,
                                    initializer=c.initializer if c.initializer is not None else (lambda rows: L.truncated_normal_(rows, std)),
                                    trainable=c.trainable) for c in embedding_columns]
        self.slab = L.EmbeddingSlab(wide, indicator_columns, device=device)
        self.interaction = FieldAwareInteraction()

    def _terms(self, inputs: Dict[str, object]):
        """(first_order [B], inter [B])"""
        for key in self.slab.keys:
            if key not in inputs:
                raise ValueError("FFM needs every field in `inputs`: {!r} is missing".format(key))
        F, k, slab = self.F, self.k, self.slab
        ids, col_start, row_base = slab.transform(inputs, slab.keys)
        if col_start is None:                                  # every field single-valued: straight from the table
            inter, first = L.ffm_gather(slab.table, slab.lin_w, slab.lin_bias, ids, row_base, F, k, slab.sparse_lr)
            return first, inter
        concat, first, _ = slab(inputs, slab.keys, second_order=False)        # [B, F * F * k]: the pooled rows, field-major
        return first, self.interaction(concat.view(-1, F, F * k))             # read in place

    def logits(self, inputs):
        first, inter = self._terms(inputs)
        return first + inter

    def call(self, inputs, **kwargs):
        return losses.sigmoid(self.logits(inputs))

    forward = call

    def predict(self, inputs):
        with torch.no_grad():
            return self.call(inputs).cpu().numpy()

    def get_config(self):
        config = {"num_fields": self.F, "latent_dim": self.k}
        return {**self._kwargs, **config}
