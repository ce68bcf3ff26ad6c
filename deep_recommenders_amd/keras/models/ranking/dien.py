"""DIEN -- Deep Interest Evolution Network (Zhou et al., AAAI 2019).  The reference's README lists it after DIN and ships no code for
it; the classes follow the DIN file's conventions (built on the first call, get_config returns the constructor arguments).

  * GRU: xp = seq W + b over all B * T rows through the MFMA GEMM path (deep_recommenders_amd.layers.mlp, whose backward yields dW, db
    and d_seq), then the whole recurrence in one kernel (layers.gru_sequence, csrc/dien.hip).  The paper's form
    h_t = (1 - u) h_{t-1} + u c, c = tanh(x W_c + r * (h_{t-1} U_c)): Keras's and PyTorch's update gate is z = 1 - u.
  * AUGRU: the same layer with the update gate scaled by an attention weight per step, u' = a_t u (the paper's eq. 15-16).
  * InterestExtractor: a GRU plus the auxiliary loss that ties h_t to the next behaviour e_{t+1} against a sampled negative.
  * InterestEvolution: a_t = softmax over the valid steps of <h_t, e_target W_a^T> (layers.sequence_attention), then an AUGRU; returns
    the final state h'(len).
  * DIEN: item table -> extractor -> evolution -> concat [h', e_target, profile] -> Dense tower (Dice) -> Dense(1) -> sigmoid.

Steps t >= lengths[b] are skipped, not multiplied by zero: whatever the sequence holds there reaches no output and no gradient."""
import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import losses
from deep_recommenders_amd import ops
from deep_recommenders_amd.keras.models.ranking.dcn import _init
from deep_recommenders_amd.keras.models.ranking.din import _ACT_CODES, Dice


def _dev(x, dtype=torch.float32):
    """a tensor of `dtype`, in HBM when there is a device (without one the kernels' wrappers raise: there is no fallback)"""
    x = torch.as_tensor(x)
    if dtype is not None and x.dtype != dtype:
        x = x.to(dtype)
    return x.cuda() if torch.cuda.is_available() and not x.is_cuda else x


def _lengths(lengths, mask, B, T, device):
    """int32 [B] on `device` from lengths or from a prefix mask [B, T] (nonzero / True at the valid steps), or None"""
    if lengths is not None and mask is not None:
        raise ValueError("give mask or lengths, not both")
    if mask is not None:
        mask = torch.as_tensor(mask).to(device)
        if tuple(mask.shape) != (B, T):
            raise ValueError("mask must be [B, T] = %s, got %s" % ((B, T), tuple(mask.shape)))
        lengths = (mask != 0).sum(dim=1)
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths).to(device).reshape(-1)
    if lengths.shape[0] != B:
        raise ValueError("lengths must be [B] = [%d], got %s" % (B, tuple(lengths.shape)))
    return lengths.to(torch.int32)


class _RowDotFn(torch.autograd.Function):
    """out[m] = <a[m], b[m]> (dr_rowdot); the gradients are row scalings (dr_rows_scale)"""

    @staticmethod
    def forward(ctx, a, b):
        a, b = L._rows(a, dense=True), L._rows(b, dense=True)
        ctx.save_for_backward(a, b)
        return ops.rowdot(a, b)

    @staticmethod
    @L._needed_only
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = L._rows(g, dense=True)
        return (ops.rows_scale(b, g) if ctx.needs_input_grad[0] else None, ops.rows_scale(a, g) if ctx.needs_input_grad[1] else None)


class _ItemRowsFn(torch.autograd.Function):
    """rows of the item table (dr_rows_gather); the table's gradient is a scatter-add into zeros (dr_rows_scatter_add)"""

    @staticmethod
    def forward(ctx, table, ids):
        ctx.save_for_backward(ids, table)
        return ops.rows_gather(ids, L._rows(table, dense=True))[0]

    @staticmethod
    @L._needed_only
    def backward(ctx, g):
        ids, table = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        d_table = L._param_grad(table)
        ops.rows_scatter_add(ids, L._rows(g, dense=True), None, 1.0, d_table, None)
        return d_table, None


class GRU(nn.Module):
    """(seq [B, T, D], lengths=None, mask=None, initial_state=None, return_state=False) -> hs [B, T, units], or (hs, h_last) with
    return_state.  kernel [D, 3 units] and recurrent_kernel [units, 3 units] have the gate columns [u | r | c]; bias [3 units] is the
    input-side bias (there is no recurrent bias).  Domain of the kernel: units % 4 == 0, 4 <= units <= 128 -- a ValueError outside
    it, there is no composed fallback."""

    def __init__(self, units, use_bias=True, kernel_init="glorot_uniform", recurrent_init="glorot_uniform", bias_init="zeros", **kwargs):
        super().__init__()
        if int(units) % 4 != 0 or not 4 <= int(units) <= 128:
            raise ValueError("units must be a multiple of 4 in [4, 128], got %r" % (units,))
        self._units = int(units)
        self._use_bias = use_bias
        self._kernel_init, self._recurrent_init, self._bias_init = kernel_init, recurrent_init, bias_init
        self._kwargs = kwargs
        self.built = False

    def build(self, in_dim, device="cuda"):
        H = self._units
        self.kernel = nn.Parameter(_init(self._kernel_init, (int(in_dim), 3 * H), device))
        self.recurrent_kernel = nn.Parameter(_init(self._recurrent_init, (H, 3 * H), device))
        self.bias = nn.Parameter(_init(self._bias_init, (3 * H,), device)) if self._use_bias else None
        self.built = True

    def _run(self, seq, attention, lengths, mask, initial_state, return_state):
        seq = _dev(seq)
        if seq.dim() != 3:
            raise ValueError("%s is called on seq [B, T, D], got %s" % (type(self).__name__, tuple(seq.shape)))
        B, T, D = seq.shape
        lengths = _lengths(lengths, mask, B, T, seq.device)
        if not self.built:
            self.build(D, seq.device)
        h0 = None if initial_state is None else _dev(initial_state)
        if attention is not None:
            attention = _dev(attention)
            if tuple(attention.shape) != (B, T):
                raise ValueError("attention must be [B, T] = %s, got %s" % ((B, T), tuple(attention.shape)))
        xp = L.mlp(seq.reshape(B * T, D), [self.kernel], [self.bias], [0]).reshape(B, T, 3 * self._units)
        hs, h_last = L.gru_sequence(xp, self.recurrent_kernel, h0, lengths, attention)
        return (hs, h_last) if return_state else hs

    def call(self, seq, lengths=None, mask=None, initial_state=None, return_state=False, **kwargs):
        return self._run(seq, None, lengths, mask, initial_state, return_state)

    forward = call

    def get_config(self):
        config = {
            "units": self._units,
            "use_bias": self._use_bias,
            "kernel_init": self._kernel_init,
            "recurrent_init": self._recurrent_init,
            "bias_init": self._bias_init,
        }
        return {**self._kwargs, **config}


class AUGRU(GRU):
    """GRU with an attentional update gate: (seq [B, T, D], attention [B, T], lengths=None, ...) with u' = attention[b, t] * u.  The
    attention receives a gradient."""

    def call(self, seq, attention, lengths=None, mask=None, initial_state=None, return_state=False, **kwargs):
        if attention is None:
            raise ValueError("AUGRU needs the attention weights [B, T]")
        return self._run(seq, attention, lengths, mask, initial_state, return_state)

    forward = call


class InterestExtractor(nn.Module):
    """The interest-extractor layer: a GRU over the behaviour embeddings, and the auxiliary loss that supervises every state with the
    next behaviour:  -mean over valid (b, t < len - 1) of [log sigmoid <h_t, e_{t+1}> + log(1 - sigmoid <h_t, e'_{t+1}>)], e' the
    sampled negatives.  The inner product needs units == the embedding width."""

    def __init__(self, units, **kwargs):
        super().__init__()
        self._units = int(units)
        self._kwargs = kwargs
        self.gru = GRU(units)

    def call(self, seq, lengths=None, mask=None, initial_state=None, return_state=False, **kwargs):
        return self.gru(seq, lengths=lengths, mask=mask, initial_state=initial_state, return_state=return_state)

    forward = call

    def auxiliary_loss(self, hs, seq, neg_seq, lengths=None):
        hs, seq, neg_seq = _dev(hs), _dev(seq), _dev(neg_seq)
        B, T, H = hs.shape
        if tuple(seq.shape) != (B, T, H) or tuple(neg_seq.shape) != (B, T, H):
            raise ValueError("auxiliary_loss: hs %s, seq %s and neg_seq %s must have one shape (units == the embedding width)"
                             % (tuple(hs.shape), tuple(seq.shape), tuple(neg_seq.shape)))
        if T < 2:
            return hs.sum() * 0.0
        lengths = _lengths(lengths, None, B, T, hs.device)
        n_next = torch.full((B,), T - 1, device=hs.device) if lengths is None else lengths.to(torch.int64).clamp(0, T) - 1
        valid = (torch.arange(T - 1, device=hs.device).unsqueeze(0) < n_next.unsqueeze(1)).reshape(-1)       # plumbing: [B (T - 1)] bool
        h = hs[:, :-1].reshape(B * (T - 1), H)
        pos = _RowDotFn.apply(h, seq[:, 1:].reshape(B * (T - 1), H)).reshape(-1)[valid]
        neg = _RowDotFn.apply(h, neg_seq[:, 1:].reshape(B * (T - 1), H)).reshape(-1)[valid]
        if pos.numel() == 0:
            return hs.sum() * 0.0
        labels = torch.cat([torch.ones_like(pos), torch.zeros_like(neg)])
        return 2.0 * losses.sigmoid_cross_entropy(labels, torch.cat([pos, neg]))       # the mean runs over both terms of a step

    def get_config(self):
        return {**self._kwargs, "units": self._units}


class InterestEvolution(nn.Module):
    """The interest-evolution layer: (hs [B, T, H], target [B, Da], lengths, return_attention=False) -> h'_last [B, units].
    q = target W_a^T with attention_kernel W_a [H, Da]; a = softmax over the valid steps of <hs[b, t], q[b]>; an AUGRU over hs with a."""

    def __init__(self, units, **kwargs):
        super().__init__()
        self._units = int(units)
        self._kwargs = kwargs
        self.augru = AUGRU(units)
        self.built = False

    def build(self, H, Da, device="cuda"):
        self.attention_kernel = nn.Parameter(_init("glorot_uniform", (int(H), int(Da)), device))
        self.built = True

    def call(self, hs, target, lengths=None, return_attention=False, **kwargs):
        hs, target = _dev(hs), _dev(target)
        if hs.dim() != 3 or target.dim() != 2 or target.shape[0] != hs.shape[0]:
            raise ValueError("InterestEvolution is called on hs [B, T, H] and target [B, Da]")
        B, T, H = hs.shape
        lengths = _lengths(lengths, None, B, T, hs.device)
        if not self.built:
            self.build(H, target.shape[1], hs.device)
        q = L.mlp(target, [self.attention_kernel.t().contiguous()], [None], [0])
        a = L.sequence_attention(hs, q, lengths)
        h_last = self.augru(hs, a, lengths=lengths, return_state=True)[1]
        return (h_last, a) if return_attention else h_last

    forward = call

    def get_config(self):
        return {**self._kwargs, "units": self._units}


class DIEN(nn.Module):
    """(behaviors [B, T] int64, lengths [B], target [B] int64, negatives=None [B, T], profile=None [B, P]) -> probability [B, 1].
    One item table [num_items, embedding_dim] serves behaviours, negatives and the target.  With use_auxiliary_loss and negatives
    given the call sets model.auxiliary_loss (else None); add it to the training loss.  The auxiliary loss is an inner product of a
    state and an embedding, so it needs gru_units == embedding_dim."""

    def __init__(self, num_items, embedding_dim, gru_units, dnn_units_size=(200, 80), activation=Dice, use_auxiliary_loss=True,
                 device="cuda", **kwargs):
        super().__init__()
        if int(embedding_dim) % 4 != 0 or not 4 <= int(embedding_dim) <= 256:
            raise ValueError("embedding_dim must be a multiple of 4 in [4, 256], got %r" % (embedding_dim,))
        if use_auxiliary_loss and int(gru_units) != int(embedding_dim):
            raise ValueError("use_auxiliary_loss needs gru_units == embedding_dim, got %r and %r" % (gru_units, embedding_dim))
        is_dice = activation is Dice or isinstance(activation, Dice)
        if not is_dice and (not (activation is None or isinstance(activation, str)) or activation not in _ACT_CODES):
            raise NotImplementedError("activation %r: relu / linear / sigmoid / tanh, or Dice" % (activation,))
        self._num_items, self._embedding_dim, self._gru_units = int(num_items), int(embedding_dim), int(gru_units)
        self._dnn_units_size = tuple(int(u) for u in dnn_units_size)
        self._activation = activation
        self._use_auxiliary_loss = bool(use_auxiliary_loss)
        self._kwargs = kwargs
        self.item_table = nn.Parameter(_init("truncated_normal", (self._num_items, self._embedding_dim), device))
        self.extractor = InterestExtractor(gru_units)
        self.evolution = InterestEvolution(gru_units)
        self.dices = nn.ModuleList([Dice() for _ in self._dnn_units_size]) if is_dice else None
        self.auxiliary_loss = None
        self.built = False

    def build(self, in_dim, device="cuda"):
        dims = (int(in_dim),) + self._dnn_units_size + (1,)
        self.dnn_w = nn.ParameterList([nn.Parameter(_init("glorot_uniform", (dims[i], dims[i + 1]), device)) for i in range(len(dims) - 1)])
        self.dnn_b = nn.ParameterList([nn.Parameter(_init("zeros", (dims[i + 1],), device)) for i in range(len(dims) - 1)])
        self.built = True

    def logits(self, behaviors, lengths, target, negatives=None, profile=None):
        beh = _dev(behaviors, torch.int64)
        tgt = _dev(target, torch.int64).reshape(-1)
        if beh.dim() != 2 or tgt.shape[0] != beh.shape[0]:
            raise ValueError("DIEN is called on behaviors [B, T] and target [B]")
        B, T = beh.shape
        D = self._embedding_dim
        with_aux = self._use_auxiliary_loss and negatives is not None
        ids = [beh.reshape(-1), tgt]
        if with_aux:
            neg = _dev(negatives, torch.int64)
            if tuple(neg.shape) != (B, T):
                raise ValueError("negatives must be [B, T] = %s, got %s" % ((B, T), tuple(neg.shape)))
            ids.append(neg.reshape(-1))
        rows = _ItemRowsFn.apply(self.item_table, torch.cat(ids))                      # one gather for the three uses of the table
        e_beh, e_tgt = rows[:B * T].reshape(B, T, D), rows[B * T:B * T + B]
        lengths = _lengths(lengths, None, B, T, beh.device)
        hs = self.extractor(e_beh, lengths=lengths)
        self.auxiliary_loss = self.extractor.auxiliary_loss(hs, e_beh, rows[B * T + B:].reshape(B, T, D), lengths) if with_aux else None
        parts = [self.evolution(hs, e_tgt, lengths), e_tgt]
        if profile is not None:
            parts.append(_dev(profile))
        x = torch.cat(parts, dim=1)
        if not self.built:
            self.build(x.shape[1], x.device)
        Ws, bs = list(self.dnn_w), list(self.dnn_b)
        if self.dices is None:
            code = _ACT_CODES[self._activation]
            return L.mlp(x, Ws, bs, [code] * (len(Ws) - 1) + [0])
        for i, dice in enumerate(self.dices):
            x = dice(L.mlp(x, [Ws[i]], [bs[i]], [0]))
        return L.mlp(x, [Ws[-1]], [bs[-1]], [0])

    def call(self, behaviors, lengths, target, negatives=None, profile=None, **kwargs):
        return losses.sigmoid(self.logits(behaviors, lengths, target, negatives, profile))

    forward = call

    def get_config(self):
        config = {
            "num_items": self._num_items,
            "embedding_dim": self._embedding_dim,
            "gru_units": self._gru_units,
            "dnn_units_size": self._dnn_units_size,
            "activation": self._activation,
            "use_auxiliary_loss": self._use_auxiliary_loss,
        }
        return {**self._kwargs, **config}
