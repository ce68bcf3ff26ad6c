"""BERT (Devlin et al., "BERT: Pre-training of Deep Bidirectional Transformers for Language Understanding", NAACL 2019): the
encoder, its embedding block and the pre-training heads (masked LM + next-sentence prediction).  The reference's README lists the
model; its tree has no code for it, so the surface follows the paper and its public TensorFlow release: post-norm blocks,
LayerNorm epsilon 1e-12 inside the root, exact (erf) GELU, truncated-normal(0.02) weights, zero biases, the MLM decoder tied to
the token table, pooled_output = tanh(Dense(first token)).

Kernels: dr_bert_embed_* (gather of three tables + LayerNorm + dropout in one pass, and its backward), dr_attn_* with the additive
padding mask, dr_add_layernorm_*, the GEMM path (layers.mlp, GELU as its activation code 4: dr_gelu_*), layers.dropout,
dr_softmax_ce_ids + dr_colsum_add inside layers.vocab_cross_entropy, dr_mlm_mask for the dynamic masking, dr_rows_gather /
dr_rows_scatter_add around the masked positions.

Not provided: bf16 / mixed precision, the tanh-approximate GELU, WordPiece tokenisation, checkpoint import."""
import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd import losses, ops
from deep_recommenders_amd.keras.models.nlp.multi_head_attention import _Seeded, _check_rate

LAYER_NORM_EPS = 1e-12
DENOM_EPS = 1e-5          # BERT's masked-LM normaliser: sum(loss * w) / (sum(w) + 1e-5)


def _ids(x):
    ids = torch.as_tensor(x)
    ids = ids if ids.is_cuda else ids.cuda()
    return ids.to(torch.int64).contiguous()


def _add_grad(p, g):
    """p.grad += g (dr_axpy), or p.grad = g where there is none yet"""
    if p.grad is None:
        p.grad = g
    else:
        ops.axpy(1.0, g.contiguous(), p.grad)


def _row_pieces(rows, D):
    """dr_rows_gather / dr_rows_scatter_add take rows of at most 256 floats: a [N, D] matrix is addressed as [N k, D / k] with the
    smallest k that fits, row r being the pieces r k .. r k + k - 1.  Returns (piece numbers, k)."""
    k = next(k for k in range(1, D // 4 + 1) if D % k == 0 and D // k <= 256 and (D // k) % 4 == 0)
    if k == 1:
        return rows, 1
    return (rows[:, None] * k + torch.arange(k, dtype=torch.int64, device=rows.device)[None, :]).reshape(-1), k


def _gather_rows(rows, mat):
    """mat[rows] for a contiguous fp32 [N, D] matrix, D % 4 == 0 (dr_rows_gather)"""
    N, D = mat.shape
    pieces, k = _row_pieces(rows, D)
    out, _ = ops.rows_gather(pieces, mat.view(N * k, D // k))
    return out.view(rows.numel(), D)


def _scatter_rows_add(rows, grads, mat):
    """mat[rows] += grads (dr_rows_scatter_add)"""
    N, D = mat.shape
    pieces, k = _row_pieces(rows, D)
    ops.rows_scatter_add(pieces, grads.contiguous().view(rows.numel() * k, D // k), None, 1.0, mat.view(N * k, D // k), None)


def _weight(shape, std, device):
    return nn.Parameter(L.truncated_normal_(torch.empty(shape, dtype=torch.float32, device=device), std))


def _zeros(n, device):
    return nn.Parameter(torch.zeros(n, dtype=torch.float32, device=device))


def _ones(n, device):
    return nn.Parameter(torch.ones(n, dtype=torch.float32, device=device))


class BertEmbedding(_Seeded):
    """dropout(LayerNorm(word_embeddings[ids] + position_embeddings[l] + token_type_embeddings[segment])) as ONE kernel.  call()
    returns a VALUE (no autograd edge to the tables); backward(d_out) adds the gradients of the latest call into the .grad of the
    three tables, gamma and beta -- explicit forward and backward, as NFM's slab."""

    def __init__(self, vocab_size, hidden_size, max_position=512, type_vocab_size=2, dropout_rate=0.1, initializer_range=0.02,
                 device="cuda", **kwargs):
        super().__init__()
        self._dropout_rate = _check_rate(dropout_rate)
        self._init_seed(kwargs)
        self.word_embeddings = _weight((vocab_size, hidden_size), initializer_range, device)
        self.position_embeddings = _weight((max_position, hidden_size), initializer_range, device)
        self.token_type_embeddings = _weight((type_vocab_size, hidden_size), initializer_range, device)
        self.gamma = _ones(hidden_size, device)
        self.beta = _zeros(hidden_size, device)
        self._saved = None

    def call(self, input_ids, segment_ids=None, training=False, **kwargs):
        ids = _ids(input_ids)
        seg = torch.zeros_like(ids) if segment_ids is None else _ids(segment_ids)
        rate = self._dropout_rate if training else 0.0
        seed = self._next_seed()
        out, stats = ops.bert_embed_fwd(ids, seg, self.word_embeddings.data, self.position_embeddings.data,
                                        self.token_type_embeddings.data, self.gamma.data, self.beta.data, LAYER_NORM_EPS, rate, seed)
        self._saved = (ids, seg, stats, rate, seed)
        return out

    forward = call

    def backward(self, d_out):
        """adds the gradients that d_out [B, L, D] (the gradient of the latest call's output) sends to the five parameters into
        their .grad; every sum has a fixed order"""
        if self._saved is None:
            raise RuntimeError("BertEmbedding.backward needs a call() first")
        ids, seg, stats, rate, seed = self._saved
        d_tok = torch.zeros_like(self.word_embeddings.data)
        _, d_gamma, d_beta, d_pos, d_seg = ops.bert_embed_bwd(ids, seg, self.word_embeddings.data, self.position_embeddings.data,
                                                              self.token_type_embeddings.data, self.gamma.data, stats, d_out, d_tok,
                                                              rate, seed)
        d_pos_full = torch.zeros_like(self.position_embeddings.data)
        d_pos_full[:d_pos.shape[0]].copy_(d_pos)
        for p, g in ((self.word_embeddings, d_tok), (self.position_embeddings, d_pos_full), (self.token_type_embeddings, d_seg),
                     (self.gamma, d_gamma), (self.beta, d_beta)):
            if p.requires_grad:
                _add_grad(p, g)


class BertLayer(_Seeded):
    """One encoder block: self-attention over a single [D, 3 D] QKV projection (the heads and q / k / v are column blocks of its
    output, read in place through their row pitch), output projection, dropout, Add & Norm; Dense(F) -> GELU -> Dense(D), dropout,
    Add & Norm.  A call draws three seeds: attention probabilities, the two hidden dropouts."""

    def __init__(self, hidden_size, num_heads, intermediate_size, hidden_dropout=0.1, attention_dropout=0.1, initializer_range=0.02,
                 device="cuda", **kwargs):
        super().__init__()
        if hidden_size % num_heads != 0:
            raise ValueError("hidden_size {} is not a multiple of num_heads {}".format(hidden_size, num_heads))
        D, F, s = hidden_size, intermediate_size, initializer_range
        self._num_heads = num_heads
        self._hidden_dropout = _check_rate(hidden_dropout)
        self._attention_dropout = _check_rate(attention_dropout)
        self._init_seed(kwargs)
        self.last_seeds = None          # (attention, dropout, dropout) seeds of the latest call
        self.qkv_kernel, self.qkv_bias = _weight((D, 3 * D), s, device), _zeros(3 * D, device)
        self.attention_output_kernel, self.attention_output_bias = _weight((D, D), s, device), _zeros(D, device)
        self.attention_norm_gamma, self.attention_norm_beta = _ones(D, device), _zeros(D, device)
        self.intermediate_kernel, self.intermediate_bias = _weight((D, F), s, device), _zeros(F, device)
        self.output_kernel, self.output_bias = _weight((F, D), s, device), _zeros(D, device)
        self.output_norm_gamma, self.output_norm_beta = _ones(D, device), _zeros(D, device)

    def call(self, x, key_mask=None, training=False, **kwargs):
        """x [B, L, D]; key_mask [B, L] bool, True at padded keys (dr_attn_*'s additive mask)"""
        B, Ln, D = x.shape
        x2 = x.reshape(B * Ln, D)
        hidden = self._hidden_dropout if training else 0.0
        seeds = [self._next_seed() for _ in range(3)]
        self.last_seeds = tuple(seeds)
        qkv = L.mlp(x2, [self.qkv_kernel], [self.qkv_bias], [0]).reshape(B, Ln, 3 * D)
        q, k, v = qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:]
        context = L.attention(q, k, v, self._num_heads, key_mask, False, self._attention_dropout if training else 0.0, seeds[0])
        a = L.mlp(context.reshape(B * Ln, D), [self.attention_output_kernel], [self.attention_output_bias], [0])
        if hidden > 0.0:
            a = L.dropout(a, hidden, seeds[1])
        h = L.add_layer_norm(a, x2, self.attention_norm_gamma, self.attention_norm_beta, LAYER_NORM_EPS)
        f = L.mlp(h, [self.intermediate_kernel, self.output_kernel], [self.intermediate_bias, self.output_bias], [4, 0])
        if hidden > 0.0:
            f = L.dropout(f, hidden, seeds[2])
        return L.add_layer_norm(f, h, self.output_norm_gamma, self.output_norm_beta, LAYER_NORM_EPS).reshape(B, Ln, D)

    forward = call


class BERT(_Seeded):
    def __init__(self, vocab_size, hidden_size=768, num_layers=12, num_heads=12, intermediate_size=3072, max_position=512,
                 type_vocab_size=2, hidden_dropout=0.1, attention_dropout=0.1, initializer_range=0.02, device="cuda", **kwargs):
        super().__init__()
        self._config = dict(vocab_size=vocab_size, hidden_size=hidden_size, num_layers=num_layers, num_heads=num_heads,
                            intermediate_size=intermediate_size, max_position=max_position, type_vocab_size=type_vocab_size,
                            hidden_dropout=_check_rate(hidden_dropout), attention_dropout=_check_rate(attention_dropout),
                            initializer_range=initializer_range)
        self._init_seed(kwargs)
        self._kwargs = kwargs
        self.embeddings = BertEmbedding(vocab_size, hidden_size, max_position, type_vocab_size, hidden_dropout, initializer_range, device,
                                        seed=self.seed * 131)
        self.layers = nn.ModuleList([BertLayer(hidden_size, num_heads, intermediate_size, hidden_dropout, attention_dropout,
                                               initializer_range, device, seed=self.seed * 131 + 1 + i) for i in range(num_layers)])
        self.pooler_kernel, self.pooler_bias = _weight((hidden_size, hidden_size), initializer_range, device), _zeros(hidden_size, device)
        self.last_seeds = None          # (embedding, [per layer: attention, dropout, dropout]) seeds of the latest call
        self._x0 = None

    def encode(self, input_ids, segment_ids=None, input_mask=None, training=False):
        """sequence_output [B, L, D] alone (no pooler): what call() and BertPretraining build on"""
        ids = _ids(input_ids)
        mask = (ids != 0) if input_mask is None else torch.as_tensor(input_mask).to(device=ids.device, dtype=torch.bool)
        key_mask = ~mask                                        # True = padded, the kernels' convention
        x0 = self.embeddings.call(ids, segment_ids, training)
        x0.requires_grad_(torch.is_grad_enabled())              # a leaf: the tape starts here, embeddings_backward continues below it
        self._x0 = x0
        x = x0
        for layer in self.layers:
            x = layer.call(x, key_mask, training)
        self.last_seeds = (self.embeddings.last_seed, [layer.last_seeds for layer in self.layers])
        return x

    def pool(self, first_token):
        """tanh(Dense(first_token [B, D]))"""
        return L.mlp(first_token, [self.pooler_kernel], [self.pooler_bias], [3])

    def call(self, input_ids, segment_ids=None, input_mask=None, training=False, **kwargs):
        """(sequence_output [B, L, D], pooled_output [B, D]).  input_mask [B, L] is True / 1 at real tokens and defaults to
        ids != 0; dropout rates are 0 unless training.  Gradients from the two outputs reach every encoder and pooler parameter
        through autograd.  They do NOT reach the embedding tables and the embedding LayerNorm (the embedding block is an explicit
        kernel pair, as NFM's slab): after outputs.backward(...), embeddings_backward(x0.grad) -- with no argument it takes the
        gradient autograd left on the encoder's input -- delivers them into the .grad of those five parameters."""
        sequence_output = self.encode(input_ids, segment_ids, input_mask, training)
        return sequence_output, self.pool(sequence_output[:, 0, :])

    forward = call

    def embeddings_backward(self, d_x0=None):
        """adds the embedding block's parameter gradients for the latest call: d_x0 [B, L, D], default the .grad of the encoder input"""
        if d_x0 is None:
            d_x0 = self._x0.grad if self._x0 is not None else None
        if d_x0 is None:
            raise RuntimeError("embeddings_backward: no gradient has reached the encoder input of the latest call")
        self.embeddings.backward(d_x0)

    @property
    def x0(self):
        """the encoder input of the latest call (the embedding block's output, a leaf of the tape)"""
        return self._x0

    def reset_calls(self):
        """rewinds the dropout streams of the model, its embedding block and every layer"""
        for m in self.modules():
            if isinstance(m, _Seeded):
                m._calls = 0

    def get_config(self):
        return {**self._kwargs, **self._config}


class BertPretraining(nn.Module):
    """The pre-training heads over a BERT: masked LM (Dense(D) -> GELU -> LayerNorm, decoder tied to the token table + an output bias
    [V]) and next-sentence prediction (Dense(2) over pooled_output).  Ids below num_special are never masked ([PAD], [UNK], [CLS],
    [SEP], [MASK] = 0 .. 4 by default) and mask_id replaces 80 % of the chosen positions."""

    def __init__(self, bert, num_special=5, mask_id=4, device=None, **kwargs):
        super().__init__()
        self.bert = bert
        cfg = bert.get_config()
        D, V, s = cfg["hidden_size"], cfg["vocab_size"], cfg["initializer_range"]
        device = bert.pooler_kernel.device if device is None else device
        self._vocab_size, self._num_special, self._mask_id = V, int(num_special), int(mask_id)
        self.transform_kernel, self.transform_bias = _weight((D, D), s, device), _zeros(D, device)
        self.transform_norm_gamma, self.transform_norm_beta = _ones(D, device), _zeros(D, device)
        self.output_bias = _zeros(V, device)
        self.nsp_kernel, self.nsp_bias = _weight((D, 2), s, device), _zeros(2, device)
        self._mask_calls = 0

    def mask(self, input_ids, prob=0.15, max_predictions=20, seed=None):
        """(masked ids [B, L], positions int32 [B, P], labels int64 [B, P]) of dr_mlm_mask on the device; seed None draws the next one
        of this head's own counter stream"""
        if seed is None:
            self._mask_calls += 1
            seed = (self.bert.seed * 1000003 + 7919 * self._mask_calls) & 0xFFFFFFFFFFFFFFFF
        return ops.mlm_mask(_ids(input_ids), self._vocab_size, self._num_special, self._mask_id, prob, max_predictions, seed)

    def _transform(self, rows):
        t = L.mlp(rows, [self.transform_kernel], [self.transform_bias], [4])
        return L.add_layer_norm(t, None, self.transform_norm_gamma, self.transform_norm_beta, LAYER_NORM_EPS)

    def nsp_logits(self, first_rows):
        return L.mlp(self.bert.pool(first_rows), [self.nsp_kernel], [self.nsp_bias], [0])

    @staticmethod
    def _rows_of(positions, Ln):
        """flat row numbers b * L + position of the [B, P] positions (a padding slot, -1, names the row's first token: its label is
        negative, so it gets no loss and a zero gradient), and of the first tokens"""
        B = positions.shape[0]
        base = torch.arange(B, dtype=torch.int64, device=positions.device) * Ln
        return (base[:, None] + positions.to(torch.int64).clamp(min=0)).reshape(-1), base

    @staticmethod
    def _nsp_loss(logits, nsp_labels):
        y = _ids(nsp_labels).reshape(-1)
        onehot = torch.stack([(y == 0), (y == 1)], dim=1).to(torch.float32)
        w = torch.full((y.shape[0],), 1.0 / y.shape[0], dtype=torch.float32, device=logits.device)
        return losses._SoftmaxCEFn.apply(logits.contiguous(), onehot, w).reshape(())

    def losses(self, input_ids, segment_ids, positions, labels, nsp_labels, input_mask=None, training=False):
        """(mlm_loss, nsp_loss) as device scalars (values, no tape): mlm_loss = sum_r w_r CE_r / (sum_r w_r + 1e-5) over the slots
        with labels >= 0, nsp_loss the mean cross-entropy of the two-way head.  input_ids are the MASKED ids."""
        with torch.no_grad():
            seq = self.bert.encode(input_ids, segment_ids, input_mask, training)
            B, Ln, D = seq.shape
            rows, first = self._rows_of(positions, Ln)
            seq2 = seq.reshape(B * Ln, D).contiguous()
            masked_rows = _gather_rows(rows, seq2)
            first_rows = _gather_rows(first, seq2)
            y = labels.reshape(-1).contiguous()
            w = (y >= 0).to(torch.float32)
            denom = ops.reduce_sum(w)
            loss_rows, _ = L.vocab_cross_entropy(self._transform(masked_rows), self.bert.embeddings.word_embeddings, self.output_bias, y,
                                                 weight=w, denom=denom, denom_eps=DENOM_EPS)
            mlm = ops.reduce_sum(loss_rows) / (denom + DENOM_EPS)
            return mlm.reshape(()), self._nsp_loss(self.nsp_logits(first_rows), nsp_labels)

    def pretrain_step(self, input_ids, segment_ids, nsp_labels, optimizer, masked=None, input_mask=None, prob=0.15, max_predictions=20):
        """One pre-training step; returns (mlm_loss, nsp_loss) as device scalars.  In order: dynamic masking on the device (unless
        masked = (ids, positions, labels) is given); the encoder forward with dropout; a cut at sequence_output -- the rows at the
        masked positions and the first-token rows are gathered (dr_rows_gather) and become leaves; the heads under autograd;
        layers.vocab_cross_entropy with denom = sum(weights) on the device and denom_eps = 1e-5; the NSP loss; one
        torch.autograd.backward through the heads; dr_rows_scatter_add of both leaf gradients into a zeroed d_seq;
        sequence_output.backward(d_seq); embeddings_backward(x0.grad), the tied token table receiving the decoder's and the
        embedding's contribution; optimizer.step().  Works with optim.Adam and with torch optimizers."""
        optimizer.zero_grad(set_to_none=True)
        ids_m, positions, labels = self.mask(input_ids, prob, max_predictions) if masked is None else masked
        seq = self.bert.encode(ids_m, segment_ids, input_mask, training=True)
        B, Ln, D = seq.shape
        rows, first = self._rows_of(positions, Ln)
        seq2 = seq.reshape(B * Ln, D)
        seq_val = seq2.detach().contiguous()
        masked_rows = _gather_rows(rows, seq_val)
        first_rows = _gather_rows(first, seq_val)
        masked_rows.requires_grad_(True)
        first_rows.requires_grad_(True)
        t = self._transform(masked_rows)
        nsp_loss = self._nsp_loss(self.nsp_logits(first_rows), nsp_labels)
        y = labels.reshape(-1).contiguous()
        w = (y >= 0).to(torch.float32)
        denom = ops.reduce_sum(w)
        table = self.bert.embeddings.word_embeddings
        d_table, d_bias = torch.zeros_like(table.data), torch.zeros_like(self.output_bias.data)
        loss_rows, d_t = L.vocab_cross_entropy(t, table, self.output_bias, y, weight=w, denom=denom, denom_eps=DENOM_EPS, d_table=d_table,
                                               d_bias=d_bias)
        mlm_loss = (ops.reduce_sum(loss_rows) / (denom + DENOM_EPS)).reshape(())
        torch.autograd.backward([t, nsp_loss], [d_t, torch.ones_like(nsp_loss)])
        d_seq = torch.zeros((B * Ln, D), dtype=torch.float32, device=seq.device)
        _scatter_rows_add(rows, masked_rows.grad, d_seq)
        _scatter_rows_add(first, first_rows.grad, d_seq)
        seq2.backward(d_seq)
        self.bert.embeddings_backward()
        if table.requires_grad:
            _add_grad(table, d_table)
        if self.output_bias.requires_grad:
            _add_grad(self.output_bias, d_bias)
        optimizer.step()
        return mlm_loss, nsp_loss.detach()
