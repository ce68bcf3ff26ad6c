"""PositionEncoding, Add, PositionWiseFeedForward, LayerNormalization, Transformer, Noam and label_smoothing -- the surface of
the reference's keras/models/nlp/transformer.py.

Transformer(encoder_ids, decoder_ids) -> softmax over the vocabulary, [batch, length, vocab_size].  One `embeddings` matrix serves
the encoder gather, the decoder gather and the pre-softmax projection (its gradient is the sum of the three).  Padding masks are
`ids == 0`; the decoder's cross-attention masks the ENCODER's padded keys.  Post-norm residual blocks; LayerNormalization has
epsilon 1e-8 inside the root.  The Transformer's `dropout_rate` applies to the two embeddings + position sums only: the
MultiHeadAttention layers inside keep their own default 0.1, as in the reference.  Dropout is always on (no training switch).

Kernels: dr_token_embedding_* (gather * sqrt(D) + positions + dropout), dr_attn_* (attention), dr_add_layernorm_* (residual add +
norm in one pass), the GEMM path for the projections and the feed-forward, dr_scores_nt for the tied projection, dr_softmax_rows.
Not provided: the SavedModel round trip (get_config() + state_dict() rebuild a model)."""
import numpy as np
import torch
from torch import nn

from deep_recommenders_amd import layers as L
from deep_recommenders_amd.keras.models.nlp.multi_head_attention import MultiHeadAttention, _Seeded, _check_rate, _f32


def position_encoding_table(seq_length, model_dim):
    """[seq_length, model_dim] fp32: angle pos / 10000^((i - i % 2) / model_dim) in float64, sin on even columns, cos on odd"""
    pos = np.arange(seq_length, dtype=np.float64)[:, None]
    i = np.arange(model_dim)
    angle = pos / np.power(10000, (i - i % 2) / model_dim)[None, :]
    angle[:, 0::2] = np.sin(angle[:, 0::2])
    angle[:, 1::2] = np.cos(angle[:, 1::2])
    return angle.astype(np.float32)


class PositionEncoding(nn.Module):
    """returns the [length, model_dim] table for inputs [batch, length, ...]; the caller adds it"""

    def __init__(self, model_dim, **kwargs):
        super().__init__()
        self._model_dim = model_dim
        self._kwargs = kwargs
        self._cache = {}

    def call(self, inputs, **kwargs):
        seq_length = int(inputs.shape[1])
        device = inputs.device if isinstance(inputs, torch.Tensor) else torch.device("cpu")
        key = (seq_length, str(device))
        if key not in self._cache:
            self._cache[key] = torch.from_numpy(position_encoding_table(seq_length, self._model_dim)).to(device)
        return self._cache[key]

    forward = call

    def get_config(self):
        return {**self._kwargs, "model_dim": self._model_dim}


class Add(nn.Module):
    def __init__(self, **kwargs):
        super().__init__()
        self._kwargs = kwargs

    def call(self, inputs, **kwargs):
        input_a, input_b = inputs
        a, b = _f32(input_a), _f32(input_b)
        if a.shape != b.shape:
            b = b.expand_as(a)
        return L._AddFn.apply(a.reshape(-1), b.reshape(-1)).reshape(a.shape)

    forward = call

    def get_config(self):
        return dict(self._kwargs)


class PositionWiseFeedForward(nn.Module):
    def __init__(self, model_dim, inner_dim, trainable=True, **kwargs):
        super().__init__()
        self._model_dim = model_dim
        self._inner_dim = inner_dim
        self._trainable = trainable
        self._kwargs = kwargs
        self.built = False

    def build(self, in_dim, device="cuda"):
        def weight(shape):
            return nn.Parameter(L.glorot_uniform_(torch.empty(shape, dtype=torch.float32, device=device)), requires_grad=bool(self._trainable))

        def bias(n):                     # Keras' 'uniform' initializer: U(-0.05, 0.05)
            return nn.Parameter(nn.init.uniform_(torch.empty(n, dtype=torch.float32, device=device), -0.05, 0.05),
                                requires_grad=bool(self._trainable))
        self.weights_inner = weight((in_dim, self._inner_dim))
        self.weights_out = weight((self._inner_dim, self._model_dim))
        self.bias_inner = bias(self._inner_dim)
        self.bias_out = bias(self._model_dim)
        self.built = True

    def call(self, inputs, **kwargs):
        x = _f32(inputs)
        if not self.built:
            self.build(x.shape[-1], x.device)
        y = L.mlp(x.reshape(-1, x.shape[-1]), [self.weights_inner, self.weights_out], [self.bias_inner, self.bias_out], [1, 0])
        return y.reshape(*x.shape[:-1], self._model_dim)

    forward = call

    def get_config(self):
        return {**self._kwargs, "model_dim": self._model_dim, "inner_dim": self._inner_dim, "trainable": self._trainable}


class LayerNormalization(nn.Module):
    def __init__(self, epsilon=1e-8, **kwargs):
        super().__init__()
        self._epsilon = epsilon
        self._kwargs = kwargs
        self.built = False

    def build(self, dim, device="cuda"):
        self.beta = nn.Parameter(torch.zeros(dim, dtype=torch.float32, device=device))
        self.gamma = nn.Parameter(torch.ones(dim, dtype=torch.float32, device=device))
        self.built = True

    def call(self, inputs, residual=None, **kwargs):
        """LayerNormalization(inputs [+ residual]); the residual add of the encoder / decoder blocks rides in the same kernel"""
        x = _f32(inputs)
        if not self.built:
            self.build(x.shape[-1], x.device)
        return L.add_layer_norm(x, residual, self.gamma, self.beta, self._epsilon)

    forward = call

    def get_config(self):
        return {**self._kwargs, "epsilon": self._epsilon}


class Transformer(_Seeded):
    def __init__(self, vocab_size, model_dim, n_heads=8, encoder_stack=6, decoder_stack=6, feed_forward_size=2048, dropout_rate=0.1,
                 **kwargs):
        super().__init__()
        self._vocab_size = vocab_size
        self._model_dim = model_dim
        self._n_heads = n_heads
        self._encoder_stack = encoder_stack
        self._decoder_stack = decoder_stack
        self._feed_forward_size = feed_forward_size
        self._dropout_rate = _check_rate(dropout_rate)
        self._init_seed(kwargs)
        self._kwargs = kwargs
        self.last_seeds = None          # (encoder, decoder) embedding-dropout seeds of the latest call
        self.built = False

    def build(self, device="cuda"):
        D, H, F = self._model_dim, self._n_heads, self._feed_forward_size
        self.embeddings = nn.Parameter(L.glorot_uniform_(torch.empty((self._vocab_size, D), dtype=torch.float32, device=device)))
        n = [0]

        def mha(future=False):
            n[0] += 1
            m = MultiHeadAttention(H, D // H, future=future, seed=self.seed * 131 + n[0])
            m.build([(None, None, D)] * 3, device)
            return m

        def norm():
            m = LayerNormalization()
            m.build(D, device)
            return m

        def ff():
            m = PositionWiseFeedForward(D, F)
            m.build(D, device)
            return m

        E, S = self._encoder_stack, self._decoder_stack
        self.EncoderPositionEncoding = PositionEncoding(D)
        self.EncoderMultiHeadAttentions = nn.ModuleList([mha() for _ in range(E)])
        self.EncoderLayerNorms0 = nn.ModuleList([norm() for _ in range(E)])
        self.EncoderPositionWiseFeedForwards = nn.ModuleList([ff() for _ in range(E)])
        self.EncoderLayerNorms1 = nn.ModuleList([norm() for _ in range(E)])
        self.DecoderPositionEncoding = PositionEncoding(D)
        self.DecoderMultiHeadAttentions0 = nn.ModuleList([mha(future=True) for _ in range(S)])
        self.DecoderLayerNorms0 = nn.ModuleList([norm() for _ in range(S)])
        self.DecoderMultiHeadAttentions1 = nn.ModuleList([mha() for _ in range(S)])
        self.DecoderLayerNorms1 = nn.ModuleList([norm() for _ in range(S)])
        self.DecoderPositionWiseFeedForwards = nn.ModuleList([ff() for _ in range(S)])
        self.DecoderLayerNorms2 = nn.ModuleList([norm() for _ in range(S)])
        self.built = True

    @staticmethod
    def _ids(inputs):
        ids = torch.as_tensor(inputs)
        ids = ids if ids.is_cuda else ids.cuda()
        return ids.to(torch.int64)

    def _embed(self, ids, positions, seed):
        return L.token_embedding(self.embeddings, ids, positions(ids), self._dropout_rate, seed)

    def encoder(self, inputs, seed=None):
        ids = self._ids(inputs)
        masks = ids == 0
        encodings = self._embed(ids, self.EncoderPositionEncoding, self._next_seed() if seed is None else seed)
        for i in range(self._encoder_stack):
            attention_out = self.EncoderMultiHeadAttentions[i]([encodings, encodings, encodings, masks])
            attention_out = self.EncoderLayerNorms0[i](attention_out, encodings)                  # Add & Norm
            ff_out = self.EncoderPositionWiseFeedForwards[i](attention_out)
            encodings = self.EncoderLayerNorms1[i](ff_out, attention_out)                          # Add & Norm
        return encodings, masks

    def decoder(self, inputs, seed=None):
        decoder_inputs, encoder_encodings, encoder_masks = inputs
        ids = self._ids(decoder_inputs)
        decoder_masks = ids == 0
        encodings = self._embed(ids, self.DecoderPositionEncoding, self._next_seed() if seed is None else seed)
        for i in range(self._decoder_stack):
            masked_attention_out = self.DecoderMultiHeadAttentions0[i]([encodings, encodings, encodings, decoder_masks])
            masked_attention_out = self.DecoderLayerNorms0[i](masked_attention_out, encodings)
            attention_out = self.DecoderMultiHeadAttentions1[i]([masked_attention_out, encoder_encodings, encoder_encodings,
                                                                 encoder_masks])
            attention_out = self.DecoderLayerNorms1[i](attention_out, masked_attention_out)
            ff_out = self.DecoderPositionWiseFeedForwards[i](attention_out)
            encodings = self.DecoderLayerNorms2[i](ff_out, attention_out)
        B, Ld, D = encodings.shape
        # the pre-softmax projection shares the embedding matrix
        linear_projection = L.tied_projection(encodings.reshape(B * Ld, D), self.embeddings)
        return L.softmax_rows(linear_projection).reshape(B, Ld, self._vocab_size)

    def call(self, encoder_inputs, decoder_inputs, **kwargs):
        if not self.built:
            ids = torch.as_tensor(encoder_inputs)
            self.build(ids.device if ids.is_cuda else "cuda")
        enc_seed, dec_seed = self._next_seed(), self._next_seed()
        self.last_seeds = (enc_seed, dec_seed)
        encoder_encodings, encoder_masks = self.encoder(encoder_inputs, enc_seed)
        return self.decoder([decoder_inputs, encoder_encodings, encoder_masks], dec_seed)

    forward = call

    def reset_calls(self):
        """rewinds the dropout streams of the model and of every attention layer inside"""
        self._calls = 0
        for m in self.modules():
            if isinstance(m, MultiHeadAttention):
                m._calls = 0

    def get_config(self):
        config = {
            "vocab_size": self._vocab_size,
            "model_dim": self._model_dim,
            "n_heads": self._n_heads,
            "encoder_stack": self._encoder_stack,
            "decoder_stack": self._decoder_stack,
            "feed_forward_size": self._feed_forward_size,
            "dropout_rate": self._dropout_rate
        }
        return {**self._kwargs, **config}


class Noam:
    """The reference's Keras callback as a scheduler object over an optimizer of this package:
    lr = model_dim^-0.5 * min(step^-0.5, step * warmup_steps^-1.5), set on every parameter group."""

    def __init__(self, model_dim, step_num=0, warmup_steps=4000, verbose=False, optimizer=None):
        self._model_dim = model_dim
        self._step_num = step_num
        self._warmup_steps = warmup_steps
        self.verbose = verbose
        self.optimizer = optimizer

    def set_optimizer(self, optimizer):
        self.optimizer = optimizer
        return self

    @property
    def lr(self):
        return self.optimizer.param_groups[0]["lr"]

    def _set(self, lr):
        for group in self.optimizer.param_groups:
            group["lr"] = float(lr)

    def on_train_begin(self, logs=None):
        self._set(self._model_dim ** -.5 * self._warmup_steps ** -1.5)

    def on_batch_end(self, epoch, logs=None):
        self._step_num += 1
        self._set(self._model_dim ** -.5 * min(self._step_num ** -.5, self._step_num * self._warmup_steps ** -1.5))

    def on_epoch_begin(self, epoch, logs=None):
        if self.verbose:
            print("epoch %d: learning rate %.6g" % (epoch, self.lr))

    def on_epoch_end(self, epoch, logs=None):
        if logs is not None:
            logs['lr'] = self.lr


def label_smoothing(inputs, epsilon=0.1):
    output_dim = inputs.shape[-1]
    return (1 - epsilon) * inputs + (epsilon / output_dim)
