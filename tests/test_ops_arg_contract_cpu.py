"""What an accepted argument of the model-layer and retrieval wrappers in ops turns into, without a device.

The wrappers' argument checks are all that stands between a caller's view and a kernel that addresses memory by the pitch it is told.
The other *_cpu.py files pin what is refused; this file pins the rest: for every pitched, vector, id and table argument of the families
from FFM to IntentGC, in every layout torch hands out, the entry point that is called, every number it is given (the pitches among
them) and, for every pointer, whether it is the caller's storage at the caller's offset or a fresh buffer.

The library is replaced by a recorder (ops.lib / ops.ptr / ops.stream_ptr are looked up by name), so CPU tensors travel the whole
wrapper.  The expectations are literals, read off the wrappers' contracts; nothing in the table is computed by the code under test.
"""
import pytest
import torch

from deep_recommenders_amd import _lib, ops

E = ValueError
NEW = "<fresh buffer>"
NO_LAUNCH = "<no launch>"
f32, i64, i32 = torch.float32, torch.int64, torch.int32


def z(*shape, dtype=f32):
    return torch.zeros(shape, dtype=dtype)


class LD:
    """the slot of argument `arg`'s pitch; `default` is what the default call (contiguous inputs, no buffers given) hands over"""

    def __init__(self, arg, default):
        self.arg, self.default = arg, default


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return _lib.DR_OK
        return entry


def _storage(t):
    return t.untyped_storage()._cdata


@pytest.fixture
def recorder(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(ops, "lib", lambda: rec)
    monkeypatch.setattr(ops, "ptr", lambda t: None if t is None else (_storage(t), t.storage_offset()))
    monkeypatch.setattr(ops, "stream_ptr", lambda: 0)
    return rec


# ---- the calls: smallest legal dims; make(B) gives the keyword arguments, args the expected record of the launch ------------------
# A slot of `args` is a number, None, NEW, "B" (the batch size of the case), LD(...), the name of a caller's tensor (None when the
# caller gives none) or (name, NEW): the caller's tensor, a fresh buffer when the caller gives none.
def _bert_embed(B):     # ids [1, B]: N = L = B tokens
    return dict(ids=z(1, B, dtype=i64), segment=z(1, B, dtype=i64), tok=z(5, 4), pos=z(4, 4), seg=z(2, 4), gamma=z(4), stats=z(B, 2),
                d_out=z(B, 4), d_tok=z(5, 4))


CALLS = {
    # the older families share only the row-width rule: their default calls, D (or H) = 4
    "dot_interact_fwd": (lambda B: dict(dense=None, emb=z(B, 8), F=2, D=4),
                         "dr_dot_interact_fwd", [None, 0, "emb", LD("emb", 8), "B", 2, 4, 0, NEW, 4, 0]),
    "afm_pool_fwd": (lambda B: dict(emb=z(B, 8), W=z(4, 1), b=z(1), h=z(1), F=2),
                     "dr_afm_pool_fwd", ["emb", LD("emb", 8), "W", "b", "h", "B", 2, 4, 1, NEW, 4, NEW, None, 1, 0]),
    "pnn_outer_fwd": (lambda B: dict(emb=z(B, 4), W=z(16, 4), F=1),
                      "dr_pnn_outer_fwd", ["emb", 4, "W", 4, None, 0, "B", 1, 4, 4, NEW, 4, NEW, 4, 0]),
    "gru_seq_fwd": (lambda B: dict(xp=z(B, 1, 12), U=z(4, 12)),
                    "dr_gru_seq_fwd", ["xp", 12, "U", None, None, None, "B", 1, 4, NEW, 4, NEW, 0]),
    "seq_attn_fwd": (lambda B: dict(hs=z(B, 1, 4), q=z(B, 4)),
                     "dr_seq_attn_fwd", ["hs", 4, "q", None, "B", 1, 4, NEW, 0]),
    "ffm_fwd": (lambda B: dict(rows=z(B, 16), F=2, k=4),
                "dr_ffm_fwd", ["rows", LD("rows", 16), "B", 2, 4, NEW, 0]),
    "ffm_bwd": (lambda B: dict(rows=z(B, 16), F=2, k=4, d_inter=z(B)),
                "dr_ffm_bwd", ["rows", LD("rows", 16), "d_inter", "B", 2, 4, ("d_rows", NEW), LD("d_rows", 16), 0]),
    "ffm_gather_fwd": (lambda B: dict(ids=z(B, 2, dtype=i64), row_base=z(2, dtype=i64), table=z(5, 8), F=2, k=4),
                       "dr_ffm_gather_fwd", ["ids", "B", 2, "row_base", "table", 4, "lin_w", "lin_bias", NEW, None, 0]),
    "ffm_gather_bwd": (lambda B: dict(ids=z(B, 2, dtype=i64), row_base=z(2, dtype=i64), table=z(5, 8), F=2, k=4, d_inter=z(B)),
                       "dr_ffm_gather_bwd", ["ids", "B", 2, "row_base", "table", 4, "d_inter", ("d_rows", NEW), LD("d_rows", 16), 0]),
    "bi_interaction_fwd": (lambda B: dict(rows=z(B, 4), F=1, D=4),
                           "dr_bi_interact_fwd", ["rows", LD("rows", 4), "B", 1, 4, ("out", NEW), LD("out", 4), 0]),
    "bi_interaction_bwd": (lambda B: dict(rows=z(B, 4), F=1, D=4, d_out=z(B, 4)),
                           "dr_bi_interact_bwd", ["rows", LD("rows", 4), "d_out", LD("d_out", 4), "B", 1, 4, ("d_rows", NEW),
                                                  LD("d_rows", 4), 0]),
    "bi_interaction_gather_fwd": (lambda B: dict(ids=z(B, 1, dtype=i64), row_base=z(1, dtype=i64), table=z(5, 4), F=1, D=4),
                                  "dr_bi_interact_gather_fwd", ["ids", "B", 1, "row_base", "table", 4, "lin_w", "lin_bias", ("out", NEW),
                                                                LD("out", 4), None, 0]),
    "bi_interaction_gather_bwd": (lambda B: dict(ids=z(B, 1, dtype=i64), row_base=z(1, dtype=i64), table=z(5, 4), F=1, D=4, d_out=z(B, 4)),
                                  "dr_bi_interact_gather_bwd", ["ids", "B", 1, "row_base", "table", 4, "d_out", LD("d_out", 4),
                                                                ("d_rows", NEW), LD("d_rows", 4), 0]),
    "lsplm_fwd": (lambda B: dict(ids=z(B, 1, dtype=i64), F=1, col_start=None, row_base=z(1, dtype=i64), table=z(5, 4), m=2, bias=z(4)),
                  "dr_lsplm_fwd", ["ids", "B", 1, 1, "col_start", "row_base", "table", 2, "bias", ("z", NEW), LD("z", 4), NEW, NEW, 0]),
    "lsplm_bwd": (lambda B: dict(z=z(B, 4), F=1, m=2, d_p=z(B)),
                  "dr_lsplm_bwd", ["z", LD("z", 4), "d_p", "B", 1, 2, ("d_z", NEW), LD("d_z", 4), ("d_rows", NEW), LD("d_rows", 4), 0]),
    "lsplm_loss_fwd": (lambda B: dict(ids=z(B, 1, dtype=i64), F=1, col_start=None, row_base=z(1, dtype=i64), table=z(5, 4), m=2,
                                      bias=z(4), labels=z(B)),
                       "dr_lsplm_loss_fwd", ["ids", "B", 1, 1, "col_start", "row_base", "table", 2, "bias", "labels", "sample_weight", 1.0,
                                             NEW, NEW, NEW, ("d_z", NEW), LD("d_z", 4), ("d_rows", NEW), LD("d_rows", 4), 0]),
    "lsplm_bias_grad": (lambda B: dict(d_z=z(B, 4), m=2),
                        "dr_lsplm_bias_grad", ["d_z", LD("d_z", 4), "B", 2, NEW, NEW, 4, 0]),
    # SGNS with K = 0 (no negatives) and K = 1, the one-pass training form (row_scale) and the plain forward
    "sgns_fwd": (lambda B: dict(in_table=z(5, 4), out_table=z(6, 4), centers=z(B, dtype=i64), contexts=z(B, dtype=i64)),
                 "dr_sgns_fwd", ["in_table", "out_table", 4, "centers", "contexts", None, "B", 0, "sample_weight", 1, 0.0, NEW, NEW, None,
                                 None, 0, None, 0, 0]),
    "sgns_fwd/K0": (lambda B: dict(in_table=z(5, 4), out_table=z(6, 4), centers=z(B, dtype=i64), contexts=z(B, dtype=i64), row_scale=0.5),
                    "dr_sgns_fwd", ["in_table", "out_table", 4, "centers", "contexts", None, "B", 0, "sample_weight", 1, 0.5, NEW, NEW, None,
                                    ("d_center", NEW), LD("d_center", 4), ("d_ctx", NEW), LD("d_ctx", 4), 0]),
    "sgns_fwd/K1": (lambda B: dict(in_table=z(5, 4), out_table=z(6, 4), centers=z(B, dtype=i64), contexts=z(B, dtype=i64),
                                   negatives=z(B, 1, dtype=i64), row_scale=0.5),
                    "dr_sgns_fwd", ["in_table", "out_table", 4, "centers", "contexts", "negatives", "B", 1, "sample_weight", 1, 0.5, NEW, NEW,
                                    None, ("d_center", NEW), LD("d_center", 4), ("d_ctx", NEW), LD("d_ctx", 8), 0]),
    "sgns_bwd/K0": (lambda B: dict(in_table=z(5, 4), out_table=z(6, 4), centers=z(B, dtype=i64), contexts=z(B, dtype=i64), negatives=None,
                                   coeff=z(B, 1), d_loss=z(B)),
                    "dr_sgns_bwd", ["in_table", "out_table", 4, "centers", "contexts", None, "B", 0, 1, "coeff", "d_loss", ("d_center", NEW),
                                    LD("d_center", 4), ("d_ctx", NEW), LD("d_ctx", 4), 0]),
    "sgns_bwd/K1": (lambda B: dict(in_table=z(5, 4), out_table=z(6, 4), centers=z(B, dtype=i64), contexts=z(B, dtype=i64),
                                   negatives=z(B, 1, dtype=i64), coeff=z(B, 2), d_loss=z(B)),
                    "dr_sgns_bwd", ["in_table", "out_table", 4, "centers", "contexts", "negatives", "B", 1, 1, "coeff", "d_loss",
                                    ("d_center", NEW), LD("d_center", 4), ("d_ctx", NEW), LD("d_ctx", 8), 0]),
    # EGES with S = 1 field, P = 1 positive, K = 0
    "eges_fwd": (lambda B: dict(side_table=z(5, 4), row_base=z(1, dtype=i64), side_ids=z(B, 1, dtype=i64), att=None, att_ids=None,
                                out_table=z(6, 4), contexts=z(B, dtype=i64), row_scale=0.5),
                 "dr_eges_fwd", ["side_table", 4, "row_base", "side_ids", 1, "att", LD("att", 0), "att_ids", "out_table", "contexts", 1, None, 0,
                                 "B", "sample_weight", 1, 0.5, NEW, NEW, NEW, None, ("d_side", NEW), LD("d_side", 4), ("d_att", NEW), 4,
                                 ("d_ctx", NEW), LD("d_ctx", 4), 0]),
    "eges_fwd/att": (lambda B: dict(side_table=z(5, 4), row_base=z(1, dtype=i64), side_ids=z(B, 1, dtype=i64), att=z(3, 4),
                                    att_ids=z(B, dtype=i64), out_table=z(6, 4), contexts=z(B, dtype=i64)),
                     "dr_eges_fwd", ["side_table", 4, "row_base", "side_ids", 1, "att", LD("att", 4), "att_ids", "out_table", "contexts", 1, None,
                                     0, "B", "sample_weight", 1, 0.0, NEW, NEW, NEW, None, None, 0, None, 0, None, 0, 0]),
    "eges_embed/att": (lambda B: dict(side_table=z(5, 4), row_base=z(1, dtype=i64), side_ids=z(B, 1, dtype=i64), att=z(3, 4),
                                      att_ids=z(B, dtype=i64)),
                       "dr_eges_embed", ["side_table", 4, "row_base", "side_ids", 1, "att", LD("att", 4), "att_ids", "B", ("out", NEW),
                                         LD("out", 4), 0]),
    "eges_bwd": (lambda B: dict(side_table=z(5, 4), row_base=z(1, dtype=i64), side_ids=z(B, 1, dtype=i64), att=None, att_ids=None,
                                out_table=z(6, 4), contexts=z(B, dtype=i64), negatives=None, coeff=z(B, 1), alpha=z(B, 1), d_loss=z(B)),
                 "dr_eges_bwd", ["side_table", 4, "row_base", "side_ids", 1, "att", "att_ids", "out_table", "contexts", 1, None, 0, "B", 1,
                                 "coeff", "alpha", "d_loss", ("d_side", NEW), LD("d_side", 4), ("d_att", NEW), 4, ("d_ctx", NEW),
                                 LD("d_ctx", 4), 0]),
    "eges_embed": (lambda B: dict(side_table=z(5, 4), row_base=z(1, dtype=i64), side_ids=z(B, 1, dtype=i64)),
                   "dr_eges_embed", ["side_table", 4, "row_base", "side_ids", 1, "att", LD("att", 0), "att_ids", "B", ("out", NEW), LD("out", 4),
                                     0]),
    # the sampled blocks have no pitched argument: vectors only
    "neighbor_sample": (lambda B: dict(row_ptr=z(4, dtype=i64), col=z(3, dtype=i32), n_rows=3, nodes=z(B, dtype=i64), fanout=2, seed=7),
                        "dr_neighbor_sample", ["row_ptr", "col", 3, "nodes", "B", 2, 7, NEW, NEW, 0]),
    "frontier_build": (lambda B: dict(dst=z(B, dtype=i64), nbr=z(B, 1, dtype=i64)),
                       "dr_frontier_build", ["dst", "B", "nbr", "B", 0, NEW, NEW, NEW, NEW, 1, 0]),
    "block_csr": (lambda B: dict(cnt=z(B, dtype=i32), local=z(B, 2, dtype=i32)),
                  "dr_block_csr", ["cnt", "local", "weight", "B", 2, 0, "n_valid", NEW, NEW, NEW, NEW, 1, 0]),
    # sampled softmax: V = 5 classes, D = 4, S = 3 sampled; the recorder's workspace size is 0, so the 16-byte minimum is allocated
    "sampled_softmax_fwd": (lambda B: dict(u=z(B, 4), table=z(5, 4), labels=z(B, dtype=i64), sampled=z(3, dtype=i64)),
                            "dr_sampled_softmax_fwd", ["u", LD("u", 4), "table", 5, 4, "labels", "B", "sampled", 3, "log_q_true",
                                                       "log_q_sampled", "sample_weight", 1, NEW, NEW, NEW, None, NEW, 16, 0]),
    "sampled_softmax_bwd": (lambda B: dict(u=z(B, 4), table=z(5, 4), labels=z(B, dtype=i64), sampled=z(3, dtype=i64), true_logit=z(B),
                                           row_lse=z(B)),
                            "dr_sampled_softmax_bwd", ["u", LD("u", 4), "table", 5, 4, "labels", "B", "sampled", 3, "log_q_sampled",
                                                       "sample_weight", 1, 1.0, "true_logit", "row_lse", ("d_u", NEW), LD("d_u", 4), NEW, NEW,
                                                       NEW, 16, 0]),
    # margin rank: D = 4, S = 3 negatives of their own, cosine (code 1), no hard-negative lists
    "margin_rank_fwd": (lambda B: dict(q=z(B, 4), pos=z(B, 4), neg=z(3, 4)),
                        "dr_margin_rank_fwd", ["q", LD("q", 4), "pos", LD("pos", 4), "neg", LD("neg", 4), 4, "B", "rows of neg", "pos_ids",
                                               "neg_ids", "sample_weight", 0.2, 1, 0, 0, 1e-12, NEW, NEW, NEW, None, None, NEW, 16, 0]),
    "margin_rank_bwd": (lambda B: dict(q=z(B, 4), pos=z(B, 4), neg=z(3, 4), pos_score=z(B), hard_idx=None),
                        "dr_margin_rank_bwd", ["q", LD("q", 4), "pos", LD("pos", 4), "neg", LD("neg", 4), 4, "B", "rows of neg", "pos_ids",
                                               "neg_ids", "sample_weight", 0.2, 1, 0, 0, 1e-12, 1.0, "pos_score", None, ("d_q", NEW),
                                               LD("d_q", 4), NEW, NEW, NEW, 16, 0]),
    # BERT: [B, 4] matrices; no pitch rule beyond >= N
    "gelu_fwd": (lambda B: dict(z=z(B, 4)),
                 "dr_gelu_fwd", ["z", LD("z", 4), "B", 4, ("out", NEW), LD("out", 4), 0]),
    "gelu_bwd_": (lambda B: dict(z=z(B, 4), dy=z(B, 4)),
                  "dr_gelu_bwd", ["z", LD("z", 4), "dy", LD("dy", 4), "B", 4, 0]),
    "softmax_ce_ids": (lambda B: dict(logits=z(B, 4), labels=z(B, dtype=i64)),
                       "dr_softmax_ce_ids", ["logits", LD("logits", 4), "bias", "labels", "weight", "B", 4, 0.0, 1.0, "denom", 0.0,
                                             ("row_loss", NEW), 0, 0]),
    "colsum_add": (lambda B: dict(g=z(B, 4), dst=z(4)),
                   "dr_colsum_add", ["g", LD("g", 4), "B", 4, "dst", NEW, 4, 0]),
    "bert_embed_bwd": (_bert_embed,
                       "dr_bert_embed_bwd", ["ids", "segment", NEW, NEW, "B", "B", "tok", 5, "pos", "seg", 2, "gamma", "stats", 4, "d_out",
                                             LD("d_out", 4), 0.0, 0, NEW, NEW, NEW, "d_tok", NEW, NEW, NEW, 4, 0]),
    # IntentGC: R = 1 neighbour type, L = 1 filter, D = 4, an edgeless block
    "intent_conv_fwd": (lambda B: dict(row_ptr=z(B + 1, dtype=i64), col=z(0, dtype=i32), val=z(0), n_dst=B, R=1, h=z(B, 4), W=z(1, 2),
                                       theta=z(1)),
                        "dr_intent_conv_fwd", ["row_ptr", None, None, "B", 1, "h", LD("h", 4), 4, "W", "theta", 1, 1, ("out", NEW),
                                               LD("out", 4), None, 0]),
    "intent_mix_fwd": (lambda B: dict(h_self=z(B, 4), agg=z(B, 1, 4), W=z(1, 2), theta=z(1)),
                       "dr_intent_mix_fwd", ["h_self", LD("h_self", 4), "agg", "B", 1, 4, "W", "theta", 1, 1, ("out", NEW), LD("out", 4), 0]),
    "intent_conv_bwd": (lambda B: dict(h_self=z(B, 4), agg=z(B, 1, 4), d_out=z(B, 4), W=z(1, 2), theta=z(1)),
                        "dr_intent_conv_bwd", ["h_self", LD("h_self", 4), "agg", "d_out", LD("d_out", 4), "out", LD("out", 0), "W",
                                               "theta", "B", 1, 4, 1, 1, ("d_self", NEW), LD("d_self", 4), NEW, NEW, NEW, NEW, 4, 0]),
}
# the calls that launch for an empty batch too (every other returns its empty outputs before the launch)
LAUNCH_WHEN_EMPTY = {"lsplm_bias_grad", "gelu_fwd", "gelu_bwd_", "softmax_ce_ids", "colsum_add"}


# ---- the layouts of a pitched [rows, cols] fp32 argument ----------------------------------------------------------------------------------
def _off4(rows, cols):
    return torch.zeros(rows * cols + 1)[1:].view(rows, cols)       # starts 4 bytes into the storage


LAYOUTS = {      # name: (rows of the argument for a batch of 2 -- None: the case runs with a batch of that many --, builder)
    "contiguous": (2, lambda r, c: z(r, c)),
    "pitch+4": (2, lambda r, c: z(r, c + 4)[:, :c]),               # a column slice of a wider buffer, the pitch a multiple of 4
    "pitch+2": (2, lambda r, c: z(r, c + 2)[:, :c]),               # the same, the pitch no multiple of 4
    "transposed": (2, lambda r, c: z(c, r).t()),
    "expanded": (2, lambda r, c: z(1, c).expand(r, c)),            # stride 0: every row is the same memory
    "one row": (1, lambda r, c: z(1, c + 2)[:, :c]),               # no pitch to speak of; the stride is no legal one
    "one wide row": (1, lambda r, c: z(1, c + 4)[:, :c]),          # ... the stride is a legal pitch
    "empty": (0, lambda r, c: z(0, c)),
    "off 4 bytes": (2, _off4),
}
ORDER = ["contiguous", "pitch+4", "pitch+2", "transposed", "expanded", "one row", "one wide row", "off 4 bytes"]

# (call, argument, cols, the pitch handed over -- or E -- for each layout of ORDER).  An argument whose row count is not the batch size
# (the negatives of margin rank) is marked by rows=3.  "empty" is checked for every row of the table: no launch, or a launch with B = 0.
PITCHED = [
    # _row_pitch's families: unit column stride, a pitch that is a multiple of 4 and >= cols; one row: its stride if that is legal, else
    # cols rounded up to a multiple of 4; no alignment rule
    ("dot_interact_fwd", "emb", 8, (8, 12, E, E, E, 8, 12, 8)),
    ("afm_pool_fwd", "emb", 8, (8, 12, E, E, E, 8, 12, 8)),
    ("ffm_fwd", "rows", 16, (16, 20, E, E, E, 16, 20, 16)),
    ("ffm_bwd", "rows", 16, (16, 20, E, E, E, 16, 20, 16)),
    ("ffm_bwd", "d_rows", 16, (16, 20, E, E, E, 16, 20, 16)),
    ("ffm_gather_bwd", "d_rows", 16, (16, 20, E, E, E, 16, 20, 16)),
    ("bi_interaction_fwd", "rows", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("bi_interaction_fwd", "out", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("bi_interaction_bwd", "rows", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("bi_interaction_bwd", "d_out", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("bi_interaction_bwd", "d_rows", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("bi_interaction_gather_fwd", "out", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("bi_interaction_gather_bwd", "d_out", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("bi_interaction_gather_bwd", "d_rows", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("lsplm_fwd", "z", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("lsplm_bwd", "z", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("lsplm_bwd", "d_z", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("lsplm_bwd", "d_rows", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("lsplm_loss_fwd", "d_z", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("lsplm_loss_fwd", "d_rows", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("lsplm_bias_grad", "d_z", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("sgns_fwd/K0", "d_center", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("sgns_fwd/K0", "d_ctx", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("sgns_fwd/K1", "d_center", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("sgns_fwd/K1", "d_ctx", 8, (8, 12, E, E, E, 8, 12, 8)),
    ("sgns_bwd/K0", "d_center", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("sgns_bwd/K0", "d_ctx", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("sgns_bwd/K1", "d_center", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("sgns_bwd/K1", "d_ctx", 8, (8, 12, E, E, E, 8, 12, 8)),
    ("eges_fwd", "d_side", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("eges_fwd", "d_ctx", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("eges_bwd", "d_side", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("eges_bwd", "d_ctx", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("eges_embed", "out", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("sampled_softmax_fwd", "u", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("sampled_softmax_bwd", "u", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("sampled_softmax_bwd", "d_u", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("margin_rank_fwd", "q", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("margin_rank_fwd", "pos", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("margin_rank_fwd", "neg", 4, (4, 8, E, E, E, 4, 8, 4), 3),
    ("margin_rank_bwd", "q", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("margin_rank_bwd", "pos", 4, (4, 8, E, E, E, 4, 8, 4)),
    ("margin_rank_bwd", "neg", 4, (4, 8, E, E, E, 4, 8, 4), 3),
    ("margin_rank_bwd", "d_q", 4, (4, 8, E, E, E, 4, 8, 4)),
    # the attention matrix of EGES, att [R_att, >= S]: unit column stride, any pitch >= S; one row: its width
    ("eges_fwd/att", "att", 4, (4, 8, 6, E, E, 4, 4, 4), 3),
    ("eges_embed/att", "att", 4, (4, 8, 6, E, E, 4, 4, 4), 3),
    # BERT's row-wise kernels: unit column stride, any pitch >= N; one row: its stride if >= N, else N
    ("gelu_fwd", "z", 4, (4, 8, 6, E, E, 6, 8, 4)),
    ("gelu_fwd", "out", 4, (4, 8, 6, E, E, 6, 8, 4)),
    ("gelu_bwd_", "z", 4, (4, 8, 6, E, E, 6, 8, 4)),
    ("gelu_bwd_", "dy", 4, (4, 8, 6, E, E, 6, 8, 4)),
    ("softmax_ce_ids", "logits", 4, (4, 8, 6, E, E, 6, 8, 4)),
    ("colsum_add", "g", 4, (4, 8, 6, E, E, 6, 8, 4)),
    ("bert_embed_bwd", "d_out", 4, (4, 8, 6, E, E, 4, 4, 4)),      # d_out.reshape(N, D) gives one row the stride D
    # IntentGC: a multiple of 4 and >= D, a 16-byte aligned base; one row is always handed over with the pitch D
    ("intent_conv_fwd", "h", 4, (4, 8, E, E, E, 4, 4, E)),
    ("intent_conv_fwd", "out", 4, (4, 8, E, E, E, 4, 4, E)),
    ("intent_mix_fwd", "h_self", 4, (4, 8, E, E, E, 4, 4, E)),
    ("intent_mix_fwd", "out", 4, (4, 8, E, E, E, 4, 4, E)),
    ("intent_conv_bwd", "h_self", 4, (4, 8, E, E, E, 4, 4, E)),
    ("intent_conv_bwd", "d_out", 4, (4, 8, E, E, E, 4, 4, E)),
    ("intent_conv_bwd", "out", 4, (4, 8, E, E, E, 4, 4, E)),
    ("intent_conv_bwd", "d_self", 4, (4, 8, E, E, E, 4, 4, E)),
]


def _pitched_cases():
    for row in PITCHED:
        call, arg, cols, lds = row[:4]
        fixed_rows = row[4] if len(row) > 4 else None
        for layout, ld in zip(ORDER, lds):
            rows, build = LAYOUTS[layout]
            if fixed_rows is not None:                                                      # the batch stays 2
                yield pytest.param(call, arg, 2, build(rows if rows != 2 else fixed_rows, cols), ld, id="%s-%s-%s" % (call, arg, layout))
            else:
                yield pytest.param(call, arg, rows, build(rows, cols), ld, id="%s-%s-%s" % (call, arg, layout))
        if fixed_rows is None:
            yield pytest.param(call, arg, 0, z(0, cols), cols if call in LAUNCH_WHEN_EMPTY else NO_LAUNCH, id="%s-%s-empty" % (call, arg))


def _run(recorder, call, B, **given):
    make, kernel, args = CALLS[call]
    kw = make(B)
    kw.update(given)
    getattr(ops, call.split("/")[0])(**kw)
    launches = [a for name, a in recorder.calls if name == kernel]
    return kw, kernel, args, launches


def _check_record(kw, args, got, B, ld_of=None, fresh=()):
    """got: the recorded arguments; ld_of: {argument: the pitch expected for it}; fresh: caller's tensors expected to be copied"""
    mine = {_storage(t) for t in kw.values() if isinstance(t, torch.Tensor)}
    assert len(got) == len(args), (len(got), len(args))
    for i, (want, have) in enumerate(zip(args, got)):
        where = "argument %d of the launch" % i
        if isinstance(want, LD):
            where, want = where + " (the pitch of %s)" % want.arg, (ld_of or {}).get(want.arg, want.default)
        elif isinstance(want, str) and want == "B":
            want = B
        elif isinstance(want, str) and want.startswith("rows of "):
            want = kw[want[len("rows of "):]].shape[0]
        name, absent = want if isinstance(want, tuple) else (want, None)
        if isinstance(name, str) and name != NEW:
            t = kw.get(name)
            if t is not None and name not in fresh:
                assert have == (_storage(t), t.storage_offset()), "%s must be the caller's %s where it lies" % (where, name)
                continue
            name = absent if t is None else NEW
        if name == NEW:
            assert isinstance(have, tuple) and have[0] not in mine, "%s must be a fresh buffer, got %r" % (where, have)
        else:
            assert not isinstance(have, tuple) and have == name and type(have) is type(name), "%s: expected %r, got %r" % (where, name, have)


@pytest.mark.parametrize("call", sorted(CALLS))
@pytest.mark.parametrize("B", [2, 1])
def test_the_default_call_hands_over_what_the_contract_says(recorder, call, B):
    kw, kernel, args, launches = _run(recorder, call, B)
    assert len(launches) == 1, "%s must launch %s once" % (call, kernel)
    _check_record(kw, args, launches[0], B)


@pytest.mark.parametrize("call, arg, B, tensor, ld", list(_pitched_cases()))
def test_a_pitched_argument_in_every_layout(recorder, call, arg, B, tensor, ld):
    if ld is E:
        with pytest.raises(ValueError, match=arg):
            _run(recorder, call, B, **{arg: tensor})
        assert not recorder.calls or all(name != CALLS[call][1] for name, _ in recorder.calls)
        return
    kw, kernel, args, launches = _run(recorder, call, B, **{arg: tensor})
    if ld == NO_LAUNCH:
        assert launches == []
        return
    assert len(launches) == 1
    _check_record(kw, args, launches[0], B, ld_of={arg: ld})


# ---- vectors, ids and tables --------------------------------------------------------------------------------------------------------------
# (call, argument, the tensor for a batch of 2, what happens): E, "kept" (the caller's storage goes to the kernel), "copied" (a fresh
# contiguous copy does) or None (the kernel gets a null pointer)
def _strided(n, dtype=f32):
    return torch.zeros(2 * n, dtype=dtype)[::2]


def _ids_strided(rows, cols, dtype=i64):
    return torch.zeros((rows, 2 * cols), dtype=dtype)[:, ::2]


OTHERS = [
    # one fp32 value per example
    ("ffm_bwd", "d_inter", z(2, dtype=torch.float64), E), ("ffm_bwd", "d_inter", z(3), E), ("ffm_bwd", "d_inter", _strided(2), "copied"),
    ("ffm_bwd", "d_inter", z(2, 1), "kept"),
    ("ffm_gather_bwd", "d_inter", z(2, dtype=torch.float64), E), ("ffm_gather_bwd", "d_inter", z(3), E),
    ("ffm_gather_bwd", "d_inter", _strided(2), "copied"),
    ("lsplm_bwd", "d_p", z(2, dtype=torch.float64), E), ("lsplm_bwd", "d_p", z(3), E), ("lsplm_bwd", "d_p", _strided(2), "copied"),
    ("lsplm_bwd", "d_p", None, E),
    ("lsplm_loss_fwd", "labels", z(2, dtype=i64), E), ("lsplm_loss_fwd", "labels", z(1), E), ("lsplm_loss_fwd", "labels", _strided(2), "copied"),
    ("lsplm_loss_fwd", "labels", None, E),
    ("lsplm_loss_fwd", "sample_weight", z(2, dtype=torch.float64), E), ("lsplm_loss_fwd", "sample_weight", z(3), E),
    ("lsplm_loss_fwd", "sample_weight", _strided(2), "copied"), ("lsplm_loss_fwd", "sample_weight", z(2), "kept"),
    ("sgns_fwd", "sample_weight", z(2, dtype=torch.float64), E), ("sgns_fwd", "sample_weight", z(3), E),
    ("sgns_fwd", "sample_weight", _strided(2), "copied"), ("sgns_fwd", "sample_weight", z(2), "kept"),
    ("sgns_bwd/K1", "d_loss", z(2, dtype=torch.float64), E), ("sgns_bwd/K1", "d_loss", z(3), E), ("sgns_bwd/K1", "d_loss", _strided(2), "copied"),
    ("eges_fwd", "sample_weight", z(2, dtype=torch.float64), E), ("eges_fwd", "sample_weight", z(3), E),
    ("eges_fwd", "sample_weight", _strided(2), "copied"), ("eges_fwd", "sample_weight", z(2), "kept"),
    ("eges_bwd", "d_loss", z(2, dtype=torch.float64), E), ("eges_bwd", "d_loss", z(3), E), ("eges_bwd", "d_loss", _strided(2), "copied"),
    ("sampled_softmax_fwd", "labels", z(2, dtype=i32), E), ("sampled_softmax_fwd", "labels", z(3, dtype=i64), E),
    ("sampled_softmax_fwd", "labels", _strided(2, i64), "copied"), ("sampled_softmax_fwd", "labels", z(2, 1, dtype=i64), "kept"),
    ("sampled_softmax_fwd", "log_q_true", z(2, dtype=torch.float64), E), ("sampled_softmax_fwd", "log_q_true", z(3), E),
    ("sampled_softmax_fwd", "log_q_true", _strided(2), "copied"), ("sampled_softmax_fwd", "log_q_true", z(2), "kept"),
    ("sampled_softmax_fwd", "log_q_sampled", z(3, dtype=torch.float64), E), ("sampled_softmax_fwd", "log_q_sampled", z(2), E),
    ("sampled_softmax_fwd", "log_q_sampled", _strided(3), "copied"), ("sampled_softmax_fwd", "log_q_sampled", z(3), "kept"),
    ("sampled_softmax_fwd", "sample_weight", z(3), E), ("sampled_softmax_fwd", "sample_weight", _strided(2), "copied"),
    ("sampled_softmax_bwd", "true_logit", z(2, dtype=torch.float64), E), ("sampled_softmax_bwd", "true_logit", z(3), E),
    ("sampled_softmax_bwd", "true_logit", _strided(2), "copied"), ("sampled_softmax_bwd", "row_lse", z(3), E),
    ("sampled_softmax_bwd", "row_lse", _strided(2), "copied"),
    ("margin_rank_fwd", "pos_ids", z(2, dtype=i32), E), ("margin_rank_fwd", "pos_ids", z(3, dtype=i64), E),
    ("margin_rank_fwd", "pos_ids", _strided(2, i64), "copied"), ("margin_rank_fwd", "pos_ids", z(2, dtype=i64), "kept"),
    ("margin_rank_fwd", "neg_ids", z(3, dtype=i32), E), ("margin_rank_fwd", "neg_ids", z(2, dtype=i64), E),
    ("margin_rank_fwd", "neg_ids", _strided(3, i64), "copied"), ("margin_rank_fwd", "neg_ids", z(3, dtype=i64), "kept"),
    ("margin_rank_fwd", "sample_weight", z(2, dtype=torch.float64), E), ("margin_rank_fwd", "sample_weight", z(3), E),
    ("margin_rank_fwd", "sample_weight", _strided(2), "copied"),
    ("margin_rank_bwd", "pos_score", z(2, dtype=torch.float64), E), ("margin_rank_bwd", "pos_score", z(3), E),
    ("margin_rank_bwd", "pos_score", _strided(2), "copied"),
    # ids [B, F] (or [B, C]), row_base [F], col_start [F + 1]
    ("ffm_gather_fwd", "ids", z(2, 2, dtype=i32), E), ("ffm_gather_fwd", "ids", z(2, 3, dtype=i64), E), ("ffm_gather_fwd", "ids", z(4, dtype=i64), E),
    ("ffm_gather_fwd", "ids", _ids_strided(2, 2), "copied"),
    ("ffm_gather_fwd", "row_base", z(2, dtype=i32), E), ("ffm_gather_fwd", "row_base", z(3, dtype=i64), E),
    ("ffm_gather_fwd", "row_base", _strided(2, i64), "copied"),
    ("ffm_gather_bwd", "ids", z(2, 3, dtype=i64), E), ("ffm_gather_bwd", "ids", _ids_strided(2, 2), "copied"),
    ("ffm_gather_bwd", "row_base", z(3, dtype=i64), E), ("ffm_gather_bwd", "row_base", _strided(2, i64), "copied"),
    ("bi_interaction_gather_fwd", "ids", z(2, 1, dtype=i32), E), ("bi_interaction_gather_fwd", "ids", z(2, 2, dtype=i64), E),
    ("bi_interaction_gather_fwd", "ids", _ids_strided(2, 1), "copied"),
    ("bi_interaction_gather_fwd", "row_base", z(1, dtype=i32), E), ("bi_interaction_gather_fwd", "row_base", z(2, dtype=i64), E),
    ("bi_interaction_gather_bwd", "ids", z(2, 2, dtype=i64), E), ("bi_interaction_gather_bwd", "ids", _ids_strided(2, 1), "copied"),
    ("bi_interaction_gather_bwd", "row_base", z(2, dtype=i64), E),
    ("lsplm_fwd", "ids", z(2, 1, dtype=i32), E), ("lsplm_fwd", "ids", z(2, 2, dtype=i64), E), ("lsplm_fwd", "ids", z(2, dtype=i64), E),
    ("lsplm_fwd", "ids", _ids_strided(2, 1), "copied"),
    ("lsplm_fwd", "row_base", z(1, dtype=i32), E), ("lsplm_fwd", "row_base", z(2, dtype=i64), E),
    ("lsplm_fwd", "col_start", z(2, dtype=i64), E), ("lsplm_fwd", "col_start", z(3, dtype=i32), E),
    ("lsplm_fwd", "col_start", z(2, dtype=i32), "kept"), ("lsplm_fwd", "col_start", _strided(2, i32), "copied"),
    ("sgns_fwd/K1", "negatives", z(2, 1, dtype=i32), E), ("sgns_fwd/K1", "negatives", z(3, 1, dtype=i64), E),
    ("sgns_fwd/K1", "negatives", z(2, dtype=i64), E), ("sgns_fwd/K1", "negatives", _ids_strided(2, 1), "copied"),
    ("sgns_fwd", "centers", z(2, dtype=i32), E), ("sgns_fwd", "centers", z(2, 1, dtype=i64), E), ("sgns_fwd", "centers", _strided(2, i64), "copied"),
    ("sgns_fwd", "contexts", z(3, dtype=i64), E), ("sgns_fwd", "contexts", _strided(2, i64), "copied"),
    ("eges_fwd", "side_ids", z(2, 1, dtype=i32), E), ("eges_fwd", "side_ids", z(2, dtype=i64), E), ("eges_fwd", "side_ids", z(2, 17, dtype=i64), E),
    ("eges_fwd", "side_ids", _ids_strided(2, 1), "copied"),
    ("eges_fwd", "row_base", z(1, dtype=i32), E), ("eges_fwd", "row_base", z(2, dtype=i64), E), ("eges_fwd", "row_base", z(1, 1, dtype=i64), E),
    ("eges_fwd", "contexts", z(2, dtype=i32), E), ("eges_fwd", "contexts", z(3, dtype=i64), E), ("eges_fwd", "contexts", z(2, 1, dtype=i64), "kept"),
    ("eges_fwd", "contexts", _ids_strided(2, 1), "copied"),
    ("eges_fwd", "negatives", z(2, 1, dtype=i32), E), ("eges_fwd", "negatives", z(3, 1, dtype=i64), E),
    ("eges_embed", "side_ids", z(2, 1, dtype=i32), E), ("eges_embed", "side_ids", _ids_strided(2, 1), "copied"),
    ("sampled_softmax_fwd", "sampled", z(3, dtype=i32), E), ("sampled_softmax_fwd", "sampled", z(3, 1, dtype=i64), E),
    ("neighbor_sample", "nodes", z(2, dtype=i32), E), ("neighbor_sample", "nodes", z(2, 1, dtype=i64), E),
    ("neighbor_sample", "nodes", _strided(2, i64), "copied"), ("neighbor_sample", "row_ptr", z(5, dtype=i64), E),
    ("neighbor_sample", "col", z(3, dtype=i64), E), ("neighbor_sample", "col", _strided(3, i32), "copied"),
    ("frontier_build", "dst", z(2, dtype=i32), E), ("frontier_build", "dst", _strided(2, i64), "copied"),
    ("frontier_build", "nbr", z(2, 1, dtype=i32), E), ("frontier_build", "nbr", _ids_strided(2, 1), "copied"),
    ("block_csr", "cnt", z(2, dtype=i64), E), ("block_csr", "cnt", z(3, dtype=i32), E), ("block_csr", "cnt", _strided(2, i32), "copied"),
    ("block_csr", "local", z(2, 2, dtype=i64), E), ("block_csr", "local", _ids_strided(2, 2, i32), "copied"),
    ("block_csr", "weight", z(2, 3), E), ("block_csr", "weight", z(2, 2), "kept"), ("block_csr", "n_valid", z(2, dtype=i64), E),
    ("block_csr", "n_valid", z(1, dtype=i64), "kept"),
    # tables: contiguous fp32 [R, cols]; a view is refused, never copied
    ("ffm_gather_fwd", "table", z(5, 8, dtype=torch.float64), E), ("ffm_gather_fwd", "table", z(5, 12), E),
    ("ffm_gather_fwd", "table", z(5, 16)[:, :8], E), ("ffm_gather_fwd", "table", z(40), E),
    ("ffm_gather_bwd", "table", z(5, 12), E), ("ffm_gather_bwd", "table", z(5, 16)[:, :8], E),
    ("bi_interaction_gather_fwd", "table", z(5, 4, dtype=torch.float64), E), ("bi_interaction_gather_fwd", "table", z(5, 8), E),
    ("bi_interaction_gather_fwd", "table", z(5, 8)[:, :4], E),
    ("bi_interaction_gather_bwd", "table", z(5, 8), E), ("bi_interaction_gather_bwd", "table", z(5, 8)[:, :4], E),
    ("lsplm_fwd", "table", z(5, 4, dtype=torch.float64), E), ("lsplm_fwd", "table", z(5, 8), E), ("lsplm_fwd", "table", z(5, 8)[:, :4], E),
    ("lsplm_loss_fwd", "table", z(5, 8), E), ("lsplm_loss_fwd", "table", z(5, 8)[:, :4], E),
    ("sgns_fwd", "in_table", z(5, 4, dtype=torch.float64), E), ("sgns_fwd", "in_table", z(5, 6), E), ("sgns_fwd", "in_table", z(5, 8)[:, :4], E),
    ("sgns_fwd", "out_table", z(6, 8), E), ("sgns_fwd", "out_table", z(6, 8)[:, :4], E), ("sgns_fwd", "out_table", z(4, 6).t(), E),
    ("sgns_bwd/K1", "in_table", z(5, 8)[:, :4], E), ("sgns_bwd/K1", "out_table", z(6, 8)[:, :4], E),
    ("eges_fwd", "side_table", z(5, 4, dtype=torch.float64), E), ("eges_fwd", "side_table", z(5, 6), E),
    ("eges_fwd", "side_table", z(5, 8)[:, :4], E), ("eges_fwd", "out_table", z(6, 8), E), ("eges_fwd", "out_table", z(6, 8)[:, :4], E),
    ("eges_embed", "side_table", z(5, 8)[:, :4], E),
    ("sampled_softmax_fwd", "table", z(5, 4, dtype=torch.float64), E), ("sampled_softmax_fwd", "table", z(5, 6), E),
    ("sampled_softmax_fwd", "table", z(5, 8)[:, :4], E), ("sampled_softmax_bwd", "table", z(5, 8)[:, :4], E),
]


@pytest.mark.parametrize("call, arg, tensor, outcome", [pytest.param(*row, id="%s-%s-%d" % (row[0], row[1], i)) for i, row in enumerate(OTHERS)])
def test_a_vector_id_or_table_argument(recorder, call, arg, tensor, outcome):
    if outcome is E:
        with pytest.raises(ValueError):
            _run(recorder, call, 2, **{arg: tensor})
        assert all(name != CALLS[call][1] for name, _ in recorder.calls)
        return
    kw, kernel, args, launches = _run(recorder, call, 2, **{arg: tensor})
    assert len(launches) == 1
    _check_record(kw, args, launches[0], 2, fresh=(arg,) if outcome == "copied" else ())


def test_rows_given_as_contiguous_3d_or_4d_tensors_are_taken_where_they_lie(recorder):
    taken = (("dot_interact_fwd", "emb", z(2, 2, 4), 8), ("afm_pool_fwd", "emb", z(2, 2, 4), 8), ("ffm_fwd", "rows", z(2, 2, 2, 4), 16),
             ("ffm_fwd", "rows", z(2, 2, 8), 16), ("ffm_bwd", "d_rows", z(2, 2, 2, 4), 16), ("bi_interaction_fwd", "rows", z(2, 1, 4), 4),
             ("bi_interaction_bwd", "d_rows", z(2, 1, 4), 4), ("sgns_fwd/K1", "d_ctx", z(2, 2, 4), 8), ("sgns_bwd/K1", "d_ctx", z(2, 2, 4), 8))
    for call, arg, tensor, cols in taken:
        recorder.calls.clear()
        kw, kernel, args, launches = _run(recorder, call, 2, **{arg: tensor})
        assert len(launches) == 1
        _check_record(kw, args, launches[0], 2, ld_of={arg: cols})
    # a view, another trailing shape, another batch size
    refused = (("ffm_fwd", "rows", z(2, 2, 4, 4)[:, :, :2]), ("ffm_fwd", "rows", z(2, 4, 4)), ("bi_interaction_fwd", "rows", z(2, 2, 4)),
               ("bi_interaction_fwd", "rows", z(2, 1, 8)[:, :, :4]), ("sgns_fwd/K1", "d_ctx", z(2, 2, 8)[:, :, :4]),
               ("sgns_fwd/K1", "d_ctx", z(3, 2, 4)))
    for call, arg, tensor in refused:
        with pytest.raises(ValueError):
            _run(recorder, call, 2, **{arg: tensor})
