"""CPU checks of the restatements the GPU tests of EGES / Airbnb compare against (tests/eges_ref.py) and of the host side of the
feature: graph_from_sessions and the ops wrappers' argument checks."""
import numpy as np
import pytest
import torch

import eges_ref as E
import sgns_ref as R
from deep_recommenders_amd import layers, ops
from deep_recommenders_amd.keras.models.retrieval import EGES, Airbnb, graph_from_sessions

# what this file restates and checks the host side of: without these names nothing here has a subject
SUBJECTS = (ops.eges_fwd, ops.eges_bwd, ops.eges_embed, ops.random_walk_weighted, layers.eges_loss, EGES, Airbnb, graph_from_sessions)
DD = torch.float64


def _case(S=4, P=2, K=5, B=14, D=12, seed=0):
    """random float64 tables and logits with every mask pattern of the GPU tests: a missing field first / in the middle / last, all
    fields missing, att_ids = -1, a positive of -1 at j >= 1, contexts[b, 0] = -1, a negative equal to the second positive"""
    g = torch.Generator().manual_seed(seed)
    sizes = [11, 5, 4, 3][:S]
    row_base = torch.tensor(np.concatenate([[0], np.cumsum(sizes[:-1])]).astype(np.int64))
    side_table = torch.randn(sum(sizes), D, generator=g, dtype=DD)
    att = torch.randn(sizes[0], 4, generator=g, dtype=DD)
    out_table = torch.randn(13, D, generator=g, dtype=DD)
    side_ids = torch.stack([torch.randint(0, n, (B,), generator=g) for n in sizes], dim=1)
    att_ids = side_ids[:, 0].clone()
    contexts = torch.randint(0, 13, (B, P), generator=g)
    negatives = torch.randint(0, 13, (B, K), generator=g)
    side_ids[1, 0] = -1
    side_ids[2, min(1, S - 1)] = -1
    side_ids[3, S - 1] = -1
    side_ids[4, :] = -1
    att_ids[5] = -1
    if P > 1:
        contexts[6, 1] = -1
    contexts[7, 0] = -1
    negatives[8, 2] = contexts[8, P - 1]
    negatives[9, 0] = contexts[9, 0]
    negatives[10, 1] = -1
    side_ids[11, 0] = -1                                       # a cold item: no id row, no logits
    att_ids[11] = -1
    w = torch.rand(B, generator=g, dtype=DD) + 0.5
    return dict(side_table=side_table, row_base=row_base, side_ids=side_ids, att=att, att_ids=att_ids, out_table=out_table,
                contexts=contexts, negatives=negatives, w=w)


def _args(c, att=True):
    return (c["side_table"], c["row_base"], c["side_ids"], c["att"] if att else None, c["att_ids"] if att else None, c["out_table"],
            c["contexts"], c["negatives"])


@pytest.mark.parametrize("with_att", [True, False])
@pytest.mark.parametrize("skip_equal", [True, False])
def test_hand_written_gradient_equals_autograd(skip_equal, with_att):
    c = _case()
    for k in ("side_table", "att", "out_table"):
        c[k].requires_grad_(True)
    B = len(c["side_ids"])
    d_loss = torch.rand(B, dtype=DD) + 0.1
    loss, scores, keep, alpha, u = E.loss_expr(*_args(c, with_att), c["w"], skip_equal)
    (loss * d_loss).sum().backward()
    det = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    h = E.hand_grads(*_args(det, with_att), d_loss, det["w"], skip_equal)
    assert torch.equal(keep, h["keep"]) and torch.equal(alpha.detach(), h["alpha"])
    g_side, g_att, g_out = E.table_grads(c["side_table"].shape[0], c["att"].shape[0], c["out_table"].shape[0], c["row_base"], c["side_ids"],
                                         c["att_ids"] if with_att else None, h)
    wants = [(g_side, c["side_table"].grad), (g_out, c["out_table"].grad)]
    if with_att:
        wants.append((g_att, c["att"].grad[:, :4]))
    else:
        assert c["att"].grad is None and (h["d_att"] == 0).all()
    for got, want in wants:
        assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    loss = loss.detach()
    # what the masks mean
    assert float(loss[4]) == 0 and float(loss[7]) == 0 and not keep[4].any() and not keep[7].any()
    assert (h["alpha"][4] == 0).all() and (h["alpha"][7] == 0).all() and (h["d_side"][4] == 0).all() and (h["d_side"][7] == 0).all()
    assert h["alpha"][1, 0] == 0 and h["alpha"][2, 1] == 0 and h["alpha"][3, 3] == 0
    ok = torch.ones(B, dtype=torch.bool)
    ok[[4, 7]] = False
    assert (h["alpha"][ok].sum(1) - 1).abs().max() < 1e-15
    assert torch.allclose(h["alpha"][5], torch.full((4,), 0.25, dtype=DD)) and (h["d_att"][5] == 0).all()
    assert torch.allclose(h["alpha"][11], torch.tensor([0, 1 / 3, 1 / 3, 1 / 3], dtype=DD))       # the cold-start rule
    side = c["side_table"].detach()
    rows = (c["side_ids"][11] + c["row_base"])[1:]
    assert torch.allclose(h["u"][11], side[rows].mean(0))
    assert not keep[6, 1] and keep[6, 0] and not keep[10, 3]
    assert bool(keep[8, 4]) != skip_equal and bool(keep[9, 2]) != skip_equal
    assert (h["g"][~keep] == 0).all() and (h["d_ctx"][~keep] == 0).all()


def test_single_field_single_positive_is_sgns():
    """S = 1, P = 1, no attention: the restatement is sgns_ref's, so the GPU anchor compares like with like"""
    c = _case(S=1, P=1)
    d_loss = torch.rand(len(c["side_ids"]), dtype=DD) + 0.1
    centers, contexts = c["side_ids"][:, 0], c["contexts"][:, 0]
    for skip_equal in (True, False):
        h = E.hand_grads(*_args(c, False), d_loss, c["w"], skip_equal)
        g, d_center, d_ctx, _, _ = R.hand_grads(c["side_table"], c["out_table"], centers, contexts, c["negatives"], d_loss, c["w"], skip_equal)
        assert torch.equal(h["g"], g) and torch.equal(h["d_side"][:, 0], d_center) and torch.equal(h["d_ctx"], d_ctx)
        loss = E.loss_expr(*_args(c, False), c["w"], skip_equal)[0]
        assert torch.equal(loss, R.loss_expr(c["side_table"], c["out_table"], centers, contexts, c["negatives"], c["w"], skip_equal)[0])


def test_weighted_search_rule_takes_each_edge_weight_times():
    row_ptr, col, weights = E.weighted_six_node_graph()
    cum = np.cumsum(weights)
    assert tuple(weights[:4]) == (3, 0, 1, 5)
    for v in range(len(row_ptr) - 1):
        lo, hi = int(row_ptr[v]), int(row_ptr[v + 1])
        total = int(weights[lo:hi].sum())
        taken = np.zeros(len(col), dtype=np.int64)
        for t in range(total):
            taken[E.weighted_pick(cum, lo, hi, t)] += 1
        assert np.array_equal(taken[lo:hi], weights[lo:hi]) and taken.sum() == total          # a zero-weight edge: never


def test_weighted_walk_restatement():
    row_ptr, col, weights = E.weighted_six_node_graph()
    cum = np.cumsum(weights)
    starts = np.asarray([0, 1, 2, 3, 4, 5, -1, 6] * 8, dtype=np.int64)
    walks = E.random_walk_weighted_ref(row_ptr, col, cum, 6, starts, 12, seed=7)
    assert (walks[:, 0] == starts).all()
    zero_edges = {(0, 2), (2, 0), (2, 3), (3, 4)}
    edges = {(i, int(col[e])) for i in range(6) for e in range(row_ptr[i], row_ptr[i + 1])}
    for row in walks:
        for a, b in zip(row[:-1], row[1:]):
            if b >= 0:
                assert (int(a), int(b)) in edges and (int(a), int(b)) not in zero_edges
            else:
                assert a < 0 or a >= 5 or a == 2                # past the graph, isolated, or the row whose total is 0
    assert (walks[starts == 2][:, 1:] == -1).all()
    # unit weights: the uniform walk, bit for bit
    for rp, cl in (R.six_node_graph(), R.dead_end_graph()):
        st = np.arange(-1, len(rp) + 1, dtype=np.int64)
        unit = E.random_walk_weighted_ref(rp, cl, np.arange(1, len(cl) + 1), len(rp) - 1, st, 9, seed=3)
        assert np.array_equal(unit, R.random_walk_ref(rp, cl, len(rp) - 1, st, 9, seed=3))


def test_graph_from_sessions_equals_the_loops():
    import scipy.sparse as sp
    rng = np.random.default_rng(0)
    sessions = [rng.integers(0, 9, size=n).tolist() for n in (5, 1, 0, 12, 2, 7)] + [[3, 3, 3], [0, 8, 0, 8]]
    idx, val, shape = graph_from_sessions(sessions, 9)
    assert shape == (9, 9) and idx.shape == (len(val), 2) and (val == 1).all()
    dense = np.asarray(sp.coo_matrix((val, (idx[:, 0], idx[:, 1])), shape=shape).todense()).astype(np.int64)
    want = E.graph_from_sessions_loops(sessions, 9)
    assert np.array_equal(dense, want) and want[3, 3] >= 2 and want[0, 8] >= 2
    assert graph_from_sessions([], 4)[0].shape == (0, 2)
    with pytest.raises(ValueError):
        graph_from_sessions([[0, 9]], 9)


def test_wrappers_refuse_out_of_domain_arguments():
    """every refusal is a ValueError raised before the library is touched: the tensors live on the CPU"""
    f32, i64 = torch.float32, torch.int64
    good = dict(side_table=torch.zeros((9, 8), dtype=f32), row_base=torch.zeros(2, dtype=i64), side_ids=torch.zeros((3, 2), dtype=i64),
                att=torch.zeros((5, 4), dtype=f32), att_ids=torch.zeros(3, dtype=i64), out_table=torch.zeros((7, 8), dtype=f32),
                contexts=torch.zeros((3, 2), dtype=i64), negatives=torch.zeros((3, 5), dtype=i64))
    bad = [dict(side_table=torch.zeros((9, 6), dtype=f32)), dict(side_table=torch.zeros((9, 260), dtype=f32)),
           dict(side_table=torch.zeros((9, 8), dtype=torch.float64)), dict(side_table=torch.zeros((9, 16), dtype=f32)[:, :8]),
           dict(row_base=torch.zeros(3, dtype=i64)), dict(row_base=torch.zeros(2, dtype=torch.int32)),
           dict(side_ids=torch.zeros((3, 2), dtype=torch.int32)), dict(side_ids=torch.zeros(3, dtype=i64)),
           dict(side_ids=torch.zeros((3, 17), dtype=i64), row_base=torch.zeros(17, dtype=i64), att=None),
           dict(att=torch.zeros((5, 1), dtype=f32)), dict(att_ids=None), dict(att_ids=torch.zeros(4, dtype=i64)),
           dict(out_table=torch.zeros((7, 12), dtype=f32)), dict(contexts=torch.zeros((3, 5), dtype=i64)),
           dict(contexts=torch.zeros((4, 2), dtype=i64)), dict(negatives=torch.zeros((3, 63), dtype=i64)),
           dict(negatives=torch.zeros((2, 5), dtype=i64)), dict(negatives=torch.zeros((3, 5), dtype=torch.int32))]
    order = ("side_table", "row_base", "side_ids", "att", "att_ids", "out_table", "contexts", "negatives")
    for b in bad:
        a = dict(good, **b)
        with pytest.raises(ValueError):
            ops.eges_fwd(*[a[k] for k in order])
        with pytest.raises(ValueError):
            ops.eges_bwd(*[a[k] for k in order], torch.zeros((3, 7), dtype=f32), torch.zeros((3, 2), dtype=f32), torch.zeros(3, dtype=f32))
    g = [good[k] for k in order]
    with pytest.raises(ValueError):
        ops.eges_fwd(*g, sample_weight=torch.zeros(4, dtype=f32))
    with pytest.raises(ValueError):
        ops.eges_fwd(*g, d_side=torch.zeros((3, 16), dtype=f32))                               # buffers without a row_scale
    with pytest.raises(ValueError):
        ops.eges_fwd(*g, row_scale=1.0, d_att=torch.zeros((3, 2), dtype=f32))                  # d_att is [B, pad4(S)]
    with pytest.raises(ValueError):
        ops.eges_fwd(*g, row_scale=1.0, d_side=torch.zeros((3, 18), dtype=f32)[:, :16])        # a pitch that is no multiple of 4
    with pytest.raises(ValueError):
        ops.eges_bwd(*g, torch.zeros((3, 6), dtype=f32), torch.zeros((3, 2), dtype=f32), torch.zeros(3, dtype=f32))
    with pytest.raises(ValueError):
        ops.eges_bwd(*g, torch.zeros((3, 7), dtype=f32), torch.zeros((3, 3), dtype=f32), torch.zeros(3, dtype=f32))
    for b in bad[:12]:
        a = dict(good, **b)
        with pytest.raises(ValueError):
            ops.eges_embed(a["side_table"], a["row_base"], a["side_ids"], a["att"], a["att_ids"])
    with pytest.raises(ValueError):
        ops.eges_embed(good["side_table"], good["row_base"], good["side_ids"], out=torch.zeros((3, 12), dtype=f32))
    rp, col, cum, st = torch.zeros(4, dtype=i64), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=i64), torch.zeros(5, dtype=i64)
    for args in ((rp.int(), col, cum, 3, st, 4), (rp, col.long(), cum, 3, st, 4), (rp, col, cum.int(), 3, st, 4), (rp, col, cum[:1], 3, st, 4),
                 (rp, col, cum, 4, st, 4), (rp, col, cum, 3, st.int(), 4), (rp, col, cum, 3, st, 0)):
        with pytest.raises(ValueError):
            ops.random_walk_weighted(*args, seed=1)
