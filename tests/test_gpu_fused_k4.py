"""GPU parity: the first-layer dgrad with K4's unique-row pass as its epilogue (dr_h2_dgrad_emb_sgd + dr_emb_pool_bwd_sorted parts | 8)
against the two launches it replaces (dr_h2_linear_nt into d_concat, then dr_emb_pool_bwd_sorted).  The epilogue repeats K4's
arithmetic operation for operation, so tables, first-order weights and bias must come out BIT-identical -- which carries every
oracle-backed tolerance of the K4 / engine tests over to the fused step (autodiff of keras/models/ranking/deepfm.py:30-34,44-45 and
fm.py:23-37 of the reference w.r.t. the embedding tables)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from deep_recommenders_amd import ops as _ops
    return _ops


def _setup(ops, B, F, V, H, n_dense, seed, skew=False, missing=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    D = 64
    if skew:
        ids = np.minimum((rng.pareto(1.05, size=(B, F)) * 3).astype(np.int64), V - 1)      # hot rows: shared by hundreds of slots
    else:
        ids = rng.integers(0, V, size=(B, F))
    if missing:
        ids[rng.random((B, F)) < missing] = -1
    ids = torch.as_tensor(ids).cuda()
    row_base = (torch.arange(F, dtype=torch.int64) * V).cuda()
    R = F * V
    table = torch.randn((R, D), device="cuda", generator=g) * 0.125
    lin = torch.randn(R, device="cuda", generator=g) * 0.01
    in_dim = F * D + n_dense
    W = torch.randn((in_dim, H), device="cuda", generator=g) / in_dim ** 0.5
    dy = torch.randn((B, H), device="cuda", generator=g) * (torch.rand((B, H), device="cuda", generator=g) > 0.5) / B
    dl = torch.randn(B, device="cuda", generator=g) / B
    # what the forward leaves behind: sum_x, the first-order weight every slot read
    idc = ids.clamp_min(0) + row_base[None, :]
    x = table[idc] * (ids >= 0)[..., None]
    sum_x = x.sum(1).contiguous()
    lin_old_t = lin[idc].t().contiguous()
    return dict(D=D, R=R, ids=ids, row_base=row_base, table=table, lin=lin, W=W, dy=dy, dl=dl, sum_x=sum_x, lin_old_t=lin_old_t, in_dim=in_dim)


def _run(ops, s, fused, lr=0.05):
    B, F = s["ids"].shape
    D, R = s["D"], s["R"]
    table, lin, bias = s["table"].clone(), s["lin"].clone(), torch.zeros(1, device="cuda")
    plan = ops.emb_sort_slots(s["ids"], s["row_base"], R)
    wp = ops.H2WeightPlanes(s["W"])
    dy_am = ops.h2_amax(s["dy"])
    tab_am = ops.h2_amax(table)
    ld = (s["in_dim"] + 3) // 4 * 4
    d_concat = torch.full((B, ld), float("nan"), device="cuda")
    xs = torch.full((B * F, D), float("nan"), device="cuda")
    ops.emb_snapshot_sorted_rows(plan, table, R, xs)
    k4 = lambda parts: ops.emb_pool_bwd_sorted(s["ids"], s["row_base"], plan, D, R, d_concat, s["dl"], -lr, table, lin, bias, sum_x=s["sum_x"],
                                               x_sorted=xs, parts=parts, lin_old_t=s["lin_old_t"], table_amax=tab_am)
    if fused:
        ids_t = ops.ids_transpose_i32(s["ids"])
        ops.h2_dgrad_emb_sgd(s["dy"], dy_am, wp.w, ids_t, plan, s["row_base"], table, lin, s["lin_old_t"], s["sum_x"], s["dl"], -lr, d_concat,
                             table_amax=tab_am)
        k4(1 | 8)
        k4(2 | 8)
    else:
        ops.h2_linear_nt(s["dy"], dy_am, wp.w, out=d_concat[:, :s["in_dim"]])
        k4(1)
        k4(2)
    torch.cuda.synchronize()
    return table, lin, bias, tab_am.clone(), plan, d_concat


SHAPES = [
    (1024, 6, 5000, 64, 0, False, 0.0),          # interior row tiles, 1.5 column tiles
    (1000, 5, 300, 96, 13, False, 0.05),         # ragged last row tile, many shared rows, missing ids, dense columns behind the embeddings
    (2500, 9, 200000, 256, 13, False, 0.0),      # mostly unique rows, K = 256 (the bench layer's width), 3 column tiles
    (3000, 4, 4000, 32, 0, True, 0.02),          # Zipf-like ids: hot rows through the duplicate pass
]


@pytest.mark.parametrize("B,F,V,H,n_dense,skew,missing", SHAPES)
def test_fused_dgrad_k4_is_bit_identical_to_dgrad_then_k4(ops, B, F, V, H, n_dense, skew, missing):
    s = _setup(ops, B, F, V, H, n_dense, seed=B + F, skew=skew, missing=missing)
    t0, l0, b0, a0, plan, _ = _run(ops, s, fused=False)
    t1, l1, b1, a1, _, _ = _run(ops, s, fused=True)
    uniq = int(plan.flags[:B * F].sum().item())
    assert 0 < uniq <= B * F
    assert not torch.equal(t0, s["table"])                                  # the step did move the table
    assert torch.equal(t1, t0), "tables differ: %d elements" % int((t1 != t0).sum().item())
    assert torch.equal(l1, l0)
    assert torch.equal(b1, b0)
    assert torch.equal(a1, a0)                                              # the table's amax record as K4 leaves it


@pytest.mark.parametrize("B,F,V,H,n_dense,skew,missing", SHAPES + [(1500, 7, 100000, 128, 13, False, 0.0)])
def test_fused_dgrad_k4_against_fp64(ops, B, F, V, H, n_dense, skew, missing):
    """... and the whole backward -- fused dgrad + unique rows, duplicate pass, hot rows -- against a float64 restatement of the update:
    EVERY touched row and first-order weight (the gradient summed over all slots that share the row, x read before the update, a
    missing id contributing nothing), every other row bit-identical, the first-order bias against -lr sum(dl), and what the launch
    leaves in d_concat for the duplicate pass (the rows of the slots that are not unique) against dy W^T.  The fused launch documents
    d_concat as [M, >= 64 F]: it does not write the dense features' columns (nothing trains them), so those are compared on the
    unfused dgrad, which does.
    Bounds: 2e-6 max |want| on rows (and, relative to max |dx|, on d_concat), 1e-7 on first-order weights; the bias is one fp32 sum of
    B terms: B 2^-24 lr sum |dl|, the worst case of any summation order."""
    s = _setup(ops, B, F, V, H, n_dense, seed=B + F, skew=skew, missing=missing)
    lr = 0.05
    t1, l1, b1, _, plan, dc = _run(ops, s, fused=True, lr=lr)
    D, R, in_dim = 64, s["R"], s["in_dim"]
    flags = plan.flags[:B * F].reshape(B, F).bool()
    valid = s["ids"] >= 0
    assert bool((valid & ~flags).any()) and bool(flags.any()) and (missing == 0.0 or bool((~valid).any()))
    idc = s["ids"].clamp_min(0) + s["row_base"][None, :]
    dx_all = s["dy"].double() @ s["W"].double().t()
    dx = dx_all[:, :F * D].reshape(B, F, D)
    dl = s["dl"].double()
    x = s["table"][idc].double()
    g = (dx + dl[:, None, None] * (s["sum_x"].double()[:, None, :] - x)) * valid[..., None]
    G = torch.zeros((R, D), dtype=torch.float64, device="cuda").index_add_(0, idc.reshape(-1), g.reshape(-1, D))
    GL = torch.zeros(R, dtype=torch.float64, device="cuda").index_add_(0, idc.reshape(-1), (dl[:, None] * valid).reshape(-1))
    rows = torch.unique(idc[valid])
    cnt = torch.bincount(idc[valid], minlength=R)
    assert not skew or int(cnt.max()) > 32                                  # (the skewed case does reach the parked-pieces path)
    want = s["table"][rows].double() - lr * G[rows]
    err = (t1[rows].double() - want).abs().max().item()
    print("rows: worst |err| %.3e, bound %.3e" % (err, 2e-6 * want.abs().max().item()))
    assert err <= 2e-6 * want.abs().max().item()
    wl = s["lin"][rows].double() - lr * GL[rows]
    err_l = (l1[rows].double() - wl).abs().max().item()
    print("first-order weights: worst |err| %.3e, bound 1e-7" % err_l)
    assert err_l <= 1e-7
    rest = torch.ones(R, dtype=torch.bool, device="cuda")
    rest[rows] = False
    assert torch.equal(t1[rest], s["table"][rest]) and torch.equal(l1[rest], s["lin"][rest]), "a row no slot looked up changed"
    want_b = -lr * dl.sum().item()
    tol_b = B * 2.0 ** -24 * lr * dl.abs().sum().item()
    print("first-order bias: |err| %.3e, bound %.3e" % (abs(b1.item() - want_b), tol_b))
    assert abs(b1.item() - want_b) <= tol_b
    scale = dx_all.abs().max().item()
    got = dc[:, :F * D].reshape(B, F, D)[~flags].double()
    err_d = (got - dx[~flags]).abs().max().item()
    print("d_concat rows of the non-unique slots: worst |err| %.3e, bound %.3e" % (err_d, 2e-6 * scale))
    assert err_d <= 2e-6 * scale
    if n_dense:
        dc0 = _run(ops, s, fused=False, lr=lr)[5]
        err_n = (dc0[:, F * D:in_dim].double() - dx_all[:, F * D:]).abs().max().item()
        print("d_concat dense columns (unfused dgrad): worst |err| %.3e, bound %.3e" % (err_n, 2e-6 * scale))
        assert err_n <= 2e-6 * scale


@pytest.mark.parametrize("V,zipf", [(3000, False), (200000, False), (50000, True)])
def test_engine_with_fused_k4_is_bit_identical_to_the_three_kernel_backward(V, zipf, monkeypatch):
    """DeepFMEngine's default step (wgrad -> dgrad + K4's unique rows -> duplicate pass) against DR_FUSE_K4=0 (dgrad -> wgrad -> K4):
    same arithmetic in every kernel, so parameters and losses must be bit-identical over prefetched steps -- many shared rows
    (V = 3000), mostly unique rows, and a skewed batch whose hot rows take the parked-pieces path."""
    from deep_recommenders_amd.engine import DeepFMEngine
    F, B, Nd, D = 5, 2304, 3, 64
    g = torch.Generator(device="cuda")
    g.manual_seed(21)
    def keys():
        if zipf:
            u = torch.rand((B, F), device="cuda", generator=g)
            return (1.0 / (u + 1e-4)).long()                      # heavy head: a few keys hundreds of times
        return torch.randint(0, 10**12, (B, F), device="cuda", generator=g)
    batches = [(keys(), torch.rand((B, Nd), device="cuda", generator=g), (torch.rand(B, device="cuda", generator=g) < 0.3).float())
               for _ in range(3)]

    def run():
        eng = DeepFMEngine(F, V, D, [256, 16], B, num_dense=Nd, lr=0.05, seed=3, lin_init_std=0.1)
        losses = []
        for n in range(5):
            k, d, l = batches[n % 3]
            nk, nd = batches[(n + 1) % 3][0], batches[(n + 1) % 3][1]
            losses.append(float(eng.train_step(k, d, l, next_keys=nk, next_dense=nd).item()))
        torch.cuda.synchronize()
        return eng, losses
    fused, l1 = run()
    assert fused.fuse_k4 and fused.h2
    monkeypatch.setenv("DR_FUSE_K4", "0")
    plain, l0 = run()
    assert not plain.fuse_k4
    assert l1 == l0
    assert torch.equal(fused.table, plain.table) and torch.equal(fused.lin_w, plain.lin_w) and torch.equal(fused.lin_bias, plain.lin_bias)
    assert torch.equal(fused.flat_params, plain.flat_params)
    assert torch.equal(fused.tab_amax, plain.tab_amax)
