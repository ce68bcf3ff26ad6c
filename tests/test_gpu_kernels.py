"""GPU parity tests: every C-ABI kernel against the CPU oracle on the same seeded inputs.
Bit-exact for the integer path and for pure-copy floating point; fp32 tolerances are written per test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tf_semantics as O
from oracle import torch_ref as T


@pytest.fixture(scope="module")
def ops():
    from deep_recommenders_amd import ops as _ops
    return _ops


def _dev(a, dtype=None):
    t = torch.as_tensor(a)
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


# ---------------------------------------------------------------- K1
def test_hash_bucket_i64_bit_exact(ops):
    rng = np.random.default_rng(42)
    B, C = 4099, 5
    keys = np.empty((B, C), dtype=np.int64)
    keys[:, 0] = rng.integers(0, 10, size=B)                     # 1 digit  (1-3 byte branch)
    keys[:, 1] = rng.integers(1000, 9999999, size=B)             # 4-7 bytes
    keys[:, 2] = rng.integers(10**8, 10**16, size=B)             # 8-16 bytes
    keys[:, 3] = rng.integers(10**16, 2**63 - 1, size=B)         # 17-19 bytes (17-32 branch)
    keys[:, 4] = rng.integers(-2**63, 2**63 - 1, size=B)         # signed, up to 20 bytes
    keys[::7, 1] = -1                                           # dropped entries
    keys[0, 4] = -2**63
    keys[1, 4] = 2**63 - 1
    keys[2, 4] = 0
    buckets = np.array([10, 6040, 10_000_000, 2**40 + 7, 3952], dtype=np.int64)
    got = ops.hash_bucket_i64(_dev(keys), _dev(buckets)).cpu().numpy()
    for c in range(C):
        want = O.hash_bucket_i64(keys[:, c], int(buckets[c]))
        np.testing.assert_array_equal(got[:, c], want)
    # pass-through column (0 buckets): ids unchanged, -1 stays -1
    got = ops.hash_bucket_i64(_dev(keys[:, :1]), _dev(np.array([0]))).cpu().numpy()
    np.testing.assert_array_equal(got, keys[:, :1])


def test_hash_bucket_i64_digit_boundaries_and_bucket_shapes(ops):
    """Every decimal length boundary (the device builds the text in 8/8/4-digit chunks) against bucket counts that stress the
    Barrett reduction: 1, powers of two, 2^63, primes."""
    ks = [0, 2**63 - 1, -2**63, -2, -10, -99999999, -100000000]
    for e in range(1, 19):
        ks += [10**e - 1, 10**e, 10**e + 1, 5 * 10**e, -(10**e)]
    ks += [10**8 * 3, 10**16 * 7, 10**16 + 10**8, 12345678_00000000, 99999999_99999999, 1_00000000_00000000]
    keys = np.array(ks, dtype=np.int64)
    bks = [1, 2, 3, 4, 1024, 2**32, 2**32 + 1, 2**62, 2**63 - 1, 10_000_000, 6040, 2**40 + 7]
    K = np.repeat(keys[:, None], len(bks), axis=1)
    got = ops.hash_bucket_i64(_dev(K), _dev(np.array(bks, dtype=np.int64))).cpu().numpy()
    for c, nb in enumerate(bks):
        np.testing.assert_array_equal(got[:, c], O.hash_bucket_i64(keys, int(nb)), err_msg=f"buckets={nb}")


def test_hash_bucket_upstream_vectors_on_device(ops):
    got = ops.hash_bucket_strings(["Hello", "TensorFlow", "2.x"], 3).cpu().tolist()
    assert got == [0, 2, 2]
    assert ops.hash_bucket_strings(["1"], 6040).item() == 1529
    assert ops.hash_bucket_i64(_dev(np.array([[1], [2]])), _dev(np.array([100]))).cpu().reshape(-1).tolist() == [49, 59]


def test_hash_bucket_bytes_all_branches(ops):
    rng = np.random.default_rng(7)
    strs = [b""] + [bytes(rng.integers(1, 256, size=n, dtype=np.uint8)) for n in
                    list(range(1, 70)) + [64, 65, 127, 128, 129, 200, 255, 256, 1000]]
    got = ops.hash_bucket_strings(strs, 1_000_003).cpu().numpy()
    want = np.array([-1 if len(s) == 0 else O.fingerprint64(s) % 1_000_003 for s in strs])
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------- K2
def test_vocab_lookup(ops):
    keys = np.array([1, 18, 99, -1, 56, 25, 0], dtype=np.int64)
    vocab = np.array([1, 18, 25, 35, 45, 50, 56], dtype=np.int64)
    got = ops.vocab_lookup_i64(_dev(keys), _dev(vocab)).cpu().numpy()
    want = O.vocab_lookup([int(k) for k in keys], [int(v) for v in vocab])
    want[3] = -1
    np.testing.assert_array_equal(got, want)
    got = ops.vocab_lookup_strings(["F", "M", "Action", "", "FM"], ["F", "M"]).cpu().tolist()
    assert got == [0, 1, -1, -1, -1]


# ---------------------------------------------------------------- K3 / K4
def _rand_problem(rng, B, Ls, Vs, D, p_missing=0.15):
    F = len(Ls)
    col_start = np.concatenate([[0], np.cumsum(Ls)]).astype(np.int32)
    row_base = np.concatenate([[0], np.cumsum(Vs)[:-1]]).astype(np.int64)
    ids = np.full((B, int(col_start[-1])), -1, dtype=np.int64)
    for f in range(F):
        for c in range(col_start[f], col_start[f + 1]):
            col = rng.integers(0, Vs[f], size=B)
            col[rng.random(B) < p_missing] = -1
            ids[:, c] = col
    R = int(np.sum(Vs))
    table = (rng.standard_normal((R, D)) / np.sqrt(D)).astype(np.float32)
    lin_w = rng.standard_normal(R).astype(np.float32)
    return F, col_start, row_base, ids, table, lin_w


@pytest.mark.parametrize("D,Ls", [(16, [1, 1, 1, 1, 1, 3, 1]), (64, [1] * 26), (128, [2, 1, 4]), (12, [1, 2]),
                                  (64, [1] * 70), (4, [1, 1]), (256, [1, 2])])
def test_emb_pool_fwd_matches_oracle(ops, D, Ls):
    rng = np.random.default_rng(42)
    B = 515
    Vs = [int(v) for v in rng.integers(3, 400, size=len(Ls))]
    F, col_start, row_base, ids, table, lin_w = _rand_problem(rng, B, Ls, Vs, D)
    single = all(l == 1 for l in Ls) and F <= 64
    cs = None if single else _dev(col_start)
    concat, sum_x, fm = ops.emb_pool_fwd(_dev(ids), F, cs, _dev(row_base), _dev(table), _dev(lin_w),
                                         _dev(np.array([0.125], np.float32)))
    torch.cuda.synchronize()
    ids_f = [ids[:, col_start[f]:col_start[f + 1]] for f in range(F)]
    tabs = [table[row_base[f]:row_base[f] + Vs[f]] for f in range(F)]
    embs = [O.embedding_mean_pool_fast(t, i) for t, i in zip(tabs, ids_f)]
    want_concat = np.concatenate(embs, 1)
    # pooled rows: pure copy / in-order sum + one divide -> bit-exact
    np.testing.assert_array_equal(concat.cpu().numpy(), want_concat)
    stack = np.stack(embs, 1)
    want_logit = (O.first_order_gather(ids_f, [lin_w[row_base[f]:row_base[f] + Vs[f]] for f in range(F)], 0.125)
                  + O.fm_second_order(stack)).reshape(-1)
    # fp32 reduction order differs (butterfly vs sequential): 1e-5 relative to the magnitude of the terms
    scale = np.abs(want_logit).max() + 1.0
    np.testing.assert_allclose(fm.cpu().numpy(), want_logit, rtol=0, atol=2e-5 * scale)
    np.testing.assert_allclose(sum_x.cpu().numpy(), stack.sum(1), rtol=0, atol=1e-5)


def test_emb_pool_fwd_padded_concat_and_no_fm(ops):
    rng = np.random.default_rng(1)
    F, col_start, row_base, ids, table, lin_w = _rand_problem(rng, 100, [1] * 5, [50] * 5, 16)
    ld = 5 * 16 + 16
    concat, sum_x, fm = ops.emb_pool_fwd(_dev(ids), F, None, _dev(row_base), _dev(table), None, None, ld_concat=ld,
                                         want_sum_x=False, want_fm=False)
    assert sum_x is None and fm is None
    want = np.concatenate([O.embedding_mean_pool_fast(table[row_base[f]:row_base[f] + 50], ids[:, f]) for f in range(5)], 1)
    np.testing.assert_array_equal(concat[:, :80].cpu().numpy(), want)
    assert float(concat[:, 80:].abs().max()) == 0.0


@pytest.mark.parametrize("D,Ls", [(16, [1, 1, 3, 1]), (64, [1] * 26), (128, [2, 1]), (12, [1, 2])])
def test_emb_pool_bwd_matches_autograd_oracle(ops, D, Ls):
    rng = np.random.default_rng(3)
    B = 300
    Vs = [int(v) for v in rng.integers(20, 400, size=len(Ls))]
    F, col_start, row_base, ids, table, lin_w = _rand_problem(rng, B, Ls, Vs, D)
    d_concat = rng.standard_normal((B, F * D)).astype(np.float32)
    d_fm = rng.standard_normal(B).astype(np.float32)
    # oracle: autograd through the torch restatement (fp64 to make it the reference)
    tt = torch.tensor(table, dtype=torch.float64, requires_grad=True)
    tl = torch.tensor(lin_w, dtype=torch.float64, requires_grad=True)
    concat_o, _, logit_o = T.emb_fm_forward(tt, tl, 0.0, torch.tensor(ids), col_start.tolist(), row_base.tolist())
    obj = (concat_o * torch.tensor(d_concat, dtype=torch.float64)).sum() + (logit_o * torch.tensor(d_fm, dtype=torch.float64)).sum()
    obj.backward()
    # device
    d_ids = _dev(ids)
    cs, rb = _dev(col_start), _dev(row_base)
    concat, sum_x, _ = ops.emb_pool_fwd(d_ids, F, cs, rb, _dev(table), _dev(lin_w), None)
    g_table = torch.zeros_like(_dev(table))
    g_lin = torch.zeros_like(_dev(lin_w))
    ops.emb_pool_bwd(d_ids, F, cs, rb, D, _dev(d_concat), concat, sum_x, _dev(d_fm), 1.0, g_table, g_lin)
    torch.cuda.synchronize()
    gt = tt.grad.numpy()
    np.testing.assert_allclose(g_table.cpu().numpy(), gt, rtol=1e-4, atol=1e-5 * (np.abs(gt).max() + 1))
    np.testing.assert_allclose(g_lin.cpu().numpy(), tl.grad.numpy(), rtol=1e-4, atol=1e-5)
    # fused-SGD form: dst = parameter, scale = -lr
    lr = 0.05
    p_table = _dev(table).clone()
    p_lin = _dev(lin_w).clone()
    ops.emb_pool_bwd(d_ids, F, cs, rb, D, _dev(d_concat), concat, sum_x, _dev(d_fm), -lr, p_table, p_lin)
    np.testing.assert_allclose(p_table.cpu().numpy(), table - lr * gt, rtol=1e-4, atol=1e-5 * (np.abs(gt).max() + 1))


# ---------------------------------------------------------------- K6
def test_fm2_fwd_bwd(ops):
    rng = np.random.RandomState(0)
    x = rng.normal(size=(10, 5, 5)).astype(np.float32)      # tests/keras/test_fm.py:17-26 shape
    out = ops.fm2_fwd(_dev(x)).cpu().numpy()
    np.testing.assert_allclose(out, O.fm_second_order(x), rtol=1e-6, atol=1e-6)
    x = rng.normal(size=(333, 26, 64)).astype(np.float32)
    out = ops.fm2_fwd(_dev(x)).cpu().numpy()
    want = O.fm_second_order(x)
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-5 * np.abs(want).max())
    g = rng.normal(size=(333,)).astype(np.float32)
    dx = ops.fm2_bwd(_dev(x), _dev(g)).cpu().numpy()
    want_dx = g[:, None, None] * (x.sum(1, keepdims=True) - x)
    np.testing.assert_allclose(dx, want_dx, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------- K7
@pytest.mark.parametrize("M,K,N,act", [(1, 3, 1, 0), (130, 70, 33, 1), (257, 1677, 256, 1), (512, 256, 32, 1), (100, 32, 1, 0),
                                       (300, 129, 131, 0), (64, 20, 40, 1), (33, 16, 72, 0), (200, 31, 36, 1)])
def test_linear_fwd_bwd(ops, M, K, N, act):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    y = ops.linear_fwd(_dev(x), _dev(W), _dev(b), act)
    want = O.dense(x, W, b, "relu" if act else None)
    ref64 = x.astype(np.float64) @ W.astype(np.float64) + b
    if act:
        ref64 = np.maximum(ref64, 0)
    tol = 2e-6 * np.sqrt(K) * (np.abs(ref64).max() + 1)      # fp32 round-off of a K-long fmaf chain
    np.testing.assert_allclose(y.cpu().numpy(), ref64, rtol=0, atol=tol)
    np.testing.assert_allclose(y.cpu().numpy(), want, rtol=0, atol=2 * tol)
    # backward
    dy = rng.standard_normal((M, N)).astype(np.float32)
    relu_src = rng.standard_normal((M, K)).astype(np.float32)
    dx = ops.linear_bwd_dx(_dev(dy), _dev(W), _dev(relu_src)).cpu().numpy()
    want_dx = (dy.astype(np.float64) @ W.T.astype(np.float64)) * (relu_src > 0)
    np.testing.assert_allclose(dx, want_dx, rtol=0, atol=2e-6 * np.sqrt(N) * (np.abs(want_dx).max() + 1))
    want_dW = x.T.astype(np.float64) @ dy.astype(np.float64)
    for ws in (None, ops.linear_bwd_dw_workspace(M, K, N, "cuda")):      # atomic combine / deterministic reduce
        dW = torch.zeros((K, N), device="cuda")
        db = torch.zeros(N, device="cuda")
        ops.linear_bwd_dw(_dev(x), _dev(dy), 1.0, dW, db, workspace=ws)
        np.testing.assert_allclose(dW.cpu().numpy(), want_dW, rtol=0, atol=4e-6 * np.sqrt(M) * (np.abs(want_dW).max() + 1))
        np.testing.assert_allclose(db.cpu().numpy(), dy.astype(np.float64).sum(0), rtol=0, atol=1e-5 * np.sqrt(M) * 4)


@pytest.mark.parametrize("M,K,N", [(8192, 512, 256), (16384, 256, 32), (10000, 300, 64), (5000, 512, 256)])
@pytest.mark.parametrize("mode", ["bf16x3", "native"])
def test_linear_bwd_dw_splitk_ignores_unwritten_workspace(ops, M, K, N, mode):
    """Split-K wgrad with a workspace: trailing reduction slices can be empty (M = 8192, K = 512, N = 256 -> 31 slices of 288
    rows, the last two start past M).  The reduce must not sum them: the workspace is poisoned with NaN."""
    rng = np.random.default_rng(77)
    x = rng.standard_normal((M, K)).astype(np.float32)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    want = x.T.astype(np.float64) @ dy.astype(np.float64)
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        ws = ops.linear_bwd_dw_workspace(M, K, N, "cuda")
        ws.fill_(float("nan"))
        dW = torch.zeros((K, N), device="cuda")
        db = torch.zeros(N, device="cuda")
        ops.linear_bwd_dw(_dev(x), _dev(dy), 1.0, dW, db, workspace=ws)
    finally:
        ops.set_gemm_mode(prev)
    got = dW.cpu().numpy()
    assert np.isfinite(got).all(), "an unwritten split-K slice was summed into the weights"
    np.testing.assert_allclose(got, want, rtol=0, atol=4e-6 * np.sqrt(M) * (np.abs(want).max() + 1))


@pytest.mark.parametrize("M,K,N,mask", [(32, 128, 32, True), (96, 256, 32, True), (4096, 256, 32, True),
                                          (640, 256, 17, False), (2048, 512, 32, True), (64, 128, 1, True),
                                          (32 * 700, 256, 32, True)])
def test_linear_bwd_narrow_fused(ops, M, K, N, mask):
    """Fused dx + dW + db of a narrow layer == the two-kernel path's definition (fp64 reference), in-place SGD on W."""
    rng = np.random.default_rng(31)
    x = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)        # post-ReLU activations (zeros included)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    scale = -0.01
    ldn = (N + 3) // 4 * 4
    Wd = torch.zeros((K, ldn), device="cuda")[:, :N]
    Wd.copy_(_dev(W))
    bd = _dev(b).clone()
    dyd = torch.zeros((M, ldn), device="cuda")[:, :N]
    dyd.copy_(_dev(dy))
    dx = torch.full((M, K), 7.0, device="cuda")
    ops.linear_bwd_narrow(_dev(x), dyd, Wd, scale, Wd, bd, dx, relu_mask=mask)
    want_dx = dy.astype(np.float64) @ W.T.astype(np.float64)
    if mask:
        want_dx = want_dx * (x > 0)
    np.testing.assert_allclose(dx.cpu().numpy(), want_dx, rtol=0, atol=2e-6 * np.sqrt(N) * (np.abs(want_dx).max() + 1))
    gW = x.T.astype(np.float64) @ dy.astype(np.float64)
    np.testing.assert_allclose(Wd.cpu().numpy(), W + scale * gW, rtol=0,
                               atol=abs(scale) * 4e-6 * np.sqrt(M) * (np.abs(gW).max() + 1) + 1e-7)
    gb = dy.astype(np.float64).sum(0)
    np.testing.assert_allclose(bd.cpu().numpy(), b + scale * gb, rtol=0, atol=abs(scale) * 1e-5 * np.sqrt(M) * 4 + 1e-6)
    # deterministic: a second run from the same inputs gives the same bits
    Wd2 = torch.zeros((K, ldn), device="cuda")[:, :N]
    Wd2.copy_(_dev(W))
    bd2 = _dev(b).clone()
    dx2 = torch.empty((M, K), device="cuda")
    ops.linear_bwd_narrow(_dev(x), dyd, Wd2, scale, Wd2, bd2, dx2, relu_mask=mask)
    assert torch.equal(Wd, Wd2) and torch.equal(bd, bd2) and torch.equal(dx, dx2)


def test_linear_bwd_narrow_shape_contract(ops):
    x = torch.zeros((40, 256), device="cuda")
    dy = torch.zeros((40, 32), device="cuda")
    W = torch.zeros((256, 32), device="cuda")
    assert not ops.linear_bwd_narrow_supported(40, 256, 32) and not ops.linear_bwd_narrow_supported(64, 200, 32)
    assert not ops.linear_bwd_narrow_supported(64, 256, 33) and ops.linear_bwd_narrow_supported(64, 256, 32)
    with pytest.raises(RuntimeError, match="DR_ESHAPE"):
        ops.linear_bwd_narrow(x, dy, W, -0.1, W, None, torch.empty_like(x))


@pytest.mark.parametrize("M,K,H,mode", [(128, 256, 32, 0), (1000, 256, 32, 0), (4096 + 77, 64, 32, 1), (513, 100, 17, 2),
                                         (65536, 256, 32, 0)])
def test_tower_head_fused(ops, M, K, H, mode):
    """Fused Dense(H, relu) + Dense(1) + extra logit + BCE + Dense(1) backward/SGD == the op-by-op definition."""
    rng = np.random.default_rng(41)
    x = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)
    W1 = (rng.standard_normal((K, H)) / np.sqrt(K)).astype(np.float32)
    b1 = (rng.standard_normal(H) * 0.1).astype(np.float32)
    w2 = (rng.standard_normal((H, 1)) / np.sqrt(H)).astype(np.float32)
    b2 = np.array([0.05], np.float32)
    extra = rng.standard_normal(M).astype(np.float32)
    z = (rng.random(M) < 0.3).astype(np.float32)
    scale = -0.05
    W2d = torch.zeros((H, 4), device="cuda")[:, :1]
    W2d.copy_(_dev(w2))
    b2d = _dev(b2).clone()
    xd = torch.zeros((M, (K + 3) // 4 * 4), device="cuda")[:, :K]
    xd.copy_(_dev(x))
    h_out = torch.empty((M, (H + 3) // 4 * 4), device="cuda")[:, :H]
    loss, prob, d_logit, d_h = ops.tower_head_fwd_bwd(xd, _dev(W1), _dev(b1), W2d, b2d, _dev(extra), _dev(z), mode, scale,
                                                       h_out=h_out)
    # fp64 reference through torch autograd
    tx = torch.tensor(x, dtype=torch.float64)
    tW1 = torch.tensor(W1, dtype=torch.float64)
    tw2 = torch.tensor(w2, dtype=torch.float64, requires_grad=True)
    tb2 = torch.tensor(b2, dtype=torch.float64, requires_grad=True)
    pre = (tx @ tW1 + torch.tensor(b1, dtype=torch.float64)).requires_grad_(True)
    h = torch.relu(pre)
    logit = (h @ tw2).reshape(-1) + tb2 + torch.tensor(extra, dtype=torch.float64)
    logit.retain_grad()
    tz = torch.tensor(z, dtype=torch.float64)
    if mode == 0:
        lo = T.sigmoid_cross_entropy(tz, logit)
    elif mode == 1:
        lo = T.log_loss(tz, torch.sigmoid(logit))
    else:
        lo = T.keras_bce(tz, torch.sigmoid(logit))
    lo.backward()
    np.testing.assert_allclose(h_out.cpu().numpy(), h.detach().numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(prob.cpu().numpy(), torch.sigmoid(logit).detach().numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(loss.item(), lo.item(), rtol=1e-5)                       # north_star tolerance on the loss
    np.testing.assert_allclose(d_logit.cpu().numpy() * M, logit.grad.numpy() * M, rtol=0, atol=5e-5)
    np.testing.assert_allclose(d_h.cpu().numpy() * M, pre.grad.numpy() * M, rtol=0, atol=1e-4)
    np.testing.assert_allclose(W2d.cpu().numpy(), w2 + scale * tw2.grad.numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(b2d.cpu().numpy(), b2 + scale * tb2.grad.numpy(), rtol=0, atol=2e-6)


def test_linear_bwd_narrow_in_two_halves(ops):
    """parts = 1 then parts = 2 of dr_linear_bwd_narrow: the same two launches as one call (parts = 3), so the same bits; part 1 alone
    leaves dx complete and the weights untouched.  M = 32 * 515: 512 blocks, three of them with a second chunk; N = 17: a ragged
    column tile.  dx and the weight step also against the fp64 definition, tolerances of test_linear_bwd_narrow_fused."""
    rng = np.random.default_rng(32)
    M, K, N, scale = 32 * 515, 256, 17, -0.01
    x = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    xd = _dev(x)
    dyd = torch.zeros((M, 20), device="cuda")[:, :N]
    dyd.copy_(_dev(dy))

    def fresh():
        Wd = torch.zeros((K, 20), device="cuda")[:, :N]
        Wd.copy_(_dev(W))
        return Wd, _dev(b).clone(), torch.full((M, K), 7.0, device="cuda")
    ws = ops.linear_bwd_narrow_workspace(M, K, N, "cuda")
    W3, b3, dx3 = fresh()
    ops.linear_bwd_narrow(xd, dyd, W3, scale, W3, b3, dx3, workspace=ws)
    ws.fill_(float("nan"))
    W12, b12, dx12 = fresh()
    ops.linear_bwd_narrow(xd, dyd, W12, scale, W12, b12, dx12, workspace=ws, parts=1)
    assert torch.equal(dx12, dx3) and torch.equal(W12, _dev(W)) and torch.equal(b12, _dev(b))
    ops.linear_bwd_narrow(xd, dyd, W12, scale, W12, b12, dx12, workspace=ws, parts=2)
    assert torch.equal(W12, W3) and torch.equal(b12, b3) and torch.equal(dx12, dx3)
    want_dx = (dy.astype(np.float64) @ W.T.astype(np.float64)) * (x > 0)
    np.testing.assert_allclose(dx3.cpu().numpy(), want_dx, rtol=0, atol=2e-6 * np.sqrt(N) * (np.abs(want_dx).max() + 1))
    gW = x.T.astype(np.float64) @ dy.astype(np.float64)
    np.testing.assert_allclose(W3.cpu().numpy(), W + scale * gW, rtol=0, atol=abs(scale) * 4e-6 * np.sqrt(M) * (np.abs(gW).max() + 1) + 1e-7)
    with pytest.raises(RuntimeError, match="DR_EINVAL"):
        ops.linear_bwd_narrow(xd, dyd, W12, scale, W12, b12, dx12, workspace=ws, parts=4)


def test_tower_head_in_two_halves(ops):
    """parts = 1 then parts = 2 of dr_tower_head_fwd_bwd against one call (parts = 3, checked against torch at this shape by
    test_tower_head_fused): the same two launches, so the same bits; part 1 alone leaves prob, d_logit and d_h complete and w2, b2 and the
    loss untouched.  M = 513: full row tiles and a ragged one; H = 17, K = 100: ragged in both."""
    rng = np.random.default_rng(41)
    M, K, H, mode, scale = 513, 100, 17, 2, -0.05
    xd = torch.zeros((M, K), device="cuda")
    xd.copy_(_dev(np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)))
    W1 = _dev((rng.standard_normal((K, H)) / np.sqrt(K)).astype(np.float32))
    b1 = _dev((rng.standard_normal(H) * 0.1).astype(np.float32))
    w2 = _dev((rng.standard_normal((H, 1)) / np.sqrt(H)).astype(np.float32))
    b2 = _dev(np.array([0.05], np.float32))
    extra, z = _dev(rng.standard_normal(M).astype(np.float32)), _dev((rng.random(M) < 0.3).astype(np.float32))

    def run(parts_seq):
        w2d = torch.zeros((H, 4), device="cuda")[:, :1]
        w2d.copy_(w2)
        o = dict(w2=w2d, b2=b2.clone(), loss=torch.full((1,), 7.0, device="cuda"), prob=torch.full((M,), 7.0, device="cuda"),
                 d_logit=torch.full((M,), 7.0, device="cuda"), d_h=torch.full((M, 20), 7.0, device="cuda")[:, :H],
                 ws=ops.tower_head_workspace(M, "cuda"))
        o["ws"].fill_(float("nan"))
        snaps = []
        for parts in parts_seq:
            ops.tower_head_fwd_bwd(xd, W1, b1, o["w2"], o["b2"], extra, z, mode, scale, prob=o["prob"], d_logit=o["d_logit"], d_h=o["d_h"],
                                   loss=o["loss"], workspace=o["ws"], parts=parts)
            snaps.append({k: o[k].clone() for k in ("w2", "b2", "loss", "prob", "d_logit", "d_h")})
        return snaps
    whole, = run([3])
    first, second = run([1, 2])
    for k in ("prob", "d_logit", "d_h"):
        assert torch.equal(first[k], whole[k]) and torch.equal(second[k], whole[k]), k
    assert torch.equal(first["w2"], w2) and torch.equal(first["b2"], b2) and first["loss"].item() == 7.0
    for k in ("w2", "b2", "loss"):
        assert torch.equal(second[k], whole[k]), k
    assert not torch.equal(whole["w2"], w2) and whole["loss"].item() != 7.0
    with pytest.raises(RuntimeError, match="DR_EINVAL"):
        run([0])


@pytest.mark.parametrize("M,K,H,mode", [(128, 256, 32, 0), (4096, 128, 32, 1), (2048 + 32, 256, 17, 2), (65536, 256, 32, 0)])
def test_tower_tail_fused_one_pass(ops, M, K, H, mode):
    """dr_tower_tail_fused == dr_tower_head_fwd_bwd (relu) followed by dr_linear_bwd_narrow (relu mask) of the same layer, and both
    == the op-by-op definition in fp64 (torch autograd): prob, loss, d_logit, d_h, dx and the four fused SGD updates.  Deterministic;
    the amax record of dx is exact."""
    rng = np.random.default_rng(43)
    x = np.maximum(rng.standard_normal((M, K)), 0).astype(np.float32)        # post-ReLU activations (zeros included)
    W1 = (rng.standard_normal((K, H)) / np.sqrt(K)).astype(np.float32)
    b1 = (rng.standard_normal(H) * 0.1).astype(np.float32)
    w2 = (rng.standard_normal((H, 1)) / np.sqrt(H)).astype(np.float32)
    b2 = np.array([0.05], np.float32)
    extra = rng.standard_normal(M).astype(np.float32)
    z = (rng.random(M) < 0.3).astype(np.float32)
    scale = -0.05
    ldh = (H + 3) // 4 * 4

    def params():
        W1d = torch.zeros((K, ldh), device="cuda")[:, :H]
        W1d.copy_(_dev(W1))
        W2d = torch.zeros((H, 4), device="cuda")[:, :1]
        W2d.copy_(_dev(w2))
        return W1d, _dev(b1).clone(), W2d, _dev(b2).clone()
    xd = _dev(x)
    # ---- the one-pass kernel
    W1d, b1d, W2d, b2d = params()
    dx = torch.full((M, K), 7.0, device="cuda")
    d_h = torch.full((M, ldh), 7.0, device="cuda")[:, :H]
    rec = ops.h2_record("cuda")
    rec.fill_(0x7f000000)
    loss, prob, d_logit, _ = ops.tower_tail_fused(xd, W1d, b1d, W2d, b2d, _dev(extra), _dev(z), mode, scale, dx, d_h=d_h, dx_amax=rec)
    # ---- the two launches it replaces
    W1e, b1e, W2e, b2e = params()
    dx_e = torch.empty((M, K), device="cuda")
    loss_e, prob_e, d_logit_e, d_h_e = ops.tower_head_fwd_bwd(xd, W1e, b1e, W2e, b2e, _dev(extra), _dev(z), mode, scale)
    ops.linear_bwd_narrow(xd, d_h_e, W1e, scale, W1e, b1e, dx_e, relu_mask=True)
    # ---- fp64 definition
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tW1 = torch.tensor(W1, dtype=torch.float64, requires_grad=True)
    tb1 = torch.tensor(b1, dtype=torch.float64, requires_grad=True)
    tw2 = torch.tensor(w2, dtype=torch.float64, requires_grad=True)
    tb2 = torch.tensor(b2, dtype=torch.float64, requires_grad=True)
    pre = tx @ tW1 + tb1
    pre.retain_grad()
    h = torch.relu(pre)
    logit = (h @ tw2).reshape(-1) + tb2 + torch.tensor(extra, dtype=torch.float64)
    logit.retain_grad()
    tz = torch.tensor(z, dtype=torch.float64)
    lo = T.sigmoid_cross_entropy(tz, logit) if mode == 0 else (T.log_loss(tz, torch.sigmoid(logit)) if mode == 1 else T.keras_bce(tz, torch.sigmoid(logit)))
    lo.backward()
    want_dx = tx.grad.numpy() * (x > 0)                                       # the mask of the layer BELOW (x is post-ReLU)
    np.testing.assert_allclose(prob.cpu().numpy(), torch.sigmoid(logit).detach().numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(loss.item(), lo.item(), rtol=1e-5)
    np.testing.assert_allclose(d_logit.cpu().numpy() * M, logit.grad.numpy() * M, rtol=0, atol=5e-5)
    np.testing.assert_allclose(d_h.cpu().numpy() * M, pre.grad.numpy() * M, rtol=0, atol=1e-4)
    np.testing.assert_allclose(dx.cpu().numpy() * M, want_dx * M, rtol=0, atol=2e-4)
    for got, p0, gr, nm in ((W1d, W1, tW1.grad, "W1"), (b1d, b1, tb1.grad, "b1"), (W2d, w2, tw2.grad, "w2"), (b2d, b2, tb2.grad, "b2")):
        np.testing.assert_allclose(got.cpu().numpy(), p0 + scale * gr.numpy(), rtol=0, atol=3e-6, err_msg=nm)
    # ---- against the two-launch path: same arithmetic up to the order of the K-long sums
    np.testing.assert_allclose(prob.cpu().numpy(), prob_e.cpu().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(loss.item(), loss_e.item(), rtol=2e-6)
    np.testing.assert_allclose(dx.cpu().numpy() * M, dx_e.cpu().numpy() * M, rtol=0, atol=1e-4)
    np.testing.assert_allclose(W1d.cpu().numpy(), W1e.cpu().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(W2d.cpu().numpy(), W2e.cpu().numpy(), rtol=0, atol=1e-6)
    assert int(rec.item()) == int(dx.abs().max().view(torch.int32).item()), "amax record of dx"
    assert float(d_h[:, :H].abs().max()) < 7.0 and float(dx.abs().max()) < 7.0     # every element written
    # ---- deterministic
    W1f, b1f, W2f, b2f = params()
    dx2 = torch.empty((M, K), device="cuda")
    loss2, prob2, d_logit2, _ = ops.tower_tail_fused(xd, W1f, b1f, W2f, b2f, _dev(extra), _dev(z), mode, scale, dx2)
    assert torch.equal(dx, dx2) and torch.equal(W1d, W1f) and torch.equal(W2d, W2f) and torch.equal(b1d, b1f) and torch.equal(b2d, b2f)
    assert torch.equal(loss, loss2) and torch.equal(prob, prob2)
    # ---- shape contract
    assert ops.tower_tail_supported(64, 256, 32) and not ops.tower_tail_supported(64, 512, 32) and not ops.tower_tail_supported(40, 256, 32)
    with pytest.raises(RuntimeError, match="DR_ESHAPE"):
        ops.tower_tail_fused(torch.zeros((64, 512), device="cuda"), torch.zeros((512, 32), device="cuda"), None, torch.zeros((32, 1), device="cuda"),
                             None, None, torch.zeros(64, device="cuda"), 0, -0.1, torch.zeros((64, 512), device="cuda"))


@pytest.mark.parametrize("M,K,N", [(8192, 8192, 128), (300, 5000, 40), (2048, 2049, 130)])
def test_linear_fwd_splitk_matches_fp64_and_is_deterministic(ops, M, K, N):
    """dr_linear_fwd_splitk (the two-tower dq = G c: few output tiles, long reduction split over the grid): accumulates into y,
    agrees with float64 as well as dr_linear_fwd does, and two runs are bit-identical (fixed-order reduce, no atomics)."""
    g = torch.Generator(device="cuda").manual_seed(M + N)
    x = torch.randn((M, K), device="cuda", generator=g) * 0.05
    W = torch.randn((K, N), device="cuda", generator=g)
    base = torch.randn((M, N), device="cuda", generator=g)
    y1, y2 = base.clone(), base.clone()
    ops.linear_fwd_splitk(x, W, y1)
    ops.linear_fwd_splitk(x, W, y2)
    assert torch.equal(y1, y2)
    ref = base.double() + x.double() @ W.double()
    e_new = ((y1.double() - ref).abs().max() / ref.abs().max()).item()
    e_old = (((base + ops.linear_fwd(x, W, None, 0)).double() - ref).abs().max() / ref.abs().max()).item()
    assert e_new <= 2e-6 and e_new <= 2.0 * e_old + 1e-7, (e_new, e_old)


def test_linear_transpose_detecting(ops):
    # A = I with an ASYMMETRIC B catches a swapped C/D fragment layout
    K = N = 64
    x = np.eye(K, dtype=np.float32)
    W = np.arange(K * N, dtype=np.float32).reshape(K, N)
    y = ops.linear_fwd(_dev(x), _dev(W), None, 0).cpu().numpy()
    np.testing.assert_array_equal(y, W)


# ---------------------------------------------------------------- K8
def test_cross_known_answer_and_random(ops):
    x0 = np.array([[0.1, 0.2, 0.3]], np.float32)
    x = np.array([[0.4, 0.5, 0.6]], np.float32)
    out, _ = ops.cross_fwd(_dev(x0), _dev(x), _dev(np.ones((3, 3), np.float32)), _dev(np.zeros(3, np.float32)))
    np.testing.assert_allclose(out.cpu().numpy(), [[0.55, 0.8, 1.05]], rtol=1e-6, atol=1e-6)   # tests/keras/test_dcn.py:16-23
    rng = np.random.default_rng(9)
    M, Dm = 200, 77
    x0 = rng.standard_normal((M, Dm)).astype(np.float32)
    x = rng.standard_normal((M, Dm)).astype(np.float32)
    W = (rng.standard_normal((Dm, Dm)) * 0.05).astype(np.float32)
    b = rng.standard_normal(Dm).astype(np.float32)
    out, prod = ops.cross_fwd(_dev(x0), _dev(x), _dev(W), _dev(b), 0.3, want_prod=True)
    want = O.cross(x0, x, W, b, 0.3)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(prod.cpu().numpy(), x @ W + b + 0.3 * x, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------- K11
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bce_modes(ops, mode):
    rng = np.random.default_rng(11)
    n = 70001
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    x[:4] = [30.0, -30.0, 90.0, -90.0]
    z = (rng.random(n) < 0.25).astype(np.float32)
    loss, prob, g = ops.bce_fwd_bwd(_dev(x), _dev(z), mode)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tz = torch.tensor(z, dtype=torch.float64)
    if mode == 0:
        want = O.sigmoid_cross_entropy(z, x)
        lo = T.sigmoid_cross_entropy(tz, tx)
    elif mode == 1:
        want = O.log_loss(z, O.sigmoid(x))
        lo = T.log_loss(tz, torch.sigmoid(tx.float()).double())
    else:
        want = O.keras_binary_crossentropy(z, O.sigmoid(x))
        lo = T.keras_bce(tz, torch.sigmoid(tx.float()).double())
    assert abs(loss.item() - float(want)) <= 1e-5 * abs(float(want))        # north_star: 1e-5 relative on the loss
    np.testing.assert_allclose(prob.cpu().numpy(), O.sigmoid(x), rtol=1e-6, atol=1e-7)
    if mode == 0:
        lo.backward()
        np.testing.assert_allclose(g.cpu().numpy(), tx.grad.numpy(), rtol=1e-4, atol=1e-9)


# ---------------------------------------------------------------- sharding prims
@pytest.mark.parametrize("world", [1, 2, 8])
def test_shard_bucket_ids_bit_exact(ops, world):
    rng = np.random.default_rng(13)
    B, C, V = 4099, 26, 10_000_000
    ids = rng.integers(0, V, size=(B, C))
    ids[rng.random((B, C)) < 0.01] = -1
    rps = (V + world - 1) // world
    counts, send_rows, pos = ops.shard_bucket_ids(_dev(ids), rps, world)
    flat = ids.reshape(-1)
    p = np.arange(flat.size)
    owner = np.where(flat >= 0, flat % world, p % world)
    local = np.where(flat >= 0, (p % C) * rps + flat // world, -1)
    order = np.argsort(owner, kind="stable")
    want_pos = np.empty_like(order)
    want_pos[order] = np.arange(order.size)
    np.testing.assert_array_equal(counts.cpu().numpy(), np.bincount(owner, minlength=world))
    np.testing.assert_array_equal(send_rows.cpu().numpy(), local[order])       # stable: identical layout
    np.testing.assert_array_equal(pos.cpu().numpy().reshape(-1), want_pos)


@pytest.mark.parametrize("V,path", [(50_000, "claim"), (300, "radix")])
def test_shard_dedup_bucketing_and_pack(ops, V, path):
    """Requester-side de-duplication (dr_shard_dedup_slots / dr_shard_bucket_ids with rep / dr_emb_pack_grads with unique_flags): the lowest slot of
    every row is its representative (bit-exact against NumPy), only representatives get a send slot, every slot's position points at
    its row's place, and the pack sums the gradients of the slots that share a row.  V = 300: nearly every slot shares its row (the
    plan's radix path, every slot in the sorted arrays); V = 50 000: mostly unique rows (the claim path: only the shared-row slots)."""
    rng = np.random.default_rng(21)
    B, F, D, world = 2048, 6, 64, 4
    ids = rng.integers(0, V, size=(B, F))
    ids[rng.random((B, F)) < 0.01] = -1
    base = np.arange(F, dtype=np.int64) * V
    ids_d, base_d = _dev(ids), _dev(base)
    plan = ops.emb_sort_slots(ids_d, base_d, F * V)
    rep, flags = ops.shard_dedup_slots(ids_d, base_d, F * V, plan)
    flat = ids.reshape(-1)
    rows = np.where(flat >= 0, flat + np.tile(base, B), -1 - np.arange(flat.size))
    uniq, first, cnt = np.unique(rows, return_index=True, return_counts=True)
    idx = np.searchsorted(uniq, rows)
    np.testing.assert_array_equal(rep.cpu().numpy(), first[idx])
    want_flags = np.where(flat >= 0, cnt[idx] == 1, flags.cpu().numpy()[:flat.size] != 0)      # (a missing id's flag is not consumed)
    np.testing.assert_array_equal(flags.cpu().numpy()[:flat.size][flat >= 0] != 0, want_flags[flat >= 0])
    rps = (V + world - 1) // world
    counts, send_rows, pos = ops.shard_bucket_ids(ids_d, rps, world, rep=rep)
    p = np.arange(flat.size)
    is_rep = first[idx] == p
    owner = np.where(flat >= 0, flat % world, p % world)
    local = np.where(flat >= 0, (p % F) * rps + flat // world, -1)
    keep = p[is_rep]
    order = keep[np.argsort(owner[keep], kind="stable")]
    want_pos = np.full(flat.size, -1, dtype=np.int64)
    want_pos[order] = np.arange(order.size)
    want_pos = want_pos[first[idx]]
    np.testing.assert_array_equal(counts.cpu().numpy(), np.bincount(owner[keep], minlength=world))
    n_send = order.size
    np.testing.assert_array_equal(send_rows.cpu().numpy()[:n_send], local[order])
    np.testing.assert_array_equal(pos.cpu().numpy().reshape(-1), want_pos)
    assert n_send < flat.size
    # pack: shared rows accumulate
    ld = F * D + 4
    d_concat = rng.standard_normal((B, ld)).astype(np.float32)
    concat = rng.standard_normal((B, ld)).astype(np.float32)
    sum_x = rng.standard_normal((B, D)).astype(np.float32)
    dl = rng.standard_normal(B).astype(np.float32)
    out = torch.zeros((n_send, D), device="cuda")
    out_lin = torch.zeros(n_send, device="cuda")
    bias = torch.zeros(1, device="cuda")
    ops.emb_pack_grads(pos, D, _dev(d_concat), _dev(concat), _dev(sum_x), _dev(dl), out, out_lin, bias, unique_flags=flags)
    want = np.zeros((n_send, D))
    want_lin = np.zeros(n_send)
    for f in range(F):
        g = d_concat[:, f * D:(f + 1) * D].astype(np.float64) + dl[:, None].astype(np.float64) * (sum_x.astype(np.float64) - concat[:, f * D:(f + 1) * D])
        np.add.at(want, want_pos.reshape(B, F)[:, f], g)
        np.add.at(want_lin, want_pos.reshape(B, F)[:, f], dl.astype(np.float64))
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(out_lin.cpu().numpy(), want_lin, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(float(bias[0]), float(dl.astype(np.float64).sum()), rtol=1e-5, atol=1e-4)
    if path == "claim":
        assert plan.sorted_len() < B * F                   # only the shared-row slots were sorted


def test_rows_gather_scatter_axpy(ops):
    rng = np.random.default_rng(14)
    R, D, n = 1000, 64, 5003
    table = rng.standard_normal((R, D)).astype(np.float32)
    lin = rng.standard_normal(R).astype(np.float32)
    rows = rng.integers(0, R, size=n)
    rows[::11] = -1
    out, out_lin = ops.rows_gather(_dev(rows), _dev(table), _dev(lin))
    want = np.where(rows[:, None] >= 0, table[np.maximum(rows, 0)], 0)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    np.testing.assert_array_equal(out_lin.cpu().numpy(), np.where(rows >= 0, lin[np.maximum(rows, 0)], 0))
    grads = rng.standard_normal((n, D)).astype(np.float32)
    lg = rng.standard_normal(n).astype(np.float32)
    t_dev, l_dev = _dev(table).clone(), _dev(lin).clone()
    ops.rows_scatter_add(_dev(rows), _dev(grads), _dev(lg), -0.5, t_dev, l_dev)
    want_t = table.astype(np.float64).copy()
    want_l = lin.astype(np.float64).copy()
    m = rows >= 0
    np.add.at(want_t, rows[m], -0.5 * grads[m])
    np.add.at(want_l, rows[m], -0.5 * lg[m])
    np.testing.assert_allclose(t_dev.cpu().numpy(), want_t, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(l_dev.cpu().numpy(), want_l, rtol=1e-5, atol=1e-5)
    x = _dev(rng.standard_normal(10001).astype(np.float32))
    y = _dev(rng.standard_normal(10001).astype(np.float32))
    want = y.cpu().numpy() + np.float32(-0.25) * x.cpu().numpy()
    ops.axpy(-0.25, x, y)
    np.testing.assert_allclose(y.cpu().numpy(), want, rtol=1e-6, atol=1e-7)


# ---------------------------------------------------------------- K4 deterministic (sorted) form
def check_slot_plan(plan, keys, R, expect_path=None):
    """Invariants of dr_emb_sort_slots' output against the key list `keys` [n] (row per slot, R = missing):
    flags == "my row is touched by exactly one slot"; the sorted arrays hold either exactly the slots of shared rows (claim path)
    or all slots with the missing ones last (radix path), ascending by row and by slot inside a row; the work list holds every
    segment start of a shared row plus the 32-aligned cut points of rows hit more than 32 times."""
    n = keys.size
    cnt = np.bincount(keys, minlength=R + 1)
    want_flags = ((cnt[keys] == 1) & (keys < R)).astype(np.uint8)
    np.testing.assert_array_equal(plan.flags.cpu().numpy()[:n], want_flags)
    L = plan.sorted_len()
    shared = np.nonzero((cnt[keys] > 1) & (keys < R))[0]
    path = "radix" if L == n else "claim"
    if expect_path is not None and shared.size > 0:
        assert path == expect_path or (L == n == shared.size), (path, expect_path, L, n, shared.size)
    sr, ss = plan.rows.cpu().numpy()[:L], plan.slots.cpu().numpy()[:L]
    if L == n:      # radix path (or every slot shared): a full stable sort by row
        order = np.argsort(keys, kind="stable")
    else:           # claim path: only the shared-row slots, by (row, slot)
        assert L == shared.size
        order = shared[np.argsort(keys[shared], kind="stable")]
    np.testing.assert_array_equal(ss, order.astype(np.int32))
    np.testing.assert_array_equal(sr, keys[order])
    nh = int(plan.dup_count[0].item())
    heads = np.sort(plan.dup_heads.cpu().numpy()[:nh])
    i = np.arange(L)
    valid = sr < R
    seg_start = np.ones(L, dtype=bool)
    seg_start[1:] = sr[1:] != sr[:-1]
    has_next = np.zeros(L, dtype=bool)
    has_next[:-1] = sr[1:] == sr[:-1]
    back = np.zeros(L, dtype=bool)
    back[32:] = sr[32:] == sr[:-32]
    want_heads = np.nonzero(valid & ((seg_start & has_next) | (~seg_start & (i % 32 == 0) & (i >= 32) & back)))[0]
    np.testing.assert_array_equal(heads, want_heads)
    return path


@pytest.mark.parametrize("path", ["claim", "radix"])
@pytest.mark.parametrize("D,F,V,hot", [(64, 26, 5000, False), (16, 7, 50, True), (128, 3, 7, True), (12, 5, 1000, False)])
def test_emb_bwd_sorted_matches_oracle_and_is_deterministic(ops, D, F, V, hot, path):
    """path: the plan's claim table + one-block LDS sort of the shared-row slots (default for short lists), or -- forced through
    dr_emb_plan_set_small_limit(0) -- the radix sort of all slots that skewed batches take."""
    prev = ops.emb_plan_set_small_limit(0 if path == "radix" else 16384)
    try:
        _emb_bwd_sorted_case(ops, D, F, V, hot, path)
    finally:
        ops.emb_plan_set_small_limit(prev)


def _emb_bwd_sorted_case(ops, D, F, V, hot, path):
    rng = np.random.default_rng(21)
    B = 1500
    ids = rng.integers(0, V, size=(B, F))
    if hot:
        ids[:, 0] = 3                                   # one row hit by every example: > 32-slot chunks + atomics
    ids[rng.random((B, F)) < 0.05] = -1
    row_base = (np.arange(F) * V).astype(np.int64)
    R = F * V
    grad = rng.standard_normal((B, F * D)).astype(np.float32)
    dl = rng.standard_normal(B).astype(np.float32)
    table = rng.standard_normal((R, D)).astype(np.float32)
    lin = rng.standard_normal(R).astype(np.float32)
    d_ids, d_rb = _dev(ids), _dev(row_base)
    plan = ops.emb_sort_slots(d_ids, d_rb, R)
    keys = np.where(ids.reshape(-1) >= 0, (ids + row_base[None, :]).reshape(-1), R)
    # (hot batches overflow a partition's bucket of the claim path: the device then takes the radix path by itself)
    check_slot_plan(plan, keys, R, expect_path=path if (path == "radix" or not hot) else None)
    plan2 = ops.emb_sort_slots(d_ids, d_rb, R)          # the plan itself is bit-reproducible (no arrival-order dependence)
    L = plan.sorted_len()
    assert plan2.sorted_len() == L and torch.equal(plan.rows[:L], plan2.rows[:L]) and torch.equal(plan.slots[:L], plan2.slots[:L])
    assert torch.equal(plan.flags, plan2.flags)
    outs = []
    for _ in range(2):
        t_dev, l_dev, b_dev = _dev(table).clone(), _dev(lin).clone(), torch.zeros(1, device="cuda")
        ops.emb_pool_bwd_sorted(d_ids, d_rb, plan, D, R, _dev(grad), _dev(dl), -0.1, t_dev, l_dev, b_dev)
        outs.append((t_dev.cpu().numpy(), l_dev.cpu().numpy(), b_dev.item()))
    want_t = table.astype(np.float64).copy()
    want_l = lin.astype(np.float64).copy()
    for f in range(F):
        m = ids[:, f] >= 0
        np.add.at(want_t, ids[m, f] + row_base[f], -0.1 * grad[m, f * D:(f + 1) * D])
        np.add.at(want_l, ids[m, f] + row_base[f], -0.1 * dl[m])
    tol = 1e-5 * (B if hot else 8)
    np.testing.assert_allclose(outs[0][0], want_t, rtol=1e-5, atol=tol)
    np.testing.assert_allclose(outs[0][1], want_l, rtol=1e-5, atol=tol)
    assert abs(outs[0][2] - (-0.1 * dl.astype(np.float64).sum())) < 1e-3
    if not hot:     # no row is hit by more than 32 slots -> plain RMW everywhere -> bit-reproducible
        np.testing.assert_array_equal(outs[0][0], outs[1][0])
        np.testing.assert_array_equal(outs[0][1], outs[1][1])
    # K4 without the unique rows' first-order weights (parts | 4) + dr_emb_lin_update_unique == K4: same bits on the first-order
    # weights of unique rows (one fma each, either way), tables untouched by the split
    t_dev, l_dev, b_dev = _dev(table).clone(), _dev(lin).clone(), torch.zeros(1, device="cuda")
    ops.emb_pool_bwd_sorted(d_ids, d_rb, plan, D, R, _dev(grad), _dev(dl), -0.1, t_dev, l_dev, b_dev, parts=3 | 4)
    ops.emb_lin_update_unique(d_ids, d_rb, plan, _dev(dl), -0.1, l_dev)
    if hot:     # (no x_sorted here: a hot row's pieces meet through atomics, run-to-run rounding)
        np.testing.assert_allclose(t_dev.cpu().numpy(), want_t, rtol=1e-5, atol=tol)
    else:
        np.testing.assert_array_equal(t_dev.cpu().numpy(), outs[1][0])
    uniq_rows = (ids + row_base[None, :]).reshape(-1)[plan.flags.cpu().numpy().astype(bool) & (ids.reshape(-1) >= 0)]
    np.testing.assert_array_equal(l_dev.cpu().numpy()[uniq_rows], outs[1][1][uniq_rows])
    np.testing.assert_allclose(l_dev.cpu().numpy(), want_l, rtol=1e-5, atol=tol)
    # with the x_sorted buffer the pieces of a hot row park their sums and are added in sorted order: bit-reproducible ALWAYS
    # (the buffer's content is don't-care here -- no FM term -- so it starts as NaN: nothing unwritten may be read)
    outs = []
    for _ in range(2):
        t_dev, l_dev, b_dev = _dev(table).clone(), _dev(lin).clone(), torch.zeros(1, device="cuda")
        xs = torch.full((B * F, D), float("nan"), device="cuda")
        ops.emb_pool_bwd_sorted(d_ids, d_rb, plan, D, R, _dev(grad), _dev(dl), -0.1, t_dev, l_dev, b_dev, x_sorted=xs)
        outs.append((t_dev.cpu().numpy(), l_dev.cpu().numpy(), b_dev.item()))
    np.testing.assert_allclose(outs[0][0], want_t, rtol=1e-5, atol=tol)
    np.testing.assert_allclose(outs[0][1], want_l, rtol=1e-5, atol=tol)
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("case", ["one_partition_two_passes", "one_partition_one_pass", "one_row", "spread", "three_passes"])
def test_slot_plan_large_path_sorts_any_partition(ops, case):
    """The LARGE path in one launch (plan_large_kernel, round 6): block b sorts partition b with as many 8-bit passes as its rows
    differ in.  Cases: a partition of 50 000 keys (49 steps of 1024) whose rows differ in 12 bits (two passes: ends where it
    started), in 8 bits (one pass: starts with a copy), not at all (no pass); keys spread over all partitions; 20-bit differences."""
    rng = np.random.default_rng(5)
    if case == "one_partition_two_passes":
        B, F, V = 50000, 2, 1_000_000
        ids = np.stack([rng.integers(0, 3000, B), rng.integers(0, V, B)], 1)
    elif case == "one_partition_one_pass":
        B, F, V = 50000, 2, 1_000_000
        ids = np.stack([rng.integers(0, 200, B), rng.integers(0, 200, B)], 1)
    elif case == "one_row":
        B, F, V = 3000, 1, 100_000
        ids = np.full((B, F), 777)
    elif case == "spread":
        B, F, V = 20000, 5, 300
        ids = rng.integers(0, V, (B, F))
    else:
        B, F, V = 30000, 1, 200_000_000                 # one field of 2e8 rows: a partition spans 781 K rows = 20 bits
        ids = rng.integers(0, 4000, (B, F)) * 50_000 + rng.integers(0, 3, (B, F))
    ids[rng.random((B, F)) < 0.03] = -1
    row_base = (np.arange(F) * V).astype(np.int64)
    R = F * V
    keys = np.where(ids.reshape(-1) >= 0, (ids + row_base[None, :]).reshape(-1), R)
    prev = ops.emb_plan_set_small_limit(0)
    try:
        plan = ops.emb_sort_slots(_dev(ids), _dev(row_base), R)
        plan2 = ops.emb_sort_slots(_dev(ids), _dev(row_base), R)
    finally:
        ops.emb_plan_set_small_limit(prev)
    n = B * F
    assert plan.sorted_len() == n
    order = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(plan.slots.cpu().numpy()[:n], order.astype(np.int32))
    np.testing.assert_array_equal(plan.rows.cpu().numpy()[:n], keys[order])
    assert torch.equal(plan.rows[:n], plan2.rows[:n]) and torch.equal(plan.slots[:n], plan2.slots[:n]) and torch.equal(plan.flags, plan2.flags)
    sr = keys[order]
    uniq, cnt = np.unique(keys, return_counts=True)
    c_of = cnt[np.searchsorted(uniq, keys)]
    np.testing.assert_array_equal(plan.flags.cpu().numpy()[:n], ((c_of == 1) & (keys < R)).astype(np.uint8))
    i = np.arange(n)
    seg_start = np.ones(n, dtype=bool); seg_start[1:] = sr[1:] != sr[:-1]
    has_next = np.zeros(n, dtype=bool); has_next[:-1] = sr[1:] == sr[:-1]
    back = np.zeros(n, dtype=bool); back[32:] = sr[32:] == sr[:-32]
    want_heads = np.nonzero((sr < R) & ((seg_start & has_next) | (~seg_start & (i % 32 == 0) & (i >= 32) & back)))[0]
    nh = int(plan.dup_count[0].item())
    np.testing.assert_array_equal(np.sort(plan.dup_heads.cpu().numpy()[:nh]), want_heads)


@pytest.mark.parametrize("B,F,V,trans", [(65536, 26, 10_000_000, True), (1000, 7, 5000, True), (77, 1, 50, False), (4096, 64, 3000, True),
                                          (300, 65, 100, True), (130, 3, 1 << 40, True)])
def test_hash_sort_slots_equals_the_three_calls(ops, B, F, V, trans):
    """dr_hash_sort_slots (round 6: K1 + field-major ids + composite keys + partition histogram in ONE kernel, then the plan) against
    dr_hash_bucket_i64 -> dr_ids_transpose_i32 -> dr_emb_sort_slots: ids, ids_t and every plan array bit for bit.  Shapes: the bench's;
    ragged example groups; one field; the widest fused geometry (F = 64); F = 65 and 2^40 rows (the entry point falls back to the three
    calls: no fused front / no composite key).  Keys include negatives, -1 (dropped) and a pass-through column."""
    g = torch.Generator(device="cuda").manual_seed(B + F)
    keys = torch.randint(-(10**6), 10**15, (B, F), device="cuda", generator=g)
    keys[torch.rand((B, F), device="cuda", generator=g) < 0.05] = -1
    buckets = torch.full((F,), V, dtype=torch.int64, device="cuda")
    if F > 2:
        buckets[2] = 0                                        # pass-through column: the key is the id
        keys[:, 2] = torch.randint(0, min(V, 10**6), (B,), device="cuda", generator=g)
    row_base = (torch.arange(F, dtype=torch.int64, device="cuda") * V)
    R = F * V
    ids0 = ops.hash_bucket_i64(keys, buckets)
    idt0 = ops.ids_transpose_i32(ids0) if trans else None
    plan0 = ops.emb_sort_slots(ids0, row_base, R)
    ids1 = torch.full_like(ids0, -7)
    idt1 = torch.full((F, B), -7, dtype=torch.int32, device="cuda") if trans else None
    plan1 = ops.hash_sort_slots(keys, buckets, row_base, R, ids1, idt1)
    torch.cuda.synchronize()
    assert torch.equal(ids1, ids0)
    if trans:
        assert torch.equal(idt1, idt0)
    L = plan0.sorted_len()
    assert plan1.sorted_len() == L
    assert torch.equal(plan1.flags, plan0.flags)
    assert torch.equal(plan1.rows[:L], plan0.rows[:L]) and torch.equal(plan1.slots[:L], plan0.slots[:L])
    nh = int(plan0.dup_count[0].item())
    assert int(plan1.dup_count[0].item()) == nh
    assert torch.equal(torch.sort(plan1.dup_heads[:nh]).values, torch.sort(plan0.dup_heads[:nh]).values)


def test_slot_plan_geometry_beyond_the_composite_key(ops):
    """num_rows >= 2^31 - 1 cannot go through the 31-bit claim tables / the composite key: the host sends such a call to the
    chip-wide radix sort of all slots (the only path that still takes more than one launch per phase)."""
    rng = np.random.default_rng(6)
    B, F = 6000, 1
    R = (1 << 31) + 1000
    ids = R - 1 - rng.integers(0, 3000, (B, F)) * 7
    ids[rng.random((B, F)) < 0.05] = -1
    row_base = np.zeros(F, dtype=np.int64)
    keys = np.where(ids.reshape(-1) >= 0, ids.reshape(-1), R)
    plan = ops.emb_sort_slots(_dev(ids), _dev(row_base), R)
    n = B * F
    assert plan.sorted_len() == n
    order = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(plan.slots.cpu().numpy()[:n], order.astype(np.int32))
    np.testing.assert_array_equal(plan.rows.cpu().numpy()[:n], keys[order])
    uniq, cnt = np.unique(keys, return_counts=True)
    c_of = cnt[np.searchsorted(uniq, keys)]
    np.testing.assert_array_equal(plan.flags.cpu().numpy()[:n], ((c_of == 1) & (keys < R)).astype(np.uint8))


@pytest.mark.parametrize("D,F,V,hot", [(64, 26, 5000, False), (16, 7, 50, True), (12, 5, 1000, False)])
def test_emb_bwd_sorted_adam_matches_oracle_over_steps(ops, D, F, V, hot):
    """Fused row-wise Adam K4 over 3 steps == oracle (pre-summed duplicate gradients, [TF] B15 update on touched rows);
    first-order table and FM term included; hot rows (one row hit by every example) summed by one owner."""
    rng = np.random.default_rng(33)
    B, R = 900, F * V
    lr, b1, b2, eps = 0.01, 0.9, 0.999, 1e-8
    row_base = (np.arange(F) * V).astype(np.int64)
    table = (rng.standard_normal((R, D)) * 0.3).astype(np.float32)
    lin = (rng.standard_normal(R) * 0.1).astype(np.float32)
    t_dev, l_dev = _dev(table).clone(), _dev(lin).clone()
    m_dev, v_dev = torch.zeros_like(t_dev), torch.zeros_like(t_dev)
    ml_dev, vl_dev = torch.zeros_like(l_dev), torch.zeros_like(l_dev)
    tt, tl = torch.tensor(table, dtype=torch.float64), torch.tensor(lin, dtype=torch.float64)
    tm, tv, tml, tvl = torch.zeros_like(tt), torch.zeros_like(tt), torch.zeros_like(tl), torch.zeros_like(tl)
    d_rb = _dev(row_base)
    zero_bias = torch.zeros(1, device="cuda")
    for step in range(1, 4):
        ids = rng.integers(0, V, size=(B, F))
        if hot:
            ids[:, 0] = 3
        ids[rng.random((B, F)) < 0.05] = -1
        grad = rng.standard_normal((B, F * D)).astype(np.float32)
        dl = rng.standard_normal(B).astype(np.float32)
        d_ids = _dev(ids)
        plan = ops.emb_sort_slots(d_ids, d_rb, R)
        concat, sum_x, _ = ops.emb_pool_fwd(d_ids, F, None, d_rb, t_dev, l_dev, zero_bias)       # forward activations
        ops.emb_pool_bwd_sorted_adam(d_ids, d_rb, plan, D, R, _dev(grad), _dev(dl), ops.adam_lr_t(lr, b1, b2, step), b1, b2, eps,
                                     t_dev, m_dev, v_dev, l_dev, ml_dev, vl_dev, concat=concat, sum_x=sum_x)
        # oracle (fp64): per-slot gradient incl. the FM term, summed per row, then the row-wise Adam update
        rows = torch.tensor(np.where(ids >= 0, ids + row_base[None, :], -1))
        x = torch.zeros((B, F, D), dtype=torch.float64)
        mask = rows >= 0
        x[mask] = tt[rows[mask]]
        sx = x.sum(1)
        g = torch.tensor(grad, dtype=torch.float64).reshape(B, F, D) + torch.tensor(dl, dtype=torch.float64)[:, None, None] * (sx[:, None, :] - x)
        dense_g = torch.zeros_like(tt)
        dense_g.index_add_(0, rows[mask], g[mask])
        dense_gl = torch.zeros_like(tl)
        dense_gl.index_add_(0, rows[mask], torch.tensor(dl, dtype=torch.float64)[:, None].expand(B, F)[mask])
        T.adam_rows_step(tt, dense_g, rows.reshape(-1), tm, tv, lr, step, b1, b2, eps)
        T.adam_rows_step(tl, dense_gl, rows.reshape(-1), tml, tvl, lr, step, b1, b2, eps)
    # Adam normalises every step to ~lr whatever the gradient's size, and m / sqrt(v) of a tiny gradient is where fp32 and
    # fp64 differ most: parameters are compared to 1 % of one step, the moments relatively
    np.testing.assert_allclose(t_dev.cpu().numpy(), tt.numpy(), rtol=0, atol=1e-2 * lr)
    np.testing.assert_allclose(l_dev.cpu().numpy(), tl.numpy(), rtol=0, atol=1e-2 * lr)
    np.testing.assert_allclose(m_dev.cpu().numpy(), tm.numpy(), rtol=1e-4, atol=1e-5 * (B if hot else 8))
    np.testing.assert_allclose(v_dev.cpu().numpy(), tv.numpy(), rtol=2e-4, atol=1e-5 * (B if hot else 8))
    np.testing.assert_allclose(ml_dev.cpu().numpy(), tml.numpy(), rtol=1e-4, atol=1e-5 * (B if hot else 8))


def test_adam_step_dense(ops):
    rng = np.random.default_rng(34)
    n = 100003
    p = rng.standard_normal(n).astype(np.float32)
    pd, md, vd = _dev(p).clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    tp, tm, tv = torch.tensor(p, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 5):
        g = rng.standard_normal(n).astype(np.float32)
        ops.adam_step(pd, _dev(g), md, vd, ops.adam_lr_t(0.01, 0.9, 0.999, step), 0.9, 0.999, 1e-8, grad_scale=0.5)
        T.adam_dense_step(tp, torch.tensor(g, dtype=torch.float64) * 0.5, tm, tv, 0.01, step)
    np.testing.assert_allclose(pd.cpu().numpy(), tp.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(md.cpu().numpy(), tm.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(vd.cpu().numpy(), tv.numpy(), rtol=1e-5, atol=1e-7)


def test_ftrl_step_dense(ops):
    rng = np.random.default_rng(35)
    n = 50021
    p = (rng.standard_normal(n) * 0.5).astype(np.float32)
    pd, ad, ld = _dev(p).clone(), torch.full((n,), 0.1, device="cuda"), torch.zeros(n, device="cuda")
    tp = torch.tensor(p, dtype=torch.float64)
    ta, tl = torch.full((n,), 0.1, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for _ in range(4):
        g = (rng.standard_normal(n) * 2).astype(np.float32)
        ops.ftrl_step(pd, _dev(g), ad, ld, 0.01, -0.5, 0.5, 0.001)
        T.ftrl_dense_step(tp, torch.tensor(g, dtype=torch.float64), ta, tl, 0.01, -0.5, 0.5, 0.001)
    np.testing.assert_allclose(pd.cpu().numpy(), tp.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ad.cpu().numpy(), ta.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ld.cpu().numpy(), tl.numpy(), rtol=1e-4, atol=1e-4)
    assert 0 < (pd == 0).float().mean().item() < 1                        # the l1 proximal step zeroes some weights


def test_linear_bwd_dx_fm_epilogue(ops):
    rng = np.random.default_rng(22)
    M, F, D, Nd, N = 300, 5, 16, 3, 40
    K = F * D + Nd
    ld = (K + 3) // 4 * 4
    dy = rng.standard_normal((M, N)).astype(np.float32)
    W = rng.standard_normal((K, N)).astype(np.float32)
    dl = rng.standard_normal(M).astype(np.float32)
    concat = np.zeros((M, ld), np.float32)
    concat[:, :K] = rng.standard_normal((M, K)).astype(np.float32)
    sum_x = concat[:, :F * D].reshape(M, F, D).sum(1)
    out = torch.empty((M, ld), device="cuda")
    ops.linear_bwd_dx_fm(_dev(dy), _dev(W), _dev(dl), _dev(sum_x), _dev(concat), D, F * D, out[:, :K])
    want = dy.astype(np.float64) @ W.T.astype(np.float64)
    fm = dl[:, None, None] * (sum_x[:, None, :] - concat[:, :F * D].reshape(M, F, D))
    want[:, :F * D] += fm.reshape(M, F * D)
    np.testing.assert_allclose(out[:, :K].cpu().numpy(), want, rtol=0, atol=2e-5 * (np.abs(want).max() + 1))


@pytest.mark.parametrize("hot", [False, True])
def test_emb_bwd_sorted_with_fm_term_equals_atomic_kernel(ops, hot):
    rng = np.random.default_rng(23)
    B, F, D, V = 900, 9, 32, 400
    ids = rng.integers(0, V, size=(B, F))
    if hot:
        ids[:, 2] = 7                                   # one row shared by every example: 29 pieces of 32 slots
        ids[::3, 5] = 11                                # and one hit 300 times
    ids[rng.random((B, F)) < 0.05] = -1
    row_base = (np.arange(F) * V).astype(np.int64)
    R = F * V
    table = rng.standard_normal((R, D)).astype(np.float32)
    lin = rng.standard_normal(R).astype(np.float32)
    d_ids, d_rb = _dev(ids), _dev(row_base)
    cs = _dev(np.arange(F + 1).astype(np.int32))
    concat, sum_x, _ = ops.emb_pool_fwd(d_ids, F, None, d_rb, _dev(table), _dev(lin), None)
    d_concat = _dev(rng.standard_normal((B, F * D)).astype(np.float32))
    dl = _dev(rng.standard_normal(B).astype(np.float32))
    t1, l1, b1 = _dev(table).clone(), _dev(lin).clone(), torch.zeros(1, device="cuda")
    ops.emb_pool_bwd(d_ids, F, cs, d_rb, D, d_concat, concat, sum_x, dl, -0.2, t1, l1, b1)
    plan = ops.emb_sort_slots(d_ids, d_rb, R)
    srows, sslots, flags = plan.rows, plan.slots, plan.flags
    t2, l2, b2 = _dev(table).clone(), _dev(lin).clone(), torch.zeros(1, device="cuda")
    ops.emb_pool_bwd_sorted(d_ids, d_rb, plan, D, R, d_concat, dl, -0.2, t2, l2, b2, concat=concat, sum_x=sum_x)
    atol = 1e-5 * (B if hot else 1)
    np.testing.assert_allclose(t2.cpu().numpy(), t1.cpu().numpy(), rtol=1e-5, atol=atol)
    np.testing.assert_allclose(l2.cpu().numpy(), l1.cpu().numpy(), rtol=1e-5, atol=atol)
    assert abs(b1.item() - b2.item()) < 1e-3
    # concat never built: x of the shared-row slots from the snapshot taken before the update; hot rows' pieces parked in the same
    # buffer and applied in order -- same result, bit-identical run to run
    # (the deterministic update reads x from the table itself, so the snapshot is optional: second run without it, buffer all NaN)
    res = []
    for snap in (True, False):
        t3, l3, b3 = _dev(table).clone(), _dev(lin).clone(), torch.zeros(1, device="cuda")
        xs = torch.full((B * F, D), float("nan"), device="cuda")
        if snap:
            ops.emb_snapshot_sorted_rows(plan, t3, R, xs)
        ops.emb_pool_bwd_sorted(d_ids, d_rb, plan, D, R, d_concat, dl, -0.2, t3, l3, b3, sum_x=sum_x, x_sorted=xs)
        res.append((t3.cpu().numpy(), l3.cpu().numpy()))
    np.testing.assert_allclose(res[0][0], t1.cpu().numpy(), rtol=1e-5, atol=atol)
    np.testing.assert_allclose(res[0][1], l1.cpu().numpy(), rtol=1e-5, atol=atol)
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])


# ---------------------------------------------------------------- GEMM product modes
def test_gemm_bf16x3_matches_fp64_as_well_as_native(ops):
    """The default GEMM mode forms fp32 products from six bf16 MFMA products of exact three-way operand splits.  Its error
    against an fp64 reference must not exceed the native fp32 MFMA path's (same accumulation order, same fp32 accumulators);
    shapes cover the lean k-loop, the reduction tail (K % 32 != 0), edge tiles in M and N, and a wide dynamic range."""
    g = torch.Generator(device="cuda").manual_seed(5)
    M, K, N = 1000, 333, 200
    x = torch.randn((M, K), device="cuda", generator=g) * torch.exp(3 * torch.randn((M, 1), device="cuda", generator=g))
    W = torch.randn((K, N), device="cuda", generator=g) / K ** 0.5
    b = torch.randn(N, device="cuda", generator=g)
    dy = torch.randn((M, N), device="cuda", generator=g)
    ref_y = x.double() @ W.double() + b.double()
    ref_dx = dy.double() @ W.double().t()
    ref_dw = x.double().t() @ dy.double()
    ref_db = dy.double().sum(0)
    errs = {}
    prev = ops.get_gemm_mode()
    try:
        for mode in ("native", "bf16x3"):
            ops.set_gemm_mode(mode)
            assert ops.get_gemm_mode() == mode
            y = ops.linear_fwd(x, W, b, 0)
            dx = ops.linear_bwd_dx(dy, W, None)
            dW = torch.zeros((K, N), device="cuda"); db = torch.zeros(N, device="cuda")
            ops.linear_bwd_dw(x, dy, 1.0, dW, db, workspace=ops.linear_bwd_dw_workspace(M, K, N, "cuda"))
            errs[mode] = [float((y.double() - ref_y).abs().max() / ref_y.abs().max()),
                          float((dx.double() - ref_dx).abs().max() / ref_dx.abs().max()),
                          float((dW.double() - ref_dw).abs().max() / ref_dw.abs().max()),
                          float((db.double() - ref_db).abs().max() / ref_db.abs().max())]
    finally:
        ops.set_gemm_mode(prev)
    for e_nat, e_bf3 in zip(errs["native"], errs["bf16x3"]):
        assert e_bf3 <= 2e-6, errs                       # fp32-level agreement with fp64
        assert e_bf3 <= 1.5 * e_nat + 1e-7, errs        # and no worse than the native fp32 MFMA path


@pytest.mark.parametrize("mode", ["bf16x3", "native"])
def test_gemm_componentwise_error_bound_per_row(ops, mode):
    """Per-ELEMENT accuracy: rows of x span e^+-9 in magnitude, so a global max-norm would only see the
    largest rows.  Every output element must satisfy the componentwise fp32 bound |err_ij| <= c * sqrt(K) * 2^-24 * (|x| |W|)_ij
    (c = 4: the accumulation is a K-long fp32 chain; the bf16x3 split drops terms below 2^-24 |x_ik w_kj| each), i.e. each row
    is judged against its own scale; same for dgrad (rows of dy scaled) and wgrad (columns inherit both operands' scales)."""
    g = torch.Generator(device="cuda").manual_seed(11)
    M, K, N = 1024, 333, 200
    rs = torch.exp(3 * torch.randn((M, 1), device="cuda", generator=g))           # e^+-9 across rows
    x = torch.randn((M, K), device="cuda", generator=g) * rs
    W = torch.randn((K, N), device="cuda", generator=g) / K ** 0.5
    dy = torch.randn((M, N), device="cuda", generator=g) * rs
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(mode)
    try:
        y = ops.linear_fwd(x, W, None, 0)
        dx = ops.linear_bwd_dx(dy, W, None)
        dW = torch.zeros((K, N), device="cuda")
        ops.linear_bwd_dw(x, dy, 1.0, dW, None, workspace=ops.linear_bwd_dw_workspace(M, K, N, "cuda"))
    finally:
        ops.set_gemm_mode(prev)
    u = 2.0 ** -24
    for name, got, a, b, red in (("fwd", y, x, W, K), ("dgrad", dx, dy, W.t(), N), ("wgrad", dW, x.t(), dy, M)):
        ref = a.double() @ b.double()
        bound = 4 * red ** 0.5 * u * (a.double().abs() @ b.double().abs())
        err = (got.double() - ref).abs()
        worst = float((err / bound).max())
        assert worst <= 1.0, (name, mode, worst)
        # the smallest-magnitude rows are resolved as well as the largest ones
        small = rs.reshape(-1).argsort()[:16]
        if name != "wgrad":
            rel = (err[small].max(dim=1).values / ref[small].abs().max(dim=1).values)
            assert float(rel.max()) <= 4e-6, (name, mode, float(rel.max()))


def test_gemm_bf16x3_special_operands(ops):
    """What the bf16x3 product mode does with operands outside the normal range:
    * fp32 subnormal operands: the split keeps at most bf16's 8 significant bits of a subnormal (absolute error < 2^-133 per
      value), their products are far below the accumulator's rounding -- results stay within the ordinary bound, and a row
      made only of subnormals yields a result of subnormal magnitude, finite;
    * +-inf operand: the residual inf - inf is NaN, so that output ROW is non-finite (native: +-inf / NaN by IEEE rules);
      every other row is untouched;
    * values near FLT_MAX whose bf16 rounding overflows behave like inf (same row-local effect)."""
    g = torch.Generator(device="cuda").manual_seed(12)
    M, K, N = 256, 96, 64
    x = torch.randn((M, K), device="cuda", generator=g)
    W = torch.randn((K, N), device="cuda", generator=g) / K ** 0.5
    x[3, ::7] = 1e-40
    x[3, 1::7] = -3e-39
    x[5, :] = 1e-40                                       # a row of subnormals only
    x[9, 4] = float("inf")
    x[11, 8] = 3.4e38                                     # bf16_rn overflows to inf
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode("bf16x3")
    try:
        y = ops.linear_fwd(x, W, None, 0)
    finally:
        ops.set_gemm_mode(prev)
    ok = torch.ones(M, dtype=torch.bool, device="cuda")
    ok[9] = ok[11] = False
    xr = x.clone()
    ref = xr[ok].double() @ W.double()
    bound = 4 * K ** 0.5 * 2.0 ** -24 * (xr[ok].double().abs() @ W.double().abs()) + 1e-37
    assert bool(torch.isfinite(y[ok]).all())
    assert float(((y[ok].double() - ref).abs() / bound).max()) <= 1.0
    assert float(y[5].abs().max()) <= 1e-37
    assert not bool(torch.isfinite(y[9]).all())           # inf operand: the row is poisoned (NaN / inf), documented
    assert not bool(torch.isfinite(y[11]).all()) or float((y[11].double() - x[11].double() @ W.double()).abs().max()) < 1e33


def test_gemm_mode_api(ops):
    prev = ops.set_gemm_mode("native")
    assert ops.set_gemm_mode("bf16x3") == "native"
    assert ops.get_gemm_mode() == "bf16x3"
    ops.set_gemm_mode(prev)
    with pytest.raises(ValueError):
        ops.set_gemm_mode(7)
    assert ops.get_gemm_mode() == prev


# ---- K7p: GEMMs on pre-split ("planes") operands ------------------------------------------------------------------------------
def _rel(got, ref):
    ref = ref.double()
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def test_bf3_split_join_exact_and_zero_padded():
    """x -> three bf16 planes -> x is the identity bit for bit (also transposed, at an offset), and the padding stays zero."""
    from deep_recommenders_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((77, 53), device="cuda", generator=g) * torch.exp(torch.randn((77, 1), device="cuda", generator=g) * 6)
    x[3, 5] = 0.0
    p = ops.bf3_split(x, ops.Planes(77, 53, "cuda"))
    assert torch.equal(ops.bf3_join(p), x)
    # a denormal may be flushed by the conversion (absolute error below 1.2e-38; DESIGN.md section 6 lists the out-of-range cases)
    xd = x.clone()
    xd[10, 0] = 1e-39
    assert (ops.bf3_join(ops.bf3_split(xd, ops.Planes(77, 53, "cuda"))) - xd).abs().max().item() <= 1.2e-38
    assert p.buf[:, 77:, :].abs().max() == 0 and p.buf[:, :, 53:].abs().max() == 0
    pt = ops.bf3_split(x, ops.Planes(53, 77, "cuda"), transpose=True)
    assert torch.equal(ops.bf3_join(pt), x.t().contiguous())


@pytest.mark.parametrize("M,K,N", [(200, 83, 40), (1000, 300, 257), (4096, 128, 520), (300, 64, 600), (2085, 1677, 256), (513, 32, 1677)])
def test_bf3_linear_nt_matches_fp64(M, K, N):
    """dr_bf3_linear_nt (fp32 activations split in registers x pre-split weights): forward with bias + ReLU, dgrad with a ReLU'
    mask, accumulate -- against float64, no worse than the in-kernel-split GEMM (both are six exact bf16 products per fp32 product).
    Shapes: edge tiles in both dimensions, a reduction tail (K % 32 != 0, K % 4 != 0), K < one k-tile, the bench's first layer."""
    from deep_recommenders_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M + N)
    x = torch.randn((M, K), device="cuda", generator=g)
    W = torch.randn((K, N), device="cuda", generator=g) * 0.1
    b = torch.randn((N,), device="cuda", generator=g)
    wp = ops.WeightPlanes(W)
    y = ops.bf3_linear_nt(x, wp.wt, bias=b, act=1)
    ref = torch.relu(x.double() @ W.double() + b.double())
    e_new, e_old = _rel(y, ref), _rel(ops.linear_fwd(x, W, b, 1), ref)
    assert e_new <= 3e-6 and e_new <= 1.5 * e_old + 2e-7, (e_new, e_old)
    # dgrad with the ReLU' mask of the layer below, then accumulated on top of an existing buffer
    dy = torch.randn((M, N), device="cuda", generator=g) * 1e-2
    below = torch.randn((M, K), device="cuda", generator=g)
    dx = ops.bf3_linear_nt(dy, wp.w, mask=below)
    ref = (dy.double() @ W.double().t()) * (below > 0)
    assert _rel(dx, ref) <= 3e-6
    base = torch.randn((M, K), device="cuda", generator=g) * 1e-2
    acc = base.clone()
    ops.bf3_linear_nt(dy, wp.w, accumulate=True, out=acc)
    assert _rel(acc, base.double() + dy.double() @ W.double().t()) <= 3e-6
    # NaN-poisoned padding of the ACTIVATION must not leak in (the kernel reads whole 16-byte vectors past K)
    xp = torch.full((M, (K + 3) // 4 * 4 + 4), float("nan"), device="cuda")
    xp[:, :K] = x
    assert torch.equal(ops.bf3_linear_nt(xp[:, :K], wp.wt, bias=b, act=1), y)


@pytest.mark.parametrize("M,F,Nd,K,fm", [(300, 3, 0, 40, True), (2085, 26, 13, 256, True), (4096, 7, 5, 64, False), (513, 1, 2, 256, True)])
def test_bf3_linear_nt_pack_equals_dgrad_then_pack(M, F, Nd, K, fm):
    """dr_bf3_linear_nt_pack (first-layer dgrad + dr_emb_pack_grads in one launch) == dr_bf3_linear_nt followed by dr_emb_pack_grads:
    every slot's gradient row at its permuted destination, the first-order copies, the bias sum.  Same accumulators, same FM
    expression; the one fused multiply-add the compiler may form differently bounds the difference at an ulp of the terms."""
    from deep_recommenders_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M + F)
    N = 64 * F + Nd
    dy = torch.randn((M, K), device="cuda", generator=g) * 1e-2
    W = torch.randn((N, K), device="cuda", generator=g) * 0.1          # first layer [in = N, out = K]
    wp = ops.WeightPlanes(W)
    pos = torch.randperm(M * F, device="cuda", generator=g).reshape(M, F)
    dl = torch.randn((M,), device="cuda", generator=g)
    ldc = (N + 3) // 4 * 4
    concat = torch.randn((M, ldc), device="cuda", generator=g)
    sum_x = concat[:, :64 * F].reshape(M, F, 64).sum(1).contiguous()
    # reference: two kernels
    d_concat = torch.zeros((M, ldc), device="cuda")
    ops.bf3_linear_nt(dy, wp.w, out=d_concat[:, :N])
    rows0 = torch.full((M * F, 64), float("nan"), device="cuda")
    lin0 = torch.full((M * F,), float("nan"), device="cuda")
    b0 = torch.zeros(1, device="cuda")
    ops.emb_pack_grads(pos, 64, d_concat, concat if fm else None, sum_x if fm else None, dl, rows0, lin0, b0)
    # fused
    rows1 = torch.full((M * F, 64), float("nan"), device="cuda")
    lin1 = torch.full((M * F,), float("nan"), device="cuda")
    b1 = torch.zeros(1, device="cuda")
    ops.bf3_linear_nt_pack(dy, wp.w, pos, dl, rows1, lin1, b1, sum_x=sum_x if fm else None, x=concat if fm else None)
    assert not torch.isnan(rows1).any() and not torch.isnan(lin1).any()          # a permutation: every destination written
    assert torch.equal(lin1, lin0) and torch.equal(b1, b0)
    scale = (rows0.abs().max().item() + 1e-30)
    assert (rows1 - rows0).abs().max().item() <= 2e-7 * scale + 1e-7 * (dl.abs().max().item() * concat.abs().max().item())
    if not fm:
        assert torch.equal(rows1, rows0)


@pytest.mark.parametrize("M,F,Nd,K", [(1024, 26, 13, 256), (512, 3, 0, 64), (2048, 7, 5, 32)])
def test_h2_linear_nt_pack_equals_dgrad_then_pack(M, F, Nd, K):
    """dr_h2_linear_nt_pack (round 5: the first-layer dgrad in the f16x2 split with the gradient pack as its epilogue -- accumulator
    blocks turned through the LDS, float4 moves) == dr_h2_linear_nt followed by dr_emb_pack_grads: every slot's gradient row at its
    permuted destination, the first-order copies, the bias sum.  Same accumulators, same FM expression up to the one fused
    multiply-add the compiler may form differently.  Outside the epilogue's domain (M not a multiple of 256) the entry point says
    DR_ESHAPE and the caller keeps the two launches."""
    from deep_recommenders_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M + F)
    N = 64 * F + Nd
    dy = torch.randn((M, K), device="cuda", generator=g) * 1e-2
    W = torch.randn((N, K), device="cuda", generator=g) * 0.1          # first layer [in = N, out = K]
    wp = ops.H2WeightPlanes(W)
    dy_amax = ops.h2_amax(dy)
    pos = torch.randperm(M * F, device="cuda", generator=g).reshape(M, F)
    dl = torch.randn((M,), device="cuda", generator=g)
    ldc = (N + 3) // 4 * 4
    concat = torch.randn((M, ldc), device="cuda", generator=g)
    sum_x = concat[:, :64 * F].reshape(M, F, 64).sum(1).contiguous()
    d_concat = torch.zeros((M, ldc), device="cuda")
    ops.h2_linear_nt(dy, dy_amax, wp.w, out=d_concat[:, :N])
    rows0 = torch.full((M * F, 64), float("nan"), device="cuda")
    lin0 = torch.full((M * F,), float("nan"), device="cuda")
    b0 = torch.zeros(1, device="cuda")
    ops.emb_pack_grads(pos, 64, d_concat, concat, sum_x, dl, rows0, lin0, b0)
    rows1 = torch.full((M * F, 64), float("nan"), device="cuda")
    lin1 = torch.full((M * F,), float("nan"), device="cuda")
    b1 = torch.zeros(1, device="cuda")
    ops.h2_linear_nt_pack(dy, dy_amax, wp.w, pos, dl, rows1, lin1, b1, sum_x=sum_x, x=concat)
    assert not torch.isnan(rows1).any() and not torch.isnan(lin1).any()          # a permutation: every destination written
    assert torch.equal(lin1, lin0) and torch.equal(b1, b0)
    scale = (rows0.abs().max().item() + 1e-30)
    assert (rows1 - rows0).abs().max().item() <= 2e-7 * scale + 1e-7 * (dl.abs().max().item() * concat.abs().max().item())
    with pytest.raises(RuntimeError, match="DR_ESHAPE"):
        ops.h2_linear_nt_pack(dy[:100], dy_amax, wp.w, pos[:100], dl[:100], rows1, lin1, b1, sum_x=sum_x[:100], x=concat[:100])


_RS64_SNIPPET = r"""
import hashlib, sys, torch
sys.path.insert(0, %r)
from deep_recommenders_amd import ops
h = hashlib.sha256()
for (M, K, N) in [(1000, 300, 257), (2085, 1677, 256), (513, 32, 1677), (66000, 256, 300)]:
    g = torch.Generator(device="cuda").manual_seed(M + N)
    x = torch.randn((M, K), device="cuda", generator=g)
    W = torch.randn((K, N), device="cuda", generator=g) * 0.1
    b = torch.randn((N,), device="cuda", generator=g)
    wp = ops.WeightPlanes(W)
    y = ops.bf3_linear_nt(x, wp.wt, bias=b, act=1)
    dy = torch.randn((M, N), device="cuda", generator=g) * 1e-2
    below = torch.randn((M, K), device="cuda", generator=g)
    dx = ops.bf3_linear_nt(dy, wp.w, mask=below)
    acc = below.clone()
    ops.bf3_linear_nt(dy, wp.w, accumulate=True, out=acc)
    ref = torch.relu(x.double() @ W.double() + b.double())
    assert ((y.double() - ref).abs().max() / ref.abs().max()).item() <= 3e-6
    for t in (y, dx, acc):
        h.update(t.contiguous().cpu().numpy().tobytes())
print("DIGEST", h.hexdigest())
"""


def test_bf3_linear_nt_rs64_bit_identical():
    """The register-split GEMM's 4-wave x 64-row shape (DR_BF3_RS64=1: one wave per SIMD, 256 accumulator registers; read once per
    process) gives bit for bit what the default 8-wave x 32-row shape gives: forward, masked dgrad, accumulate; edge tiles, a
    reduction tail, more than one tile per block."""
    import os, subprocess, sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    out = []
    for flag in ("0", "1", "2"):      # 2: 8 waves x (64 rows x 128 columns), the column-split shape
        env = dict(os.environ, DR_BF3_RS64=flag)
        r = subprocess.run([sys.executable, "-c", _RS64_SNIPPET % root], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append([l for l in r.stdout.splitlines() if l.startswith("DIGEST")][-1])
    assert out[0] == out[1] == out[2], out


@pytest.mark.parametrize("M,F,Nd,N", [(300, 3, 0, 40), (2085, 26, 13, 256), (4096, 7, 5, 300), (257, 1, 2, 64),
                                      (70000, 2, 3, 64), (40001, 1, 0, 600)])
def test_bf3_emb_linear_fwd_equals_pool_then_linear(M, F, Nd, N):
    """dr_bf3_emb_linear_fwd (K3 fused into the first Dense layer) == dr_emb_pool_fwd followed by dr_bf3_linear_nt:
    concat's embedding part bit for bit (it is a copy of table rows; missing ids give zeros), sum_x / fm_logit within fp32
    summation-order noise, and the layer output bit for bit (same splits, same k order, same accumulation as dr_bf3_linear_nt).
    The last two shapes have more output tiles than the 256 persistent blocks (274; 157 x 3 = 471 with three column tiles per row
    panel, of which only the first stores concat / the FM terms): the gather pipeline runs across tile boundaries."""
    from deep_recommenders_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M + F)
    D, V = 64, 97
    table = torch.randn((F * V, D), device="cuda", generator=g) * 0.3
    lin_w = torch.randn((F * V,), device="cuda", generator=g)
    lin_b = torch.tensor([0.37], device="cuda")
    row_base = (torch.arange(F, device="cuda") * V).to(torch.int64)
    ids = torch.randint(0, V, (M, F), device="cuda", generator=g)
    ids[torch.rand((M, F), device="cuda", generator=g) < 0.05] = -1                     # missing values
    K = F * D + Nd
    ld = (K + 3) // 4 * 4
    dense = torch.randn((M, Nd), device="cuda", generator=g)
    W = torch.randn((K, N), device="cuda", generator=g) * 0.1
    b = torch.randn((N,), device="cuda", generator=g)
    wp = ops.WeightPlanes(W)
    # the two-kernel path
    concat0 = torch.zeros((M, ld), device="cuda")
    sum0, fm0 = torch.empty((M, D), device="cuda"), torch.empty((M,), device="cuda")
    ops.emb_pool_fwd(ids, F, None, row_base, table, lin_w, lin_b, ld_concat=ld, concat=concat0, sum_x=sum0, fm_logit=fm0)
    concat0[:, F * D:K] = dense
    y0 = ops.bf3_linear_nt(concat0[:, :K], wp.wt, bias=b, act=1)
    # the fused kernel; its concat starts NaN-poisoned in the part it must write
    concat1 = torch.zeros((M, ld), device="cuda")
    concat1[:, :F * D] = float("nan")
    concat1[:, F * D:K] = dense
    sum1, fm1 = torch.full((M, D), float("nan"), device="cuda"), torch.full((M,), float("nan"), device="cuda")
    y1 = torch.full((M, N), float("nan"), device="cuda")
    dpad = None
    if Nd:
        dpad = torch.zeros((M, 32), device="cuda")
        dpad[:, :Nd] = dense
    ops.bf3_emb_linear_fwd(ids, row_base, V, table, lin_w, lin_b, dpad, concat1, K, wp.wt, b, 1, sum1, fm1, y1)
    assert torch.equal(concat1, concat0)
    assert torch.equal(y1, y0)
    assert (sum1 - sum0).abs().max().item() <= 1e-5 * max(1.0, sum0.abs().max().item())
    assert (fm1 - fm0).abs().max().item() <= 2e-5 * max(1.0, fm0.abs().max().item())
    # D != 64 and fields of more than 2^24 rows are refused, the caller falls back to the two kernels
    with pytest.raises(RuntimeError):
        ops.bf3_emb_linear_fwd(ids, row_base, (1 << 24) + 1, table, lin_w, lin_b, dpad, concat1, K, wp.wt, b, 1, sum1, fm1, y1)
    with pytest.raises(RuntimeError):
        ops.bf3_emb_linear_fwd(ids, row_base, V, torch.zeros((F * V, 32), device="cuda"), lin_w, lin_b, dpad, concat1, K, wp.wt, b, 1, sum1, fm1, y1)


def test_bf3_emb_linear_fwd_reaches_past_4gb():
    """A slab larger than 4 GB: the fused kernel addresses every field through its own buffer resource (32-bit offsets), rows
    whose byte offset in the slab is beyond 2^32 must come out right (a resource over the whole slab wraps there)."""
    from deep_recommenders_amd import ops
    R, F, M, N, K = 20_000_000, 2, 1024, 64, 128
    table = torch.empty((R, 64), device="cuda")
    table.copy_(torch.arange(R, device="cuda", dtype=torch.float32).view(-1, 1).expand(R, 64) * 1e-6)
    row_base = torch.tensor([0, R // 2], device="cuda", dtype=torch.int64)
    g = torch.Generator(device="cuda").manual_seed(1)
    ids = torch.randint(0, R // 2, (M, F), device="cuda", generator=g)
    ids[:4, 1] = torch.tensor([R // 2 - 1, R // 2 - 2, 6777216, 6777215], device="cuda")      # slab rows around 2^24 and the last one
    wp = ops.WeightPlanes(torch.randn((K, N), device="cuda", generator=g) * 0.1)
    concat = torch.zeros((M, K), device="cuda")
    sx, fm, y = torch.empty((M, 64), device="cuda"), torch.empty((M,), device="cuda"), torch.empty((M, N), device="cuda")
    ops.bf3_emb_linear_fwd(ids, row_base, R // 2, table, None, None, None, concat, K, wp.wt, torch.zeros((N,), device="cuda"), 0, sx, fm, y)
    want = torch.cat([table[ids[:, 0]], table[ids[:, 1] + R // 2]], dim=1)
    assert torch.equal(concat, want)
    assert torch.equal(y, ops.bf3_linear_nt(want, wp.wt, bias=torch.zeros((N,), device="cuda"), act=0))


def test_bf3_cross_fwd_matches_cross_fwd_and_fp64():
    """DCN cross layer on pre-split weights == dr_cross_fwd's math (dcn.py:81-88), incl. the reference's known answer."""
    from deep_recommenders_amd import ops
    x0 = torch.tensor([[0.1, 0.2, 0.3]], device="cuda").repeat(5, 1)
    x = torch.tensor([[0.4, 0.5, 0.6]], device="cuda").repeat(5, 1)
    W = torch.ones((3, 3), device="cuda")
    x0p, xp = torch.zeros((5, 4), device="cuda"), torch.zeros((5, 4), device="cuda")
    x0p[:, :3], xp[:, :3] = x0, x
    out, _ = ops.bf3_cross_fwd(x0p[:, :3], xp[:, :3], ops.WeightPlanes(W).wt, torch.zeros(3, device="cuda"))
    np.testing.assert_allclose(out.cpu().numpy(), np.tile([[0.55, 0.8, 1.05]], (5, 1)), rtol=1e-6)     # tests/keras/test_dcn.py:16-23
    g = torch.Generator(device="cuda").manual_seed(4)
    M, Dm = 1500, 333
    buf0 = torch.randn((M, 336), device="cuda", generator=g)
    buf1 = torch.randn((M, 336), device="cuda", generator=g)
    x0, x = buf0[:, :Dm], buf1[:, :Dm]
    W = torch.randn((Dm, Dm), device="cuda", generator=g) * 0.05
    b = torch.randn((Dm,), device="cuda", generator=g)
    out, prod = ops.bf3_cross_fwd(x0, x, ops.WeightPlanes(W).wt, b, 0.3, want_prod=True)
    pr = x.double() @ W.double() + b.double() + 0.3 * x.double()
    assert _rel(prod, pr) <= 3e-6 and _rel(out, x0.double() * pr + x.double()) <= 3e-6
    o2, p2 = ops.cross_fwd(x0, x, W, b, 0.3, want_prod=True)
    assert _rel(out, o2) <= 2e-6 and _rel(prod, p2) <= 2e-6


@pytest.mark.parametrize("M,K,N", [(200, 83, 40), (1000, 300, 257), (4096, 128, 520)])
def test_bf3_planes_gemms_match_fp64(M, K, N):
    """dr_bf3_gemm_nt / _tn (both operands pre-split, LDS-DMA staging; NaN-poisoned split-K workspace)."""
    from deep_recommenders_amd import ops
    g = torch.Generator(device="cuda").manual_seed(K)
    x = torch.randn((M, K), device="cuda", generator=g)
    W = torch.randn((K, N), device="cuda", generator=g) * 0.1
    dy = torch.randn((M, N), device="cuda", generator=g) * 1e-2
    xp, dyp = ops.bf3_split(x, ops.Planes(M, K, "cuda")), ops.bf3_split(dy, ops.Planes(M, N, "cuda"))
    wp = ops.WeightPlanes(W)
    assert _rel(ops.bf3_gemm_nt(xp, wp.wt), x.double() @ W.double()) <= 3e-6
    assert _rel(ops.bf3_gemm_nt(dyp, wp.w), dy.double() @ W.double().t()) <= 3e-6
    dW = torch.zeros((K, N), device="cuda")
    ws = ops.bf3_gemm_tn_workspace(M, K, N, "cuda").fill_(float("nan"))
    ops.bf3_gemm_tn(xp, dyp, 1.0, dW, workspace=ws)
    assert _rel(dW, x.double().t() @ dy.double()) <= 5e-6


@pytest.mark.parametrize("R,F,N", [(200, 83, 40), (1000, 300, 257), (4096, 128, 520), (2085, 1677, 256), (8192, 600, 300)])
def test_bf3_wgrad_matches_fp64(R, F, N):
    """dr_bf3_wgrad (both activations fp32, x split in registers, dy split once per tile into LDS): dW and db against float64, no
    worse than the in-kernel-split wgrad; NaN-poisoned workspace (every partial the reduce reads must have been written);
    reduction tails (R % 32 != 0), edge tiles in f and n; accumulates into dstW with a scale (the fused SGD step)."""
    from deep_recommenders_amd import ops
    g = torch.Generator(device="cuda").manual_seed(R + F)
    x = torch.randn((R, F), device="cuda", generator=g)
    dy = torch.randn((R, N), device="cuda", generator=g) * 1e-2
    W0 = torch.randn((F, N), device="cuda", generator=g)
    b0 = torch.randn((N,), device="cuda", generator=g)
    W, b = W0.clone(), b0.clone()
    ws = ops.bf3_wgrad_workspace(R, F, N, "cuda").fill_(float("nan"))
    ops.bf3_wgrad(x, dy, -0.5, W, b, workspace=ws)
    refW = W0.double() - 0.5 * (x.double().t() @ dy.double())
    refb = b0.double() - 0.5 * dy.double().sum(0)
    dWref = x.double().t() @ dy.double()
    err = ((W.double() - refW).abs().max() / (0.5 * dWref.abs().max())).item()
    W2 = W0.clone()
    ops.linear_bwd_dw(x, dy, -0.5, W2, None, workspace=ops.linear_bwd_dw_workspace(R, F, N, "cuda"))
    err_old = ((W2.double() - refW).abs().max() / (0.5 * dWref.abs().max())).item()
    assert err <= 5e-6 and err <= 1.5 * err_old + 5e-7, (err, err_old)
    assert _rel(b, refb) <= 2e-6
    # deterministic: a second run gives the same bits
    W3, b3 = W0.clone(), b0.clone()
    ops.bf3_wgrad(x, dy, -0.5, W3, b3, workspace=ws)
    assert torch.equal(W3, W) and torch.equal(b3, b)
