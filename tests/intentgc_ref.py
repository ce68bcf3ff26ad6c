"""Float64 restatements for IntentGC (include/dr_hotpath.h, "IntentGC"; keras/models/retrieval/intentgc.py), written from the header's
comment and the paper's formulas with nothing shared with csrc/intent_conv.hip, the test shapes, the case builder and the error bounds.

Forward bounds (given).  u = 2^-24, gamma(n) = n u / (1 - n u).  A row of n_r entries is an fmaf chain from 0, so
    |agg - ref| <= gamma(n_r + 1) A_r,                      A_r = sum_k |val_k| |x_k|,  A_0 = |h_v| (exact)
    |p_i - ref| <= gamma(n_max + R + 2) PA_i,               PA_i = sum_r |W[i, r]| A_r      (R + 1 more fmaf steps)
    |out - ref| <= gamma(n_max + R + L + 4) sum_i |theta_i| PA_i                            (relu and linear are 1-Lipschitz)

Backward bounds (derived here).  The backward is a function of (h_self, agg, d_out, W, theta): the reference gets the SAME fp32 agg the
forward stored, so only the backward's own arithmetic is in the error.  Outside the kinks (below) fp32 and float64 take the same relu
branches.  With P_i = sum_r |W[i, r]| |a_r|, m_i = [p_i > 0], ds = d_out act'(s) (a selection: exact):
    p_i is recomputed by R + 1 fmaf steps:          |p^_i - p_i| <= gamma(R + 1) P_i, and the same for g_i = relu(p_i)
    dp_i = m_i theta_i ds is one product:           |dp^_i - dp_i| <= u |theta_i| |ds|
    d_a_r = sum_i W[i, r] dp_i, L fmaf steps on operands with one rounding each (d_self is r = 0, d_agg is r >= 1):
        |d_a_r^ - d_a_r| <= gamma(L + 1) sum_i |W[i, r]| |theta_i| m_i |ds|
    d_theta_i and d_W[i, r] are sums over every (v, c).  A term passes through d = 4 + iters + 6 + 3 + parts + 1 additions at most: the
    four-term fmaf chain of a lane's float4, the lane's `iters` destinations, six butterfly levels, three adds over the block's waves,
    and `parts` blocks from +0 ((iters, parts) = bwd_grid(n_dst, D), the kernel's grid, a function of the shape alone).  So
        |d_theta_i^ - d_theta_i| <= gamma(R + 1 + d) sum_{v,c} |ds| P_i          (g_i's error gamma(R + 1) P_i, |g_i| <= P_i)
        |d_W[i, r]^ - d_W[i, r]| <= gamma(1 + d) sum_{v,c} |theta_i| m_i |ds| |a_r|    (dp_i's one rounding, then the sum)
    A kink element may take the other branch in fp32.  It is left out of the d_self / d_agg comparison; in the two sums it cannot be
    left out, so its largest possible change is ADDED to their bounds: |d_out| (|p_i| + the bound of p_i) to d_theta_i, and
    |theta_i| |d_out| |a_r| to d_W[i, r].
    The input gradient d_h = [d_self; 0] + A^T d_agg adds one fmaf chain per source row of at most c_max + 1 steps (c_max = the longest
    column of the block) on top of d_a_r's error:  |d_h^ - d_h| <= gamma(L + c_max + 2) (|A|^T E_agg + E_self), E the sums above.

Kinks.  Element (v, c) is a kink when some |p_i| is below p_i's forward bound, or (relu outer activation) |s| is below out's forward
bound while some p_i > 0 (where every filter is off by more than its bound, s is exactly 0 in fp32 as in float64 and relu' is 0 in
both).  make_case asserts that at most 0.1 % of a case's elements are kinks."""
import numpy as np
import torch

import sage_ref

U = 2.0 ** -24
KINK_LIMIT = 1e-3            # the fraction of a case's elements that may be kinks
LONG_ROW = 512               # DR_CSR_LONG_ROW: dr_csr_spmm splits longer rows (the fused kernel does not)

#          n_dst, n_src, R, max row length, D, L
SHAPES = [(5, 9, 1, 3, 4, 1),            # every minimum: one lane per group, one filter
          (67, 150, 3, 10, 64, 4),       # odd row count, the last wave partly idle
          (33, 80, 7, 5, 256, 16),       # every maximum: 64-lane groups, the largest register footprint
          (130, 300, 2, 64, 12, 3),      # D / 4 = 3 is no power of two: one idle lane per group; the largest fanout
          (9, 700, 2, 600, 32, 2)]       # rows longer than DR_CSR_LONG_ROW, many iterations of the gather loop


def gamma(n):
    return n * U / (1.0 - n * U)


def bwd_grid(n_dst, D):
    """(passes per block, blocks) of dr_intent_conv_bwd, from the header: a group of pow2ceil(D / 4) lanes per destination, 256 lanes per
    block and pass, at most 512 blocks while a block has one pass"""
    g = 1
    while g < D // 4:
        g *= 2
    dpp = 256 // g
    passes = -(-n_dst // dpp)
    iters = max(1, -(-passes // 512))
    return iters, -(-passes // iters)


# ---- the layer ---------------------------------------------------------------------------------------------------------------------
def typed_aggregate(row_ptr, col, val, h, n_dst, R):
    """(agg, A, n) float64 [n_dst, R, D] x 2 and int [n_dst, R]: the rows' sums, the sums of magnitudes and the row lengths"""
    h = np.asarray(h, np.float64)
    D = h.shape[1]
    agg, A = np.zeros((n_dst, R, D)), np.zeros((n_dst, R, D))
    n = np.zeros((n_dst, R), dtype=np.int64)
    for q in range(n_dst * R):
        lo, hi = int(row_ptr[q]), int(row_ptr[q + 1])
        v, r = divmod(q, R)
        for k in range(lo, hi):
            agg[v, r] += float(val[k]) * h[col[k]]
            A[v, r] += abs(float(val[k])) * np.abs(h[col[k]])
        n[v, r] = hi - lo
    return agg, A, n


def conv_forward(h_self, agg, W, theta, act):
    """(p [n, L, D], s [n, D], out [n, D]) in the arrays' dtype: a = [h_self | agg], p_i = sum_r W[i, r] a_r, s = sum_i theta_i relu(p_i)"""
    a = np.concatenate([h_self[:, None, :], agg], axis=1)                  # [n, R + 1, D]
    p = np.einsum("ir,nrd->nid", W, a)
    s = np.einsum("i,nid->nd", theta, np.maximum(p, 0))
    return p, s, (np.maximum(s, 0) if act == 1 else s)


def conv_backward(h_self, agg, W, theta, act, d_out):
    """(d_self [n, D], d_agg [n, R, D], d_W [L, R + 1], d_theta [L]) by the explicit formulas of the header"""
    a = np.concatenate([h_self[:, None, :], agg], axis=1)
    p, s, _ = conv_forward(h_self, agg, W, theta, act)
    ds = d_out * (s > 0) if act == 1 else d_out
    d_theta = np.einsum("nd,nid->i", ds, np.maximum(p, 0))
    dp = (p > 0) * theta[None, :, None] * ds[:, None, :]                   # [n, L, D]
    d_W = np.einsum("nid,nrd->ir", dp, a)
    d_a = np.einsum("ir,nid->nrd", W, dp)
    return d_a[:, 0], d_a[:, 1:], d_W, d_theta


def conv_torch(h_self, agg, W, theta, act):
    """the composed expression on torch tensors (any dtype), for autograd"""
    a = torch.cat([h_self[:, None, :], agg], dim=1)
    s = torch.einsum("i,nid->nd", theta, torch.relu(torch.einsum("ir,nrd->nid", W, a)))
    return torch.relu(s) if act == 1 else s


def forward_bounds(case, h_self, agg64, A, n):
    """(agg bound [n, R, D], p bound [n, L, D], out bound [n, D], PA [n, L, D]) of the docstring, for float64 references of the case"""
    W, theta, R, L = np.abs(case["W"].astype(np.float64)), np.abs(case["theta"].astype(np.float64)), case["R"], case["L"]
    n_max = int(n.max()) if n.size else 0
    AA = np.concatenate([np.abs(h_self)[:, None, :], A], axis=1)
    PA = np.einsum("ir,nrd->nid", W, AA)
    g_agg = np.asarray([gamma(int(x) + 1) for x in n.reshape(-1)]).reshape(n.shape)[:, :, None]
    return g_agg * A, gamma(n_max + R + 2) * PA, gamma(n_max + R + L + 4) * np.einsum("i,nid->nd", theta, PA), PA


def kinks(case, p, s, p_bound, out_bound):
    """bool [n, D]: the elements fp32 may decide differently"""
    k = (np.abs(p) < p_bound).any(axis=1)
    if case["act"] == 1:
        k |= (np.abs(s) < out_bound) & (p > 0).any(axis=1)                 # with every filter off, s is exactly 0 in both precisions
    return k


def backward_bounds(case, h_self, agg, d_out, kink, p_bound):
    """bounds of (d_self, d_agg, d_W, d_theta) for a float64 reference on the same (h_self, agg); see the docstring"""
    W, theta, R, L, act = (case["W"].astype(np.float64), case["theta"].astype(np.float64), case["R"], case["L"], case["act"])
    n_dst, D = h_self.shape
    a = np.abs(np.concatenate([h_self[:, None, :], agg], axis=1))
    p, s, _ = conv_forward(h_self, agg, W, theta, act)
    ds = np.abs(d_out * (s > 0) if act == 1 else d_out)
    m = p > 0
    P = np.einsum("ir,nrd->nid", np.abs(W), a)
    iters, parts = bwd_grid(n_dst, D)
    d = 4 + iters + 6 + 3 + parts + 1
    e_a = gamma(L + 1) * np.einsum("ir,nid->nrd", np.abs(W), m * np.abs(theta)[None, :, None] * ds[:, None, :])
    e_theta = gamma(R + 1 + d) * np.einsum("nd,nid->i", ds, P)
    e_W = gamma(1 + d) * np.einsum("nid,nrd->ir", m * np.abs(theta)[None, :, None] * ds[:, None, :], a)
    if kink.any():
        ko = np.abs(d_out) * kink
        e_theta = e_theta + np.einsum("nd,nid->i", ko, np.abs(p) + p_bound)
        e_W = e_W + np.einsum("nid,nrd->ir", np.abs(theta)[None, :, None] * ko[:, None, :] * np.ones_like(p), a)
    return e_a[:, 0], e_a[:, 1:], e_W, e_theta


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def make_case(shape, grid=False, act=1, pitched=None, seed=0):
    """A typed block and a layer's inputs for `shape`.  grid: the integer grid (h and d_out in {-3 .. 3}, row lengths in {0, 1, 2, 4, 8}
    so that val is dyadic, W and theta in {-2 .. 2} / 2), every result exact in fp32.  Some virtual rows are empty, destination 1 has
    no neighbour of any type, one row has the full length, and every h row that no destination or neighbour refers to is NaN.  pitched:
    whether the GPU test passes h as a view with a row pitch > D (default: every other shape).  Asserts the kink condition."""
    n_dst, n_src, R, max_len, D, L = shape
    idx = SHAPES.index(tuple(shape)) if tuple(shape) in SHAPES else 0
    r = np.random.RandomState(1000 * seed + 10 * idx + (1 if grid else 0) + 2 * act)
    lens_allowed = [x for x in (1, 2, 4, 8) if x <= min(max_len, n_src)] if grid else None
    lens = np.zeros(n_dst * R, dtype=np.int64)
    for q in range(n_dst * R):
        if r.rand() < 0.2:
            continue                                                       # an empty virtual row
        lens[q] = r.choice(lens_allowed) if grid else r.randint(1, max_len + 1)
    lens[R:2 * R] = 0                                                      # destination 1: no neighbours at all
    lens[0] = max(lens_allowed) if grid else max_len                       # one row of the full length
    if n_dst * R > 2 * R:
        lens[2 * R] = 0
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([r.choice(n_src, size=int(x), replace=False) for x in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = np.concatenate([np.full(int(x), 1.0 / max(int(x), 1)) for x in lens] + [np.zeros(0)]).astype(np.float32)
    if grid:
        h = r.randint(-3, 4, size=(n_src, D)).astype(np.float32)
        d_out = r.randint(-3, 4, size=(n_dst, D)).astype(np.float32)
        W = (r.randint(-2, 3, size=(L, R + 1)) / 2.0).astype(np.float32)
        theta = (r.randint(-2, 3, size=(L,)) / 2.0).astype(np.float32)
    else:
        h = r.standard_normal((n_src, D)).astype(np.float32)
        d_out = r.standard_normal((n_dst, D)).astype(np.float32)
        W = r.standard_normal((L, R + 1)).astype(np.float32)
        theta = r.standard_normal((L,)).astype(np.float32)
    theta[0] = abs(theta[0]) if theta[0] != 0 else 0.5                     # with L = 1 a negative theta under the outer relu is a dead layer
    used = np.zeros(n_src, dtype=bool)
    used[:n_dst] = True
    used[col] = True
    h[~used] = np.nan
    case = dict(shape=tuple(shape), n_dst=n_dst, n_src=n_src, R=R, D=D, L=L, act=act, grid=grid, row_ptr=row_ptr, col=col, val=val, h=h,
                d_out=d_out, W=W, theta=theta, unused=int((~used).sum()), pitched=bool(idx % 2) if pitched is None else bool(pitched))
    if not grid:
        agg, A, n = typed_aggregate(row_ptr, col, val, h, n_dst, R)
        h_self = h[:n_dst].astype(np.float64)
        p, s, _ = conv_forward(h_self, agg, W.astype(np.float64), theta.astype(np.float64), act)
        _, p_bound, out_bound, _ = forward_bounds(case, h_self, agg, A, n)
        frac = kinks(case, p, s, p_bound, out_bound).mean()
        assert frac <= KINK_LIMIT, "case %s: %.3g of the elements are kinks" % (shape, frac)
        case["kink_fraction"] = float(frac)
    return case


def subset_case(case, keep):
    """the case with only the destinations `keep` (ascending positions) and the same h: rows v R .. v R + R - 1 of the CSR for v in keep.
    The kept destinations' own rows move to the top of a new h (their old places stay, so column indices still hold)."""
    R, n_dst = case["R"], case["n_dst"]
    keep = list(keep)
    rp, col, val = case["row_ptr"], case["col"], case["val"]
    lens, cols, vals = [], [], []
    for v in keep:
        for q in range(v * R, v * R + R):
            lens.append(rp[q + 1] - rp[q])
            cols.append(col[rp[q]:rp[q + 1]])
            vals.append(val[rp[q]:rp[q + 1]])
    m = len(keep)
    h = np.concatenate([case["h"][keep], case["h"]], axis=0)               # new destinations on top, every old row m places lower
    return dict(case, n_dst=m, n_src=h.shape[0], row_ptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                col=(np.concatenate(cols).astype(np.int64) + m).astype(np.int32), val=np.concatenate(vals).astype(np.float32), h=h,
                d_out=case["d_out"][keep])


# ---- translate_relations ------------------------------------------------------------------------------------------------------------
def translate_relations_ref(bipartite, top_k):
    """dense float64 [N, N] by a double loop: S[v, u] = sum_a B[v, a] B[u, a] for u != v, each row cut to its top_k largest entries, ties
    to the smaller id"""
    B = np.asarray(bipartite, np.float64)
    N = B.shape[0]
    out = np.zeros((N, N))
    for v in range(N):
        cand = []
        for u in range(N):
            if u == v:
                continue
            w = float(np.dot(B[v], B[u]))
            if w != 0.0:
                cand.append((-w, u))
        for negw, u in sorted(cand)[:top_k]:
            out[v, u] = -negw
    return out


# ---- the typed sampling chain --------------------------------------------------------------------------------------------------------
def layer_seed(seed, k):
    return (int(seed) + 0x9E3779B97F4A7C15 * (k + 1)) & (2 ** 64 - 1)


def sample_typed_blocks_ref(graphs, n_rows, seeds, fanouts, seed):
    """graphs: [(row_ptr, col)] per relation.  Per layer, innermost first: one neighbour sample per relation seeded layer_seed(seed, k R
    + r), ONE frontier over the concatenated neighbours, ONE block CSR over (destination, relation) rows.  Returns, outermost first,
    dicts of n_dst, n_src, src, row_ptr, col, val."""
    R = len(graphs)
    dst = np.asarray(seeds, np.int64)
    out = []
    for k in reversed(range(len(fanouts))):
        f = fanouts[k]
        drawn = [sage_ref.neighbor_sample_ref(rp, c, n_rows, dst, f, layer_seed(seed, k * R + r)) for r, (rp, c) in enumerate(graphs)]
        nbr = np.concatenate([d[0] for d in drawn], axis=1)
        cnt = np.stack([d[1] for d in drawn], axis=1)
        src, counts, local = sage_ref.frontier_build_ref(dst, nbr)
        n = dst.size
        rp, col, val = sage_ref.block_csr_ref(cnt.reshape(n * R), local.reshape(n * R, f), None, False, int(counts[0]) * R)
        out.append(dict(n_dst=int(counts[0]), n_src=int(counts[1]), src=src[:counts[1]], row_ptr=rp[:int(counts[0]) * R + 1], col=col, val=val))
        dst = src
    return out[::-1]


def block_dense(b, R):
    """float64 [n_dst, R, n_src] of a block dict"""
    A = np.zeros((b["n_dst"] * R, b["n_src"]))
    for q in range(b["n_dst"] * R):
        for k in range(int(b["row_ptr"][q]), int(b["row_ptr"][q + 1])):
            A[q, b["col"][k]] += float(b["val"][k])
    return A.reshape(b["n_dst"], R, b["n_src"])


# ---- one train step -------------------------------------------------------------------------------------------------------------------
def net_forward(params, x, dense_blocks, dtype):
    """(z, h0) of one IntentNet on torch tensors: x the gathered feature rows [n_src0, F], dense_blocks [n_dst, R, n_src] per layer"""
    t = lambda a: a if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a), dtype=dtype)
    h0 = t(x) @ params["proj_kernel"] + params["proj_bias"]
    h0.retain_grad()
    h = h0
    for (W, theta), A in zip(params["convs"], dense_blocks):
        A = t(A)
        agg = torch.einsum("vrs,sd->vrd", A, h)
        h = conv_torch(h[:A.shape[0]], agg, W, theta, 1)
    n = len(params["dnn"])
    for j, (K, b) in enumerate(params["dnn"]):
        h = h @ K + b
        if j < n - 1:
            h = torch.relu(h)
    return h, h0


def params_to(params, dtype):
    """a net's parameters (numpy) as torch leaves of dtype"""
    leaf = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
    return dict(proj_kernel=leaf(params["proj_kernel"]), proj_bias=leaf(params["proj_bias"]),
                convs=[(leaf(W), leaf(th)) for W, th in params["convs"]], dnn=[(leaf(K), leaf(b)) for K, b in params["dnn"]])


def flat_params(p):
    return [p["proj_kernel"], p["proj_bias"]] + [x for c in p["convs"] for x in c] + [x for c in p["dnn"] for x in c]


def train_step_ref(case, dtype=torch.float64):
    """(loss, [gradients of the user net's parameters], [the item net's], d_h0 user, d_h0 item, the hinge arguments of the kept pairs)
    of one IntentGC.train_step on the case's blocks: loss = mean_i sum_j max(0, margin - z_u[i] . z_pos[i] + z_u[i] . z_neg[j]) over the
    negatives j whose id differs from row i's positive."""
    pu, pi = params_to(case["user_params"], dtype), params_to(case["item_params"], dtype)
    z_u, h0_u = net_forward(pu, case["user_x"], case["user_dense"], dtype)
    z_i, h0_i = net_forward(pi, case["item_x"], case["item_dense"], dtype)
    B = len(case["users"])
    pos, neg = z_i[:B], z_i[B:]
    s_pos = (z_u * pos).sum(dim=1)
    s_neg = z_u @ neg.T
    keep = torch.tensor(np.asarray(case["pos_items"])[:, None] != np.asarray(case["neg_items"])[None, :])
    arg = case["margin"] - s_pos[:, None] + s_neg
    loss = (torch.relu(arg) * keep).sum() / B
    loss.backward()
    g = lambda p: [x.grad.detach() if x.grad is not None else torch.zeros_like(x) for x in flat_params(p)]
    return loss.detach(), g(pu), g(pi), h0_u.grad.detach(), h0_i.grad.detach(), arg.detach()[keep]


def _random_relation(r, n, deg):
    import scipy.sparse as sp
    rows = np.repeat(np.arange(n), deg)
    cols = np.concatenate([np.sort(r.choice(n, size=d, replace=False)) for d in deg])
    return sp.csr_matrix((np.ones(rows.size, np.float32), (rows, cols)), shape=(n, n))


MODEL_SEED = 3


def make_model_case(seed=MODEL_SEED):
    """a small dual network and one batch, everything generated on the host: two relations per side, its parameters, the sampled blocks
    by the restated chain (the GPU test checks that the model's own blocks are these)"""
    r = np.random.RandomState(seed)
    Nu, Ni, Fu, Fi, D, Lf, units, fanouts = 40, 50, 8, 12, 16, 3, (16, 8), (3, 2)
    rel_u = [_random_relation(r, Nu, r.randint(0, 6, size=Nu)) for _ in range(2)]
    rel_i = [_random_relation(r, Ni, r.randint(0, 6, size=Ni)) for _ in range(2)]
    feat_u = r.standard_normal((Nu, Fu)).astype(np.float32)
    feat_i = r.standard_normal((Ni, Fi)).astype(np.float32)

    def net(F, R):
        dnn, d = [], D
        for n in units:
            dnn.append(((r.standard_normal((d, n)) / np.sqrt(d)).astype(np.float32), (0.1 * r.standard_normal(n)).astype(np.float32)))
            d = n
        convs = []
        for _ in fanouts:
            W = (0.3 * r.standard_normal((Lf, R + 1))).astype(np.float32)
            W[:, 0] += 1.0 / Lf
            convs.append((W, (1.0 + 0.3 * r.standard_normal(Lf)).astype(np.float32)))
        return dict(proj_kernel=(r.standard_normal((F, D)) / np.sqrt(F)).astype(np.float32),
                    proj_bias=(0.1 * r.standard_normal(D)).astype(np.float32), convs=convs, dnn=dnn)

    users = np.asarray([3, 17, 17, 0, 39, 8], dtype=np.int64)              # a repeated user
    pos_items = np.asarray([5, 49, 12, 12, 30, 7], dtype=np.int64)
    neg_items = np.asarray([12, 1, 44, 30, 20], dtype=np.int64)            # two of them are some row's positive
    case = dict(Nu=Nu, Ni=Ni, D=D, L=Lf, units=units, fanouts=fanouts, margin=0.2, sample_seed=11, rel_u=rel_u, rel_i=rel_i,
                feat_u=feat_u, feat_i=feat_i, user_params=net(Fu, 2), item_params=net(Fi, 2), users=users, pos_items=pos_items,
                neg_items=neg_items)
    for side, rel, N, ids, feat in (("user", rel_u, Nu, users, feat_u), ("item", rel_i, Ni, np.concatenate([pos_items, neg_items]), feat_i)):
        graphs = [(m.indptr.astype(np.int64), m.indices.astype(np.int32)) for m in rel]
        blocks = sample_typed_blocks_ref(graphs, N, ids, list(fanouts), case["sample_seed"])
        case[side + "_blocks"] = blocks
        case[side + "_dense"] = [block_dense(b, 2) for b in blocks]
        case[side + "_x"] = feat[blocks[0]["src"]]
    return case
