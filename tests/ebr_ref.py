"""Float64 restatement of EBR's training loss (include/dr_hotpath.h, "Margin ranking loss"): the in-batch / shared-negative triplet loss
over cosine or dot-product scores with optional hard-negative mining, its hand-written gradients with respect to the raw rows, a plain
torch composition for autograd, and the random cases of the GPU test with their rounding bounds.  Plain torch on the CPU; shared by
tests/test_ebr_cpu.py and tests/test_gpu_ebr.py.

Rounding bounds, U = 2^-24, first order in U (evaluated on the float64 results; none is read off the kernel).  RR is the relative error
of an inverse norm r = (max(sum x^2, eps))^(-1/2): the sum of D squares in any order, fused or not, is off by at most (D + 1) U
relatively, the power -1/2 halves that, and 1 / sqrt itself enters as the allowance A_RSQ measured on the CPU (below) with the project's
margin of 4;  RR = (D + 1) U / 2 + 4 A_RSQ for the cosine, 0 for the dot product (r = 1 exactly).
  scores     sb_ij = (D + 1) U sum_d |q^_d n^_jd| + (2 RR + 2 U) |s_ij|       the chain of D products; two inverse norms, two multiplies
  pos_score  tb_i, the same form
  h_ij       hb_ij = tb_i + sb_ij + U |margin - t_i| + U |h_ij|               (margin - t) + s: two roundings
  row_loss   a term goes through at most n_i + 10 additions (its lane's chain over the n_i active columns, the two adds across the four
             lanes, at most 8 segments):   lb_i = w_i (sum_act hb_ij + (n_i + 10) U sum_act h_ij) + U |loss_i|
  a_ij = row_scale w_i carries one rounding.  With NA = n_i + 12 (the additions, a's rounding, the product's):
  c_i        cb_i = NA U c_i                  e_i   eb_i = sum_j a_ij sb_ij + NA U sum_j a_ij |s_ij|
  V_i = sum_j a_ij n^_j (the second product: the weight a_ij r_nj, then the chain):   Vb = (RR + NA U) Vabs,  Vabs = sum_j a_ij |n^_j|
  coef_i = pi_q (e_i - c_i t_i)               kb_i = pi_q (eb_i + cb_i |t_i| + c_i tb_i + 2 U (|e_i| + |c_i t_i|))
  d_q  = r_q (V - c p^ - coef q^):   r_q [ Vb + (cb + c (RR + 2 U)) |p^| + (kb + |coef| (RR + 2 U)) |q^| + (RR + 3 U) (Vabs + c |p^| + |coef| |q^|) ]
  d_pos = -c r_p (q^ - pi_p t p^):   r_p [ c ((RR + 2 U) Mp + pi_p tb |p^|) + (cb + c (RR + 2 U)) Mp ],  Mp = |q^| + pi_p |t| |p^|
  d_neg = r_n (W - pi_n f n^), W_j = sum_i a_ij q^_i, f_j = sum_i a_ij s_ij, over the n_j active rows of the column in NC = n_j + chunks + 6
             additions and roundings:   fb_j = sum_i a_ij sb_ij + NC U sum_i a_ij |s_ij|,   Wb = (RR + NC U) Wabs,
             r_n [ Wb + pi_n (fb + |f| (RR + 2 U)) |n^| + (RR + 3 U) (Wabs + pi_n |f| |n^|) ]
The hinge and the selection are discontinuous: a case is usable when the float64 reference decides every one of them with room --
|h_ij| > 4 hb_ij at every kept entry and, in hard mode, a gap between a row's k-th and (k + 1)-th kept score above 4 times the sum of
their bounds.  case() takes the first seed from a fixed base for which that holds (tests/test_ebr_cpu.py asserts it)."""
import functools
import math

import numpy as np
import torch

DD = torch.float64
U = 2.0 ** -24
EPS = 1e-12
MARGIN4 = 4.0
TILE, COL_GROUP, ROW_CHUNK, SPLIT_TILES, MAX_HARD = 64, 128, 128, 128, 8     # checked against ops in both test files


def _measure_rsqrt():
    """largest relative error of fp32 1 / sqrt(x) against float64 over 2^16 + 1 evenly spaced points of [2^-4, 2^4]"""
    x = torch.linspace(2.0 ** -4, 2.0 ** 4, 2 ** 16 + 1, dtype=torch.float32)
    r32, r64 = (1.0 / torch.sqrt(x)).double(), 1.0 / torch.sqrt(x.double())
    return float(((r32 - r64).abs() / r64).max())


A_RSQ = _measure_rsqrt()


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def normalise(x, metric, ok):
    """(x^ with the rows outside `ok` zeroed, r, pi): x^ = x r, r = (max(sum x^2, eps))^(-1/2), pi = [sum x^2 >= eps]; dot: r = 1, pi = 0"""
    x0 = torch.where(ok[:, None], x, torch.zeros_like(x))
    if metric == "dot":
        return x0, torch.ones(x.shape[0], dtype=x.dtype), torch.zeros(x.shape[0], dtype=x.dtype)
    ss = (x0 * x0).sum(-1)
    r = torch.clamp_min(ss, EPS) ** -0.5
    return x0 * r[:, None], r, (ss >= EPS).to(x.dtype)


def keep_mask(B, S, pos_ids, neg_ids, in_batch):
    valid = torch.ones(B, dtype=torch.bool) if pos_ids is None else pos_ids >= 0
    keep = valid[:, None].expand(B, S).clone()
    if in_batch:
        keep &= ~torch.eye(B, dtype=torch.bool)
    if neg_ids is not None:
        keep &= (neg_ids >= 0)[None, :]
    if pos_ids is not None and neg_ids is not None:
        keep &= neg_ids[None, :] != pos_ids[:, None]
    return valid, keep


def select(s, keep, num_hard):
    """(member [B, S], hard_idx [B, num_hard] or None): the num_hard kept columns of largest score, ties to the smaller j"""
    if num_hard == 0:
        return keep.clone(), None
    B, S = s.shape
    masked = s.masked_fill(~keep, -math.inf)
    order = torch.sort(masked, dim=1, descending=True, stable=True).indices          # stable: equal scores keep the column order
    k = min(num_hard, S)
    idx = torch.full((B, num_hard), -1, dtype=torch.int64)
    idx[:, :k] = order[:, :k]
    idx[:, :k][~torch.gather(keep, 1, order[:, :k])] = -1
    member = torch.zeros(B, S, dtype=torch.bool)
    for c in range(k):
        ok = idx[:, c] >= 0
        member[torch.arange(B)[ok], idx[ok, c]] = True
    return member, idx


def forward(q, pos, neg, pos_ids=None, neg_ids=None, w=None, margin=0.2, metric="cosine", in_batch=False, num_hard=0):
    """dict of the forward's results; neg is pos itself for in_batch"""
    B, S = q.shape[0], neg.shape[0]
    valid, keep = keep_mask(B, S, pos_ids, neg_ids, in_batch)
    nok = torch.ones(S, dtype=torch.bool) if neg_ids is None else neg_ids >= 0
    qh, rq, piq = normalise(q, metric, valid)
    ph, rp, pip = normalise(pos, metric, valid)
    nh, rn, pin = normalise(neg, metric, nok)
    t = (qh * ph).sum(-1)
    s = qh @ nh.T
    member, hard_idx = select(s, keep, num_hard)
    h = (margin - t)[:, None] + s
    act = member & (h > 0)
    wv = torch.ones(B, dtype=q.dtype) if w is None else w.to(q.dtype)
    hinge = torch.where(act, h, torch.zeros_like(h))
    return dict(valid=valid, keep=keep, nok=nok, qh=qh, ph=ph, nh=nh, rq=rq, rp=rp, rn=rn, piq=piq, pip=pip, pin=pin, t=t, s=s,
                member=member, hard_idx=hard_idx, h=h, act=act, w=wv, loss=wv * hinge.sum(-1), active=act.sum(-1))


def hand_grads(q, pos, neg, pos_ids=None, neg_ids=None, w=None, margin=0.2, metric="cosine", in_batch=False, num_hard=0, row_scale=1.0):
    """the closed forms of the header: the gradients of row_scale * sum_i loss_i with respect to the raw rows"""
    f = forward(q, pos, neg, pos_ids, neg_ids, w, margin, metric, in_batch, num_hard)
    a = (row_scale * f["w"])[:, None] * f["act"].to(q.dtype)
    s0 = torch.where(f["keep"], f["s"], torch.zeros_like(f["s"]))
    c, e, fj = a.sum(-1), (a * s0).sum(-1), (a * s0).sum(0)
    qh, ph, nh, t = f["qh"], f["ph"], f["nh"], f["t"]
    V, W = a @ nh, a.T @ qh
    coef = f["piq"] * (e - c * t)
    d_q = f["rq"][:, None] * (V - c[:, None] * ph - coef[:, None] * qh)
    d_pos = -(c * f["rp"])[:, None] * (qh - (f["pip"] * t)[:, None] * ph)
    d_neg = f["rn"][:, None] * (W - (f["pin"] * fj)[:, None] * nh)
    zero = torch.zeros_like(d_q)
    d_q, d_pos = torch.where(f["valid"][:, None], d_q, zero), torch.where(f["valid"][:, None], d_pos, zero)
    d_neg = torch.where(f["nok"][:, None], d_neg, torch.zeros_like(d_neg))
    out = dict(f)
    out.update(a=a, s0=s0, c=c, e=e, f=fj, V=V, W=W, coef=coef, d_q=d_q, d_pos=d_pos, d_neg=d_neg)
    return out


def composition(q, pos, neg, pos_ids=None, neg_ids=None, w=None, margin=0.2, metric="cosine", in_batch=False, num_hard=0):
    """the loss rows as the plain torch composition autograd can differentiate: normalise -> matmul -> mask -> optional topk -> relu"""
    B, S = q.shape[0], neg.shape[0]
    valid, keep = keep_mask(B, S, pos_ids, neg_ids, in_batch)
    nok = torch.ones(S, dtype=torch.bool) if neg_ids is None else neg_ids >= 0

    def unit(x, ok):
        x = torch.where(ok[:, None], x, torch.zeros_like(x))
        if metric == "dot":
            return x
        return x * torch.clamp_min((x * x).sum(-1, keepdim=True), EPS) ** -0.5

    qh, ph, nh = unit(q, valid), unit(pos, valid), unit(neg, nok)
    t = (qh * ph).sum(-1)
    s = (qh @ nh.T).masked_fill(~keep, -math.inf)
    if num_hard > 0:
        # top-k as a stable sort: torch.topk leaves the choice among equal scores open (a zero row ties with everything), the
        # definition gives it to the smaller column
        s = torch.sort(s, dim=1, descending=True, stable=True).values[:, :min(num_hard, S)]
    hinge = torch.relu((margin - t)[:, None] + s)
    wv = torch.ones(B, dtype=q.dtype) if w is None else w.to(q.dtype)
    return torch.where(valid, wv * hinge.sum(-1), torch.zeros_like(t))


# ---- the rounding bounds of the header, from the float64 results ---------------------------------------------------------------------------
def bounds(h, D, margin, metric, chunks):
    RR = 0.5 * (D + 1) * U + MARGIN4 * A_RSQ if metric == "cosine" else 0.0
    qa, pa, na = h["qh"].abs(), h["ph"].abs(), h["nh"].abs()
    kd = h["keep"].to(DD)
    s0, t, a, c, e = h["s0"], h["t"], h["a"], h["c"], h["e"]
    sb = ((D + 1) * U * (qa @ na.T) + (2 * RR + 2 * U) * s0.abs()) * kd
    tb = (D + 1) * U * (qa * pa).sum(-1) + (2 * RR + 2 * U) * t.abs()
    h0 = torch.where(h["keep"], h["h"], torch.zeros_like(h["h"]))
    hb = (tb[:, None] + sb + U * (margin - t).abs()[:, None] + U * h0.abs()) * kd
    act = h["act"].to(DD)
    n_i = act.sum(-1)
    lb = h["w"] * ((act * hb).sum(-1) + (n_i + 10) * U * (act * h0).sum(-1)) + U * h["loss"].abs()
    NA = n_i + 12
    cb = NA * U * c
    eb = (a * sb).sum(-1) + NA * U * (a * s0.abs()).sum(-1)
    Vabs = a @ na
    Vb = (RR + NA * U)[:, None] * Vabs
    kb = h["piq"] * (eb + cb * t.abs() + c * tb + 2 * U * (e.abs() + (c * t).abs()))
    coef = h["coef"].abs()
    rq, rp, rn = h["rq"], h["rp"], h["rn"]
    valid, nok = h["valid"].to(DD), h["nok"].to(DD)
    dqb = rq[:, None] * (Vb + (cb + c * (RR + 2 * U))[:, None] * pa + (kb + coef * (RR + 2 * U))[:, None] * qa
                         + (RR + 3 * U) * (Vabs + c[:, None] * pa + coef[:, None] * qa)) * valid[:, None]
    Mp = qa + (h["pip"] * t.abs())[:, None] * pa
    dpb = rp[:, None] * (c[:, None] * ((RR + 2 * U) * Mp + (h["pip"] * tb)[:, None] * pa) + (cb + c * (RR + 2 * U))[:, None] * Mp) * valid[:, None]
    n_j = act.sum(0)
    NC = n_j + chunks + 6
    fb = (a * sb).sum(0) + NC * U * (a * s0.abs()).sum(0)
    Wabs = a.T @ qa
    Wb = (RR + NC * U)[:, None] * Wabs
    fj = h["f"].abs()
    dnb = rn[:, None] * (Wb + (h["pin"] * (fb + fj * (RR + 2 * U)))[:, None] * na
                         + (RR + 3 * U) * (Wabs + (h["pin"] * fj)[:, None] * na)) * nok[:, None]
    return dict(b_s=sb, b_t=tb * valid, b_h=hb, b_loss=lb, b_dq=dqb, b_dpos=dpb, b_dneg=dnb)


def decided_with_room(h, b, num_hard):
    """the input conditions of a random case: every hinge and every selection decided by more than 4 times its bound"""
    keep = h["keep"]
    if not bool((h["h"].abs()[keep] > MARGIN4 * b["b_h"][keep]).all()):
        return False
    if num_hard > 0:
        masked = h["s"].masked_fill(~keep, -math.inf)
        val, order = torch.sort(masked, dim=1, descending=True, stable=True)
        sbo = torch.gather(b["b_s"], 1, order)
        for k in range(1, min(num_hard, masked.shape[1] - 1) + 1):           # the k-th against the (k + 1)-th, for every list length used
            both = torch.isfinite(val[:, k - 1]) & torch.isfinite(val[:, k])
            gap = val[:, k - 1] - val[:, k]
            if not bool((gap[both] > MARGIN4 * (sbo[:, k - 1] + sbo[:, k])[both]).all()):
                return False
    return True


# ---- the cases of the GPU test ---------------------------------------------------------------------------------------------------------------
DS, SS, BS = (4, 20, 64, 100, 256), (1, 63, 64, 200), (1, 3, 257)
MERGE = (20, 2 * COL_GROUP + 1, 2 * ROW_CHUNK + 1)                  # three column segments, three row chunks: crosses both merges
SHAPES = [(D, 65, B) for D in DS for B in BS] + [(64, S, B) for S in SS for B in BS] + [MERGE]       # (D, S, B), separate negatives
IN_BATCH = [(64, B, B) for B in (1, 3, 64, 257)]
OPTS = {"all": (True, True, "cosine"), "plain": (False, False, "dot")}          # (sample_weight, ids, metric)
HARD = (0, 1, 3, 8)
SEED_BASE, SEED_TRIES = 4000, 64
RANDOM_MARGIN = 33.0 / 128.0


def _lattice_rows(n, L, D, C, rng, permute):
    """n unit rows whose first C coordinates lie on the L-point lattice b_k = (2 k + 1 - L) / (2 L) (step 1 / L inside (-1/2, 1/2); per
    coordinate a permutation of it when permute, else independent draws) and whose other coordinates are a random direction scaled to
    make the norm 1"""
    k = np.stack([rng.permutation(L)[:n] if permute else rng.integers(0, L, size=n) for _ in range(C)], axis=1)
    b = (2.0 * k + 1.0 - L) / (2.0 * L)
    v = rng.standard_normal((n, D - C))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([b, np.sqrt(1.0 - (b * b).sum(1, keepdims=True)) * v], axis=1)


def _random_rows(shape, in_batch, rng):
    """The random cases' q, pos and neg.  Gaussian rows cannot be used: with the worst-case bounds above, 257 x 257 hinges and 257 x 8
    selections are never all decided with room.  So the scores are given a spectrum: the negatives are unit rows whose first C = min(3,
    D - 1) coordinates are permutations of an S-point lattice of step 1 / S, a query is (nearly) a signed unit vector of one of those
    coordinates plus a random direction of length eta = 1 / (32 S) in the others, and the positives lie on the same lattice (in-batch
    they ARE the negatives).  Then s_ij = +-b_j + O(eta) and h_ij = margin +- (k_j - k_i) / S + O(eta): with RANDOM_MARGIN = 33 / 128,
    margin * S is at least 0.23 from an integer for every S used, so |h_ij| >= 0.16 / S, and a row's scores are 0.9 / S apart --
    both far above the bounds.  Which coordinate, which sign, the permutations and the directions are the seed's."""
    D, S, B = shape
    C = min(3, D - 1)
    neg = _lattice_rows(S, S, D, C, rng, True)
    pos = neg if in_batch else _lattice_rows(B, S, D, C, rng, False)
    eta = 1.0 / (32.0 * S)
    u = rng.standard_normal((B, D - C))
    u *= eta / np.linalg.norm(u, axis=1, keepdims=True)
    q = np.zeros((B, D))
    q[np.arange(B), rng.integers(0, C, size=B)] = rng.choice([-1.0, 1.0], size=B) * math.sqrt(1.0 - eta * eta)
    q[:, C:] = u
    f = lambda x: torch.from_numpy(x.astype(np.float32)).to(DD)                                # noqa: E731
    return f(q), f(pos).clone(), None if in_batch else f(neg)


def inputs(shape, in_batch, use_ids, rng, integer=False):
    """q, pos, neg (None for in_batch), pos_ids, neg_ids as float64 / int64 on the CPU.  Every case carries what its size allows of: a
    NaN-filled padding row (row 1), a padding negative id (column S // 2) on a NaN row, and a document id that occurs twice among
    the negatives and is the positive of row 0."""
    D, S, B = shape
    if integer:
        t = lambda *s: torch.from_numpy(rng.integers(-3, 4, size=s)).to(DD)                    # noqa: E731
        q, pos = t(B, D), t(B, D)
        neg = None if in_batch else t(S, D)
    else:
        q, pos, neg = _random_rows(shape, in_batch, rng)
    pos_ids = neg_ids = None
    if use_ids:
        pos_ids = torch.arange(B, dtype=torch.int64) * 3 + 5
        if in_batch:
            if B >= 3:
                pos_ids[B - 1] = pos_ids[0]                                                    # the same document twice in the batch
        else:
            neg_ids = torch.arange(S, dtype=torch.int64) * 3 + 6                               # no id of a positive ...
            neg_ids[0] = pos_ids[0]                                                            # ... but that of row 0, twice where S allows
            if S >= 4:
                neg_ids[S - 1] = pos_ids[0]
            if S >= 2:
                neg_ids[S // 2] = -1
                neg[S // 2] = math.nan                                                         # never read
        if B >= 3:
            pos_ids[1] = -1
            q[1] = math.nan                                                                    # a padding row holding NaN
            pos[1] = math.nan                                                                  # (in-batch: its column carries id -1)
    return q, pos, neg, pos_ids, neg_ids


def build(shape, in_batch, opt, num_hard, seed, chunks):
    use_w, use_ids, metric = OPTS[opt]
    D, S, B = shape
    rng = np.random.default_rng(seed)
    q, pos, neg, pos_ids, neg_ids = inputs(shape, in_batch, use_ids, rng)
    w = torch.from_numpy((rng.random(B) + 0.5).astype(np.float32)).to(DD) if use_w else None
    scale = float(np.float32(1.0 / B))
    n_eff, nid_eff = (pos, pos_ids) if in_batch else (neg, neg_ids)
    h = hand_grads(q, pos, n_eff, pos_ids, nid_eff, w, RANDOM_MARGIN, metric, in_batch, num_hard, scale)
    b = bounds(h, D, RANDOM_MARGIN, metric, chunks)
    return dict(q=q, pos=pos, neg=neg, pos_ids=pos_ids, neg_ids=neg_ids, w=w, scale=scale, metric=metric, margin=RANDOM_MARGIN,
                num_hard=num_hard, in_batch=in_batch, ref=h, bounds=b, seed=seed, ok=decided_with_room(h, b, num_hard))


def plan_chunks(B, S):
    """the number of row chunks of the column sweep, restated from the header (checked against ops in tests/test_ebr_cpu.py)"""
    row_tiles, col_tiles = -(-B // TILE), -(-S // TILE)
    want = max(1, -(-512 // col_tiles))
    chunks = min(64, want, max(1, -(-B // ROW_CHUNK)))
    ct = max(1, -(-row_tiles // chunks))
    return max(1, -(-row_tiles // ct))


def plan_segments(S):
    col_tiles = -(-S // TILE)
    nseg = min(8, -(-S // COL_GROUP))
    seg_tiles = -(-col_tiles // nseg)
    return -(-col_tiles // seg_tiles)


@functools.lru_cache(maxsize=None)
def case(shape, in_batch, opt, num_hard):
    """the random case: the first seed from SEED_BASE + 100 * (its place in the list) whose inputs the reference decides with room"""
    shapes = IN_BATCH if in_batch else SHAPES
    base = SEED_BASE + 100 * (shapes.index(shape) + (len(SHAPES) if in_batch else 0))
    chunks = plan_chunks(shape[2], shape[1])
    for seed in range(base, base + SEED_TRIES):
        c = build(shape, in_batch, opt, num_hard, seed, chunks)
        if c["ok"]:
            return c
    raise AssertionError("no seed in [%d, %d) decides %r with room" % (base, base + SEED_TRIES, (shape, in_batch, opt, num_hard)))
