"""A restatement of DIEN's recurrences (Zhou et al., AAAI 2019) in plain torch, written from the paper and from the contract in
include/dr_hotpath.h, for the tests of csrc/dien.hip.  Every function computes in the dtype of its inputs (float64 for the reference,
float32 for the reference's own rounding error).

    step t < len[b]:  g = h_{t-1} U;  u = sigmoid(xp_u + g_u);  r = sigmoid(xp_r + g_r);  c = tanh(xp_c + r g_c);  u' = att[b, t] u
                      h_t = (1 - u') h_{t-1} + u' c;  hs[b, t] = h_t
    step t >= len[b]: h_t = h_{t-1};  hs[b, t] = 0

`Arith` carries the three things an implementation is free to choose: how a matrix product is summed, and how the two gate functions
are evaluated.  ALT is a deliberately different fp32 association (k-chunks of 4 added last chunk first, exp2-based gates)."""
import functools
import math

import numpy as np
import torch

DD = torch.float64
U24 = 2.0 ** -24


class Arith:
    def mm(self, a, b):
        return a @ b

    def sigmoid(self, x):
        return torch.sigmoid(x)

    def tanh(self, x):
        return torch.tanh(x)

    def rowsum(self, x):
        return x.sum(dim=1)


class AltArith(Arith):
    """k-chunks of 4 summed from the last chunk to the first; sigmoid and tanh through exp2; row sums from the last column to the first"""

    def mm(self, a, b):
        K = a.shape[1]
        out = torch.zeros((a.shape[0], b.shape[1]), dtype=a.dtype)
        for k in range((K - 1) // 4 * 4, -1, -4):
            part = torch.zeros_like(out)
            for kk in range(min(k + 4, K) - 1, k - 1, -1):
                part = part + a[:, kk:kk + 1] * b[kk:kk + 1, :]
            out = out + part
        return out

    def sigmoid(self, x):
        return 1.0 / (1.0 + torch.exp2(-x * x.new_tensor(math.log2(math.e))))

    def tanh(self, x):
        return 2.0 * self.sigmoid(2.0 * x) - 1.0

    def rowsum(self, x):
        out = torch.zeros(x.shape[0], dtype=x.dtype)
        for j in range(x.shape[1] - 1, -1, -1):
            out = out + x[:, j]
        return out


PLAIN, ALT = Arith(), AltArith()


def _lens(lengths, B, T):
    return torch.full((B,), T, dtype=torch.int64) if lengths is None else lengths.to(torch.int64).clamp(0, T)


def _gates(xp_t, h, U, att_t, ar):
    H = U.shape[0]
    g = ar.mm(h, U)
    u = ar.sigmoid(xp_t[:, :H] + g[:, :H])
    r = ar.sigmoid(xp_t[:, H:2 * H] + g[:, H:2 * H])
    c = ar.tanh(xp_t[:, 2 * H:] + r * g[:, 2 * H:])
    up = u if att_t is None else att_t[:, None] * u
    return g, u, r, c, up


def forward(xp, U, h0=None, lengths=None, att=None, ar=PLAIN):
    """(hs [B, T, H], h_last [B, H])"""
    B, T, H = xp.shape[0], xp.shape[1], U.shape[0]
    lens = _lens(lengths, B, T)
    h = torch.zeros((B, H), dtype=xp.dtype) if h0 is None else h0
    hs = []
    for t in range(T):
        on = (t < lens)[:, None]
        _, _, _, c, up = _gates(xp[:, t], h, U, None if att is None else att[:, t], ar)
        h = torch.where(on, (1 - up) * h + up * c, h)
        hs.append(torch.where(on, h, torch.zeros_like(h)))
    return torch.stack(hs, dim=1), h


def backward(xp, U, h0, lengths, att, d_hs=None, d_h_last=None, ar=PLAIN):
    """(d_xp [B, T, 3H], dU [H, 3H], d_h0 [B, H], d_att [B, T] | None), written out by hand: the forward's states are stored, the gates
    recomputed, t runs downward"""
    B, T, H = xp.shape[0], xp.shape[1], U.shape[0]
    lens = _lens(lengths, B, T)
    h = torch.zeros((B, H), dtype=xp.dtype) if h0 is None else h0
    states = [h]
    for t in range(T):
        on = (t < lens)[:, None]
        _, _, _, c, up = _gates(xp[:, t], h, U, None if att is None else att[:, t], ar)
        h = torch.where(on, (1 - up) * h + up * c, h)
        states.append(h)
    dh = torch.zeros((B, H), dtype=xp.dtype) if d_h_last is None else d_h_last.clone()
    d_xp = torch.zeros_like(xp)
    dU = torch.zeros_like(U)
    d_att = None if att is None else torch.zeros((B, T), dtype=xp.dtype)
    zero = torch.zeros((B, H), dtype=xp.dtype)
    for t in range(T - 1, -1, -1):
        on = (t < lens)[:, None]
        hp = states[t]
        g, u, r, c, up = _gates(xp[:, t], hp, U, None if att is None else att[:, t], ar)
        d = dh if d_hs is None else dh + d_hs[:, t]
        dc, dup, carry = d * up, d * (c - hp), d * (1 - up)
        du = dup
        if att is not None:
            d_att[:, t] = torch.where(on[:, 0], ar.rowsum(dup * u), zero[:, 0])
            du = att[:, t][:, None] * dup
        dpc = dc * (1 - c * c)
        dpu = du * u * (1 - u)
        dpr = dpc * g[:, 2 * H:] * r * (1 - r)
        dxp_t = torch.where(on, torch.cat([dpu, dpr, dpc], dim=1), torch.zeros((B, 3 * H), dtype=xp.dtype))
        dg = torch.where(on, torch.cat([dpu, dpr, dpc * r], dim=1), torch.zeros((B, 3 * H), dtype=xp.dtype))
        d_xp[:, t] = dxp_t
        dU = dU + ar.mm(torch.where(on, hp, zero).t().contiguous(), dg)
        dh = torch.where(on, carry + ar.mm(dg, U.t().contiguous()), dh)
    return d_xp, dU, dh, d_att


def attention(hs, q, lengths=None):
    """a [B, T]: the softmax over t < len[b] of <hs[b, t], q[b]>, 0 at masked steps"""
    B, T, _ = hs.shape
    lens = _lens(lengths, B, T)
    on = torch.arange(T)[None, :] < lens[:, None]
    s = (torch.where(on[:, :, None], hs, torch.zeros_like(hs)) * q[:, None, :]).sum(-1)
    s = torch.where(on, s, torch.full_like(s, -float("inf")))
    m = torch.where(lens > 0, s.max(dim=1).values, torch.zeros(B, dtype=hs.dtype))
    e = torch.where(on, torch.exp(s - m[:, None]), torch.zeros_like(s))
    return e / torch.where(lens > 0, e.sum(dim=1), torch.ones(B, dtype=hs.dtype))[:, None]


def attention_backward(hs, q, lengths, d_a):
    B, T, _ = hs.shape
    lens = _lens(lengths, B, T)
    on = (torch.arange(T)[None, :] < lens[:, None])
    a = attention(hs, q, lengths)
    ds = a * (torch.where(on, d_a, torch.zeros_like(d_a)) - (a * torch.where(on, d_a, torch.zeros_like(d_a))).sum(1, keepdim=True))
    hz = torch.where(on[:, :, None], hs, torch.zeros_like(hs))
    return ds[:, :, None] * q[:, None, :], (ds[:, :, None] * hz).sum(1)


# ---- the seeded cases of tests/test_gpu_dien.py: ((B, T, H), with_att, seed) -----------------------------------------------------------
SHAPES = [(1, 1, 4), (3, 5, 20), (17, 7, 64), (33, 12, 128), (70, 33, 32), (8200, 2, 4), (5, 200, 16)]
CASES = [(s, w, 100 + 2 * i + w) for i, s in enumerate(SHAPES) for w in (0, 1)]


def draw(shape, with_att, seed):
    """xp ~ N(0, 1), U ~ N(0, 1 / H), h0 ~ N(0, 1 / 4), att ~ U(0, 1), d_hs, d_h_last ~ N(0, 1), q ~ N(0, 1), random lengths; with
    B >= 3 the examples 0, 1, 2 have the lengths T, 1, 0, and with B >= T + 4 every length from 0 to T occurs.  float32 values held in
    float64."""
    B, T, H = shape
    rng = np.random.default_rng(seed)
    f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).double()                   # noqa: E731
    c = dict(xp=f(rng.standard_normal((B, T, 3 * H))), U=f(rng.standard_normal((H, 3 * H)) / np.sqrt(H)),
             h0=f(0.5 * rng.standard_normal((B, H))), att=f(rng.uniform(0, 1, (B, T))) if with_att else None,
             d_hs=f(rng.standard_normal((B, T, H))), d_h_last=f(rng.standard_normal((B, H))), q=f(rng.standard_normal((B, H))),
             d_a=f(rng.standard_normal((B, T))))
    lengths = rng.integers(0, T + 1, size=B)
    if B >= 3:
        lengths[:3] = (T, 1, 0)
    if B >= T + 4:
        lengths[3:T + 4] = np.arange(T + 1)
    c["lengths"] = torch.from_numpy(lengths.astype(np.int32))
    return c


ARGS = ("xp", "U", "h0", "lengths", "att")
NAMES = ("hs", "h_last", "d_xp", "dU", "d_h0", "d_att")


def run(c, dtype=DD, ar=PLAIN):
    """the six results (hs, h_last, d_xp, dU, d_h0, d_att | None) of a case in `dtype`"""
    cast = lambda t: None if t is None else (t if t.dtype in (torch.int32, torch.int64) else t.to(dtype))       # noqa: E731
    a = [cast(c[k]) for k in ARGS]
    with torch.no_grad():
        return tuple(forward(*a, ar=ar)) + tuple(backward(*a, cast(c["d_hs"]), cast(c["d_h_last"]), ar=ar))


@functools.lru_cache(maxsize=None)
def case(index):
    """inputs, the float64 results `want` and the float32 run of the same code `ref32`, computed once per session and not to be
    written to"""
    shape, with_att, seed = CASES[index]
    c = draw(shape, with_att, seed)
    c["shape"], c["with_att"] = shape, bool(with_att)
    c["want"] = run(c, DD)
    c["ref32"] = run(c, torch.float32)
    return c


def rel_err(got, want):
    """max |got - want| / max |want| (0 when want is all zero and got equals it)"""
    scale = want.abs().max().item() if want.numel() else 0.0
    err = (got.double() - want).abs().max().item() if want.numel() else 0.0
    return err / scale if scale > 0 else err


def limit(r32):
    return 16 * max(r32, 8 * U24)


# ---- the layers, for the glue tests: seq [B, T, D] -> xp = seq W + b -> the recurrence -----------------------------------------------
def gru_layer(seq, W, b, U, lengths=None, att=None, h0=None):
    B, T, D = seq.shape
    xp = (seq.reshape(B * T, D) @ W + (0 if b is None else b)).reshape(B, T, -1)
    return forward(xp, U, h0, lengths, att)


def evolution(hs, target, lengths, Wa, W, b, U):
    """InterestEvolution: q = target Wa^T, a = attention(hs, q), h'_last = AUGRU(hs, a)"""
    a = attention(hs, target @ Wa.t(), lengths)
    return gru_layer(hs, W, b, U, lengths, a)[1], a


def auxiliary_loss(hs, seq, neg_seq, lengths):
    """-mean over valid (b, t < len - 1) of [log sigmoid <h_t, e_{t+1}> + log(1 - sigmoid <h_t, e'_{t+1}>)]"""
    B, T, _ = hs.shape
    on = (torch.arange(T - 1)[None, :] < (_lens(lengths, B, T)[:, None] - 1))
    pos = (hs[:, :-1] * seq[:, 1:]).sum(-1)
    neg = (hs[:, :-1] * neg_seq[:, 1:]).sum(-1)
    terms = torch.nn.functional.logsigmoid(pos) + torch.nn.functional.logsigmoid(-neg)
    n = on.sum().clamp_min(1)
    return -(torch.where(on, terms, torch.zeros_like(terms))).sum() / n
