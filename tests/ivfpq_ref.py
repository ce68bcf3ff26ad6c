"""NumPy restatement of the IVF-PQ index (csrc/ivf_pq.hip, FaissIVFPQ): inner product, residual encoding, 256 codewords per
sub-quantiser.  `encode` is fp32 in the kernel's own order of operations (so it is comparable bit for bit); everything a search
computes (`lut`, `adc_scores`, `adc_search`, `rerank`) is float64; `pack` is the word-plane-major list layout.  Also the fp32 error
bounds the GPU tests hold the kernels to, derived from the arithmetic (u = 2^-24, gamma_n = n u / (1 - n u))."""
import numpy as np

KSUB = 256
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def code_bytes(words, m):
    """uint32 / int32 words [N, m / 4] -> uint8 codes [N, m] (code j = bits 8 * (j % 4) of word j / 4)"""
    w = np.ascontiguousarray(words).view(np.uint32).reshape(len(words), m // 4)
    return np.stack([(w[:, j // 4] >> np.uint32(8 * (j % 4))) & np.uint32(255) for j in range(m)], axis=1).astype(np.uint8)


def code_words(codes):
    """uint8 codes [N, m] -> uint32 words [N, m / 4]"""
    N, m = codes.shape
    w = np.zeros((N, m // 4), dtype=np.uint32)
    for j in range(m):
        w[:, j // 4] |= codes[:, j].astype(np.uint32) << np.uint32(8 * (j % 4))
    return w


def residuals(x, assign=None, centroids=None):
    """fp32 x - centroids[assign] (one rounding per component); an assignment outside [0, nlist) has no residual (valid False)"""
    x = np.asarray(x, dtype=np.float32)
    if assign is None:
        return x, np.ones(len(x), dtype=bool)
    centroids = np.asarray(centroids, dtype=np.float32)
    ok = (assign >= 0) & (assign < len(centroids))
    r = (x - centroids[np.where(ok, assign, 0)]).astype(np.float32)
    return r, ok


def distances(r, codebooks, dtype=np.float32):
    """[N, m, 256]: sum over ascending d of (r_d - cb_d)^2, every operation rounded to `dtype` (no fused multiply-add)"""
    cb = np.asarray(codebooks, dtype=dtype)
    m, _, dsub = cb.shape
    r = np.asarray(r, dtype=dtype).reshape(len(r), m, dsub)
    dist = np.zeros((len(r), m, KSUB), dtype=dtype)
    for d in range(dsub):
        diff = (r[:, :, d, None] - cb[None, :, :, d]).astype(dtype)
        dist = (dist + (diff * diff).astype(dtype)).astype(dtype)
    return dist


def encode(x, codebooks, assign=None, centroids=None):
    """uint32 words [N, m / 4]: per sub-vector the codeword with the smallest fp32 distance, ties to the lower code; a vector whose
    assignment is out of range encodes as zeros"""
    r, ok = residuals(x, assign, centroids)
    codes = np.argmin(distances(r, codebooks), axis=2).astype(np.uint8)          # argmin: the first (lowest) of equal minima
    codes[~ok] = 0
    return code_words(codes)


def lut(q, codebooks):
    """float64 [Bq, m, 256]: LUT[b, j, c] = q_bj . cb_j[c]"""
    cb = np.asarray(codebooks, dtype=np.float64)
    m, _, dsub = cb.shape
    return np.einsum("bjd,jcd->bjc", np.asarray(q, dtype=np.float64).reshape(len(q), m, dsub), cb)


def adc_scores(q, centroids, codebooks, codes, assign):
    """float64 [Bq, N]: q . c_assign + sum_j LUT[j][code_j] of every candidate (codes: uint8 [N, m])"""
    T = lut(q, codebooks)
    m = T.shape[1]
    coarse = np.asarray(q, dtype=np.float64) @ np.asarray(centroids, dtype=np.float64).T
    s = coarse[:, np.clip(assign, 0, len(centroids) - 1)]
    for j in range(m):
        s = s + T[:, j, :][:, codes[:, j]]
    return s


def adc_abs(q, centroids, codebooks, codes, assign):
    """float64 [Bq, N] x 2: (|q . c| summed as sum_d |q_d c_d|, sum_j sum_d |q_d cb_j[code_j]_d|) -- the magnitudes the bounds scale"""
    aq = np.abs(np.asarray(q, dtype=np.float64))
    coarse = aq @ np.abs(np.asarray(centroids, dtype=np.float64)).T
    T = lut(aq, np.abs(np.asarray(codebooks, dtype=np.float64)))
    a = np.zeros((len(aq), len(codes)))
    for j in range(T.shape[1]):
        a = a + T[:, j, :][:, codes[:, j]]
    return coarse[:, np.clip(assign, 0, len(centroids) - 1)], a


def members(assign, probes_row):
    """rows of the probed lists of one query (a probe < 0 is skipped)"""
    return np.flatnonzero(np.isin(assign, probes_row[probes_row >= 0]))


def top_by_score(scores, rows, k):
    """(scores [k], rows [k]): score descending, ties to the lower row; (-inf, -1) tail"""
    order = np.lexsort((rows, -scores))[:k]
    s = np.full(k, -np.inf)
    i = np.full(k, -1, dtype=np.int64)
    s[:len(order)] = scores[order]
    i[:len(order)] = rows[order]
    return s, i


def adc_search(q, centroids, codebooks, codes, assign, probes, k):
    """float64 ADC top k of every query over its probed lists -> (scores [Bq, k], rows [Bq, k])"""
    S = adc_scores(q, centroids, codebooks, codes, assign)
    out_s = np.empty((len(q), k))
    out_i = np.empty((len(q), k), dtype=np.int64)
    for b in range(len(q)):
        rows = members(assign, probes[b])
        out_s[b], out_i[b] = top_by_score(S[b, rows], rows, k)
    return out_s, out_i


def ivf_exact_search(q, cand, assign, probes, k):
    """float64 exact inner-product top k over the probed lists (IVF-Flat's answer)"""
    S = np.asarray(q, dtype=np.float64) @ np.asarray(cand, dtype=np.float64).T
    out_s = np.empty((len(q), k))
    out_i = np.empty((len(q), k), dtype=np.int64)
    for b in range(len(q)):
        rows = members(assign, probes[b])
        out_s[b], out_i[b] = top_by_score(S[b, rows], rows, k)
    return out_s, out_i


def rerank(q, cand, rows, k):
    """float64 exact inner products with the named rows (< 0: none), top k"""
    out_s = np.empty((len(q), k))
    out_i = np.empty((len(q), k), dtype=np.int64)
    cand = np.asarray(cand, dtype=np.float64)
    for b in range(len(q)):
        r = rows[b][rows[b] >= 0]
        out_s[b], out_i[b] = top_by_score(cand[r] @ np.asarray(q[b], dtype=np.float64), r, k)
    return out_s, out_i


def pack(words, order, list_start):
    """(packed uint32 [(blocks * m/4) * 64], packed_rows int64 [blocks * 64], blk_off int64 [nlist + 1]): list l owns blocks
    [blk_off[l], blk_off[l + 1]) of 64 vectors, packed[(blk * (m/4) + w) * 64 + lane]; padding slots hold zero words and row -1"""
    words = np.ascontiguousarray(words).view(np.uint32)
    mw = words.shape[1]
    nlist = len(list_start) - 1
    counts = np.diff(list_start)
    blk_off = np.concatenate([[0], np.cumsum((counts + 63) // 64)]).astype(np.int64)
    total = int(blk_off[-1])
    packed = np.zeros((max(total, 1), mw, 64), dtype=np.uint32)
    rows = np.full((max(total, 1), 64), -1, dtype=np.int64)
    for l in range(nlist):
        src = order[list_start[l]:list_start[l + 1]]
        for p, s in enumerate(src):
            blk, lane = blk_off[l] + p // 64, p % 64
            packed[blk, :, lane] = words[s]
            rows[blk, lane] = s
    return packed.reshape(-1), rows.reshape(-1), blk_off


# ---- fp32 error bounds ---------------------------------------------------------------------------------------------------------------
def adc_bound(coarse_abs, lut_abs, probe_score_abs, m, dsub, probe_terms):
    """|fp32 ADC score - float64 ADC score| <=
         probe_terms * u * sum_d |q_d c_d|                      the coarse score as it reaches the scan (see the callers)
       + gamma_dsub * A                                          every LUT entry is an fmaf chain of dsub terms, A = sum_j sum_d |q_d cb_d|
       + gamma_m * (|p| + (1 + gamma_dsub) * A)                  m rounded adds onto the probe score, recursive summation
    """
    return probe_terms * U * coarse_abs + gamma(dsub) * lut_abs + gamma(m) * (probe_score_abs + (1.0 + gamma(dsub)) * lut_abs)


def rerank_bound(abs_dot, D):
    """dr_rerank_topk's inner product: per lane an fmaf chain of ceil(D / 64) terms, then six levels of rounded adds across the
    lanes -- gamma_(ceil(D / 64) + 6) * sum_d |q_d x_d|"""
    return gamma((D + 63) // 64 + 6) * abs_dot
