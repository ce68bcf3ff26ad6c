"""NumPy restatements of the four sampled-block kernels (include/dr_hotpath.h, "Sampled graph blocks"), written from the header's
comment: plain loops, sorts and dicts, nothing shared with csrc/neighbor_sample.hip.  The GPU tests compare bit for bit against them."""
import numpy as np


def mix32(seed, idx):
    """dr_mix32(seed, idx): z = idx * 0x9E3779B97F4A7C15 + seed; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) *
    0x94D049BB133111EB; (z ^ z >> 31) >> 32 -- in uint64 wrap-around arithmetic, uint32 out"""
    with np.errstate(over="ignore"):
        z = np.asarray(idx).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(int(seed) & (2 ** 64 - 1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)


def neighbor_sample_ref(row_ptr, col, n_rows, nodes, fanout, seed):
    row_ptr, col, nodes = np.asarray(row_ptr, np.int64), np.asarray(col, np.int32), np.asarray(nodes, np.int64)
    n = nodes.size
    nbr = np.full((n, fanout), -1, dtype=np.int64)
    cnt = np.zeros(n, dtype=np.int32)
    for i, v in enumerate(nodes.tolist()):
        if v < 0 or v >= n_rows:
            continue
        lo, hi = int(row_ptr[v]), int(row_ptr[v + 1])
        deg = hi - lo
        if deg <= fanout:
            nbr[i, :deg] = col[lo:hi]
            cnt[i] = deg
            continue
        e = np.arange(lo, hi, dtype=np.uint64)
        keys = (mix32(seed, e).astype(np.uint64) << np.uint64(32)) | (e - np.uint64(lo))
        taken = np.sort(np.argsort(keys, kind="stable")[:fanout])          # the fanout smallest keys, then ascending e
        nbr[i] = col[lo + taken]
        cnt[i] = fanout
    return nbr, cnt


def walk_neighbors_ref(walks, T):
    walks = np.asarray(walks, np.int64)
    n = walks.shape[0]
    nbr = np.full((n, T), -1, dtype=np.int64)
    weight = np.zeros((n, T), dtype=np.float32)
    cnt = np.zeros(n, dtype=np.int32)
    for i in range(n):
        start = int(walks[i, 0, 0])
        visits = {}
        for v in walks[i, :, 1:].reshape(-1).tolist():
            if v >= 0 and v != start:
                visits[v] = visits.get(v, 0) + 1
        order = sorted(visits.items(), key=lambda kv: (-kv[1], kv[0]))[:T]
        for j, (v, c) in enumerate(order):
            nbr[i, j], weight[i, j] = v, np.float32(c)
        cnt[i] = len(order)
    return nbr, weight, cnt


def frontier_build_ref(dst, nbr):
    """(src, counts, local); nbr of any shape, local of the same shape"""
    dst, nbr = np.asarray(dst, np.int64), np.asarray(nbr, np.int64)
    flat = nbr.reshape(-1)
    n_valid = 0
    while n_valid < dst.size and dst[n_valid] >= 0:
        n_valid += 1
    where = {}
    for i, v in enumerate(dst[:n_valid].tolist()):
        where.setdefault(v, i)                                              # the lowest index of a repeated id
    new = sorted({v for v in flat.tolist() if v >= 0 and v not in where})
    for j, v in enumerate(new):
        where[v] = n_valid + j
    src = np.full(dst.size + flat.size, -1, dtype=np.int64)
    src[:n_valid] = dst[:n_valid]
    src[n_valid:n_valid + len(new)] = new
    local = np.asarray([where[v] if v >= 0 else -1 for v in flat.tolist()], dtype=np.int32).reshape(nbr.shape)
    return src, np.asarray([n_valid, n_valid + len(new)], dtype=np.int64), local


def block_csr_ref(cnt, local, weight=None, add_self=False, n_valid=None):
    """(row_ptr, col, val) with col / val cut to row_ptr[-1] entries"""
    cnt, local = np.asarray(cnt, np.int32), np.asarray(local, np.int32)
    n_dst, fanout = local.shape
    n_valid = n_dst if n_valid is None else int(n_valid)
    row_ptr = np.zeros(n_dst + 1, dtype=np.int64)
    col, val = [], []
    for r in range(n_dst):
        if r < n_valid:
            c = min(max(int(cnt[r]), 0), fanout)
            w = [np.float32(1.0)] * c if weight is None else [np.float32(x) for x in np.asarray(weight, np.float32)[r, :c]]
            ids = local[r, :c].tolist()
            if add_self:
                w, ids = [np.float32(1.0)] + w, [r] + ids
            s = np.float32(0.0)
            for x in w:
                s = np.float32(s + x)                                       # in row order, in fp32
            col += ids
            val += [np.float32(x / s) for x in w]                           # one fp32 division per entry
        row_ptr[r + 1] = len(col)
    return row_ptr, np.asarray(col, dtype=np.int32), np.asarray(val, dtype=np.float32)
