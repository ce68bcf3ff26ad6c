// Mini-batch graph sampling for GraphSAGE (Hamilton et al., NeurIPS 2017) and PinSage (Ying et al., KDD 2018); the arithmetic is
// spelled out in include/dr_hotpath.h, "Sampled graph blocks".  Integer kernels, counter-based on dr_mix32 like csrc/sampling.hip: an
// output is a function of (seed, inputs) alone, never of the launch.
//   sample    per node the `fanout` edges of its row with the smallest keys (hash(seed, e) << 32 | e - lo), written in ascending e.
//             A row of up to DR_SAMPLE_LONG_ROW edges is one wave's: the hashes go to LDS and every lane ranks its own edges against
//             all of them (deg^2 / 64 compares per lane, at most 4 K).  A longer row is a whole block's: a three-level radix select
//             (11 + 11 + 10 bits, LDS histograms) finds the fanout-th smallest hash, then every thread takes what lies below it in a
//             contiguous slice of the row.  The selection never reads col -- a key is a function of the edge index -- so a row of
//             20 000 edges costs five hash passes of 79 edges per thread and `fanout` loads.
//   walk_nbr  PinSage's importance neighbours: per start the ids of its R walks go to LDS, every lane counts the visits of its own
//             entries and the first occurrence of each id is ranked by (count desc, id asc) against the others.
//   frontier  the next layer's node list: (id, position) of dst ++ nbr are sorted by id with a stable LSD radix sort (dst first, so a
//             run of equal ids starts with the lowest dst index if dst holds the id at all); run heads that come from nbr are the new
//             ids, their exclusive scan is the ascending rank, and every nbr entry finds its run head by binary search.
//   block     row_ptr = exclusive scan of the kept counts (+ 1 with add_self), then one lane per row: sequential fp32 sum, one
//             division per entry.
// No float atomics and no float reductions across lanes; the only atomics are integer counts in LDS histograms (exact).
#include "dr_common.h"
#include "dr_rank_select.h"
#include "dr_scan.h"
#include <algorithm>

#ifndef DR_SAMPLE_LONG_ROW
#define DR_SAMPLE_LONG_ROW 512    // rows with more edges take the block path (mirrored as ops.SAMPLE_LONG_ROW)
#endif

namespace {

constexpr int SAMPLE_LONG_ROW = DR_SAMPLE_LONG_ROW;
constexpr int MAX_FANOUT = 64;
static_assert(SAMPLE_LONG_ROW >= MAX_FANOUT, "a long row must have more edges than any fanout");
constexpr int SEL_BINS = 2048;     // radix select: 11 + 11 + 10 bits of the 32-bit hash
constexpr int LONG_NODES = 16;     // nodes a block of sample_long_kernel looks at per pass

// (lo, deg) of node i's row; deg = 0 for i >= n or a node outside [0, n_rows)
__device__ __forceinline__ void row_of(const int64_t* __restrict__ row_ptr, int64_t n_rows, const int64_t* __restrict__ nodes, int64_t n,
                                       int64_t i, int64_t& lo, int64_t& deg) {
    lo = 0;
    deg = 0;
    if (i < n) {
        const int64_t v = nodes[i];
        if (v >= 0 && v < n_rows) {
            lo = row_ptr[v];
            deg = row_ptr[v + 1] - lo;
        }
    }
}

// One wave per node, four nodes per block and pass.  Rows over SAMPLE_LONG_ROW are left to sample_long_kernel.
__global__ __launch_bounds__(256) void sample_rows_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                          int64_t n_rows, const int64_t* __restrict__ nodes, int64_t n, int fanout,
                                                          uint64_t seed, int64_t* __restrict__ nbr, int32_t* __restrict__ cnt) {
    __shared__ uint32_t hs[4][SAMPLE_LONG_ROW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t* h = hs[w];
    const uint64_t lt_mask = dr_lanes_below(lane);
    for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
        const int64_t i = base + w;
        int64_t lo, deg;
        row_of(row_ptr, n_rows, nodes, n, i, lo, deg);
        const bool copy = i < n && deg <= fanout;
        const bool pick = i < n && deg > fanout && deg <= SAMPLE_LONG_ROW;
        const int d = pick ? (int)deg : 0;
        for (int j = lane; j < d; j += 64) h[j] = dr_mix32(seed, (uint64_t)(lo + j));
        __syncthreads();
        if (copy) {
            if (lane < fanout) nbr[i * fanout + lane] = lane < deg ? (int64_t)col[lo + lane] : -1;
            if (lane == 0) cnt[i] = (int32_t)deg;
        }
        if (pick) {
            int written = 0;
            for (int j0 = 0; j0 < d; j0 += 64) {
                const int j = j0 + lane;
                bool take = false;
                if (j < d) {
                    take = dr_key_rank(h, d, h[j], j) < fanout;     // keys below (h[j], j): dr_rank_select.h
                }
                const uint64_t b = __ballot(take);
                if (take) nbr[i * fanout + written + __popcll(b & lt_mask)] = (int64_t)col[lo + j];    // exactly fanout keys rank below fanout
                written += __popcll(b);
            }
            if (lane == 0) cnt[i] = fanout;
        }
        __syncthreads();                                       // h is rewritten by the next pass
    }
}

// Long rows, one at a time by the whole block.  Every block looks at LONG_NODES nodes per pass and lists the long ones in LDS: few
// nodes per block, because a batch's neighbours are mostly hubs (a node is reached in proportion to its degree) and a block takes its
// long rows one after the other.
__global__ __launch_bounds__(256) void sample_long_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                          int64_t n_rows, const int64_t* __restrict__ nodes, int64_t n, int fanout,
                                                          uint64_t seed, int64_t* __restrict__ nbr, int32_t* __restrict__ cnt) {
    __shared__ int hist[SEL_BINS];
    __shared__ int64_t red[4];
    __shared__ int list[LONG_NODES];
    __shared__ int n_list, sel_bin, sel_below;
    const int t = threadIdx.x;
    for (int64_t base = (int64_t)blockIdx.x * LONG_NODES; base < n; base += (int64_t)gridDim.x * LONG_NODES) {
        if (t == 0) n_list = 0;
        __syncthreads();
        if (t < LONG_NODES) {
            int64_t lo, deg;
            row_of(row_ptr, n_rows, nodes, n, base + t, lo, deg);
            if (deg > SAMPLE_LONG_ROW) list[atomicAdd(&n_list, 1)] = t;       // any order: every listed row writes its own outputs
        }
        __syncthreads();
        const int nl = n_list;
        for (int q = 0; q < nl; ++q) {
            const int64_t i = base + list[q];
            int64_t lo, deg;
            row_of(row_ptr, n_rows, nodes, n, i, lo, deg);
            // the hash T of the fanout-th smallest key, and `need`: how many of the edges whose hash equals T are taken (in edge order)
            uint32_t prefix = 0;
            int prefix_bits = 0, need = fanout;
            for (int level = 0; level < 3; ++level) {
                const int bits = level < 2 ? 11 : 10;
                const int shift = 32 - prefix_bits - bits;
                for (int b = t; b < SEL_BINS; b += 256) hist[b] = 0;
                __syncthreads();
                for (int64_t e = t; e < deg; e += 256) {
                    const uint32_t hv = dr_mix32(seed, (uint64_t)(lo + e));
                    if (prefix_bits == 0 || (hv >> (32 - prefix_bits)) == prefix) atomicAdd(&hist[(hv >> shift) & ((1u << bits) - 1)], 1);
                }
                __syncthreads();
                int mine = 0;
#pragma unroll
                for (int b = 0; b < SEL_BINS / 256; ++b) mine += hist[t * (SEL_BINS / 256) + b];
                int64_t total;
                int c = (int)block_excl_scan((int64_t)mine, red, total);
                if (c < need && need <= c + mine) {            // one thread: the bins' counts reach `need` inside its eight
                    for (int b = 0; b < SEL_BINS / 256; ++b) {
                        const int hb = hist[t * (SEL_BINS / 256) + b];
                        if (c + hb >= need) {
                            sel_bin = t * (SEL_BINS / 256) + b;
                            sel_below = c;
                            break;
                        }
                        c += hb;
                    }
                }
                __syncthreads();
                prefix = (prefix << bits) | (uint32_t)sel_bin;
                need -= sel_below;
                prefix_bits += bits;
                __syncthreads();                               // sel_bin / hist are rewritten by the next level
            }
            const uint32_t T = prefix;
            // thread t owns the edges [e0, e1) of the row: count, scan, write
            const int64_t per = (deg + 255) / 256;
            const int64_t e0 = t * per < deg ? t * per : deg, e1 = e0 + per < deg ? e0 + per : deg;
            int below = 0, ties = 0;
            for (int64_t e = e0; e < e1; ++e) {
                const uint32_t hv = dr_mix32(seed, (uint64_t)(lo + e));
                below += hv < T ? 1 : 0;
                ties += hv == T ? 1 : 0;
            }
            int64_t total;
            const int ties_before = (int)block_excl_scan((int64_t)ties, red, total);
            int tie_room = need - ties_before < ties ? need - ties_before : ties;
            tie_room = tie_room > 0 ? tie_room : 0;
            int pos = (int)block_excl_scan((int64_t)(below + tie_room), red, total);
            for (int64_t e = e0; e < e1; ++e) {
                const uint32_t hv = dr_mix32(seed, (uint64_t)(lo + e));
                bool take = hv < T;
                if (hv == T && tie_room > 0) {
                    take = true;
                    --tie_room;
                }
                if (take && pos < fanout) nbr[i * fanout + pos++] = (int64_t)col[lo + e];
            }
            if (t == 0) cnt[i] = fanout;
        }
        __syncthreads();                                       // list is rewritten by the next pass
    }
}

// One wave per start; LDS: ids [4][M] int64, then counts [4][M] int32 (M = R (L - 1) <= 1024)
__global__ __launch_bounds__(256) void walk_neighbors_kernel(const int64_t* __restrict__ walks, int64_t n, int R, int L, int T,
                                                             int64_t* __restrict__ nbr, float* __restrict__ weight,
                                                             int32_t* __restrict__ cnt) {
    extern __shared__ int64_t walk_lds[];
    const int M = R * (L - 1);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t* ids = walk_lds + (int64_t)w * M;
    int32_t* cs = reinterpret_cast<int32_t*>(walk_lds + 4 * (int64_t)M) + (int64_t)w * M;
    for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
        const int64_t i = base + w;
        const bool ok = i < n;
        if (ok) {
            const int64_t* wi = walks + i * R * L;
            const int64_t start = wi[0];
            for (int j = lane; j < M; j += 64) {
                const int64_t id = wi[(j / (L - 1)) * L + j % (L - 1) + 1];
                ids[j] = (id < 0 || id == start) ? -1 : id;
            }
        }
        __syncthreads();
        if (ok)
            for (int j = lane; j < M; j += 64) {               // visits of ids[j]; only an id's first occurrence keeps the count
                const int64_t id = ids[j];
                int c = 0;
                bool first = id >= 0;
                if (id >= 0)
                    for (int k = 0; k < M; ++k) {
                        const bool same = ids[k] == id;
                        c += same ? 1 : 0;
                        first = first && !(same && k < j);
                    }
                cs[j] = first ? c : 0;
            }
        __syncthreads();
        if (ok) {
            int reps = 0;
            for (int j0 = 0; j0 < M; j0 += 64) {
                const int j = j0 + lane;
                const int c = j < M ? cs[j] : 0;
                reps += __popcll(__ballot(c > 0));
                if (c > 0) {
                    const int64_t id = ids[j];
                    int rank = 0;                              // distinct ids ahead of this one: more visits, or as many and a smaller id
                    for (int k = 0; k < M; ++k) {
                        const int ck = cs[k];
                        rank += (ck > c || (ck == c && ids[k] < id)) ? 1 : 0;
                    }
                    if (rank < T) {
                        nbr[i * T + rank] = id;
                        weight[i * T + rank] = (float)c;
                    }
                }
            }
            const int kept = reps < T ? reps : T;
            for (int j = kept + lane; j < T; j += 64) {
                nbr[i * T + j] = -1;
                weight[i * T + j] = 0.f;
            }
            if (lane == 0) cnt[i] = kept;
        }
        __syncthreads();                                       // ids / cs are rewritten by the next pass
    }
}

// ---- exclusive scan in one launch for short arrays (the inner layers' frontiers are a few thousand entries: launches, not bytes) ----
constexpr int64_t SCAN_SINGLE_MAX = 8 * SCAN_TILE;

__global__ __launch_bounds__(256) void scan_single_kernel(const int64_t* __restrict__ x, int64_t n, int64_t* __restrict__ y) {
    __shared__ int64_t red[4];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < n; b0 += SCAN_TILE) {
        const int64_t base = b0 + threadIdx.x * 8;
        int64_t v[8], acc = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[i] = base + i < n ? x[base + i] : 0;
            acc += v[i];
        }
        int64_t total;
        int64_t e = carry + block_excl_scan(acc, red, total);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (base + i < n) y[base + i] = e;
            e += v[i];
        }
        carry += total;
    }
}

// y = exclusive_scan(x) (y may alias x); tmp as excl_scan's
void scan_any(const int64_t* x, int64_t n, int64_t* y, int64_t* tmp, hipStream_t st) {
    if (n <= SCAN_SINGLE_MAX) hipLaunchKernelGGL(scan_single_kernel, dim3(1), dim3(256), 0, st, x, n, y);
    else excl_scan(x, n, y, tmp, st);
}

// ---- frontier: stable LSD radix sort of (key uint64, position int32), 8 bits per pass ------------------------------------------
constexpr int RADIX_TILE = 256 * 8;

// keys[p] = the id at position p of dst ++ nbr, `none` for a negative id or one >= none; counts[0] = the length of dst's valid prefix
__global__ __launch_bounds__(256) void frontier_keys_kernel(const int64_t* __restrict__ dst, int64_t n_dst, const int64_t* __restrict__ nbr,
                                                            int64_t m, uint64_t none, uint64_t* __restrict__ keys, int32_t* __restrict__ pos,
                                                            int64_t* __restrict__ counts) {
    const int64_t N = n_dst + m;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < N; p += (int64_t)gridDim.x * 256) {
        const int64_t id = p < n_dst ? dst[p] : nbr[p - n_dst];
        keys[p] = (id < 0 || (uint64_t)id >= none) ? none : (uint64_t)id;
        pos[p] = (int32_t)p;
        if (p < n_dst && id >= 0 && (p == n_dst - 1 || dst[p + 1] < 0)) counts[0] = p + 1;     // the prefix ends here: one writer
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n_dst == 0 || dst[0] < 0)) counts[0] = 0;
}

// hist[d * n_tiles + tile] = number of keys of the tile whose digit is d
__global__ __launch_bounds__(256) void radix64_hist_kernel(const uint64_t* __restrict__ keys, int64_t n, int shift, int64_t n_tiles,
                                                           int64_t* __restrict__ hist) {
    __shared__ int c[256];
    c[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RADIX_TILE;
    for (int i = threadIdx.x; i < RADIX_TILE; i += 256)
        if (base + i < n) atomicAdd(&c[(int)((keys[base + i] >> shift) & 255)], 1);            // integer count: exact
    __syncthreads();
    hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = c[threadIdx.x];
}

// Stable scatter (csrc/graph.hip's, on 64-bit keys with one payload): the tile's keys in 8 rounds of 256 in index order; a key's
// place among equal digits of its round comes from a 64-lane match (8 ballots) plus the counts of the waves and rounds before it.
__global__ __launch_bounds__(256) void radix64_scatter_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ pay,
                                                              int64_t n, int shift, int64_t n_tiles, const int64_t* __restrict__ offs,
                                                              uint64_t* __restrict__ keys_out, int32_t* __restrict__ pay_out) {
    __shared__ int64_t base_d[256];
    __shared__ int run[256];
    __shared__ int wcnt[4][256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    base_d[t] = offs[(int64_t)t * n_tiles + blockIdx.x];
    run[t] = 0;
    const uint64_t lt_mask = dr_lanes_below(lane);
    for (int round = 0; round < RADIX_TILE / 256; ++round) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wcnt[i][t] = 0;
        __syncthreads();
        const int64_t e = (int64_t)blockIdx.x * RADIX_TILE + round * 256 + t;
        const bool ok = e < n;
        const uint64_t key = ok ? keys[e] : 0;
        const int d = (int)((key >> shift) & 255);
        uint64_t peers = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const uint64_t bl = __ballot((d >> b) & 1);
            peers &= ((d >> b) & 1) ? bl : ~bl;
        }
        const int rank = __popcll(peers & lt_mask);
        if (ok && rank == 0) wcnt[w][d] = __popcll(peers);
        __syncthreads();
        if (ok) {
            int off = run[d];
            for (int i = 0; i < w; ++i) off += wcnt[i][d];
            const int64_t p = base_d[d] + off + rank;
            keys_out[p] = key;
            pay_out[p] = pay[e];
        }
        __syncthreads();
        run[t] += wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
    }
}

// a run head whose first (lowest) position lies in nbr: an id dst does not hold
__device__ __forceinline__ bool is_new_head(const uint64_t* __restrict__ keys, const int32_t* __restrict__ pos, int64_t s, int64_t n_dst,
                                            uint64_t none) {
    const uint64_t k = keys[s];
    return k != none && (s == 0 || keys[s - 1] != k) && pos[s] >= n_dst;
}

__global__ __launch_bounds__(256) void frontier_flag_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ pos, int64_t N,
                                                            int64_t n_dst, uint64_t none, int64_t* __restrict__ flag) {
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < N; s += (int64_t)gridDim.x * 256)
        flag[s] = is_new_head(keys, pos, s, n_dst, none) ? 1 : 0;
}

// rank = exclusive scan of the flags.  Writes src, local and counts[1] (counts[0] is frontier_keys_kernel's).
__global__ __launch_bounds__(256) void frontier_emit_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ pos,
                                                            const int64_t* __restrict__ rank, int64_t N, const int64_t* __restrict__ dst,
                                                            int64_t n_dst, uint64_t none, int64_t* __restrict__ src,
                                                            int64_t* __restrict__ counts, int32_t* __restrict__ local) {
    const int64_t n_valid = counts[0];
    const int64_t n_new = rank[N - 1] + (is_new_head(keys, pos, N - 1, n_dst, none) ? 1 : 0);
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < N; s += (int64_t)gridDim.x * 256) {
        if (s < n_valid) src[s] = dst[s];
        else if (s >= n_valid + n_new) src[s] = -1;
        const int64_t p = pos[s];
        if (p < n_dst) continue;
        const uint64_t k = keys[s];
        if (k == none) {
            local[p - n_dst] = -1;
            continue;
        }
        int64_t h = s;
        if (s > 0 && keys[s - 1] == k) {                       // not the head of its run: the first position of k in the sorted keys
            int64_t a = 0, b = s;
            while (a < b) {
                const int64_t mid = a + ((b - a) >> 1);
                if (keys[mid] < k) a = mid + 1;
                else b = mid;
            }
            h = a;
        }
        const int64_t ph = pos[h];
        const int64_t c = ph < n_dst ? ph : n_valid + rank[h];
        local[p - n_dst] = (int32_t)c;
        if (h == s && ph >= n_dst) src[c] = (int64_t)k;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[1] = n_valid + n_new;
}

inline int64_t radix_tiles(int64_t N) { return (N + RADIX_TILE - 1) / RADIX_TILE; }

// ---- block CSR -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int kept_of(const int32_t* __restrict__ cnt, int64_t r, int fanout) {
    const int c = cnt[r];
    return c < 0 ? 0 : (c > fanout ? fanout : c);
}

// row_ptr[r] = the length of row r (0 for r >= the valid count and for the closing entry r == n_dst), scanned in place afterwards
__global__ __launch_bounds__(256) void block_len_kernel(const int32_t* __restrict__ cnt, int64_t n_dst, int fanout, int add_self,
                                                        const int64_t* __restrict__ n_valid, int64_t* __restrict__ row_ptr) {
    const int64_t nv = n_valid != nullptr ? *n_valid : n_dst;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r <= n_dst; r += (int64_t)gridDim.x * 256)
        row_ptr[r] = (r < n_dst && r < nv) ? kept_of(cnt, r, fanout) + (add_self ? 1 : 0) : 0;
}

__global__ __launch_bounds__(256) void block_fill_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ local,
                                                         const float* __restrict__ weight, int64_t n_dst, int fanout, int add_self,
                                                         const int64_t* __restrict__ n_valid, const int64_t* __restrict__ row_ptr,
                                                         int32_t* __restrict__ col, float* __restrict__ val) {
    const int64_t nv = n_valid != nullptr ? *n_valid : n_dst;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_dst && r < nv; r += (int64_t)gridDim.x * 256) {
        const int c = kept_of(cnt, r, fanout);
        float sum = add_self ? 1.f : 0.f;
        for (int k = 0; k < c; ++k) sum += weight != nullptr ? weight[r * fanout + k] : 1.f;
        int64_t o = row_ptr[r];
        if (add_self) {
            col[o] = (int32_t)r;
            val[o] = 1.f / sum;
            ++o;
        }
        for (int k = 0; k < c; ++k) {
            col[o + k] = local[r * fanout + k];
            val[o + k] = (weight != nullptr ? weight[r * fanout + k] : 1.f) / sum;
        }
    }
}

// the number of bits that hold every value below `none`'s own bit width (at least 1)
inline int key_bits(uint64_t none) {
    int bits = 1;
    while (bits < 64 && (none >> bits) != 0) ++bits;
    return bits;
}

}  // namespace

extern "C" int dr_neighbor_sample(const int64_t* row_ptr, const int32_t* col, int64_t n_rows, const int64_t* nodes, int64_t n,
                                  int32_t fanout, uint64_t seed, int64_t* nbr, int32_t* cnt, dr_stream_t stream) {
    if (n_rows < 0 || n < 0 || fanout < 1 || fanout > MAX_FANOUT) return DR_EINVAL;
    if (n == 0) return DR_OK;
    if (!row_ptr || !nodes || !nbr || !cnt) return DR_EINVAL;     // col may be NULL for a graph without edges: no degree is > 0
    hipStream_t st = dr_s(stream);
    hipLaunchKernelGGL(sample_rows_kernel, dim3(dr_grid_for(n, 4)), dim3(256), 0, st, row_ptr, col, n_rows, nodes, n, (int)fanout, seed, nbr,
                       cnt);
    hipLaunchKernelGGL(sample_long_kernel, dim3(dr_grid_for(n, LONG_NODES)), dim3(256), 0, st, row_ptr, col, n_rows, nodes, n, (int)fanout,
                       seed, nbr, cnt);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int dr_walk_neighbors(const int64_t* walks, int64_t n, int32_t R, int32_t L, int32_t T, int64_t* nbr, float* weight,
                                 int32_t* cnt, dr_stream_t stream) {
    if (n < 0 || R < 1 || L < 1 || T < 1 || T > MAX_FANOUT || (int64_t)R * (L - 1) > 1024) return DR_EINVAL;
    if (n == 0) return DR_OK;
    if (!walks || !nbr || !weight || !cnt) return DR_EINVAL;
    const size_t lds = (size_t)4 * R * (L - 1) * (sizeof(int64_t) + sizeof(int32_t));      // <= 48 KiB
    return dr_launch(walk_neighbors_kernel, dim3(dr_grid_for(n, 4)), dim3(256), lds, dr_s(stream), walks, n, (int)R, (int)L, (int)T, nbr,
                     weight, cnt);
}

extern "C" int64_t dr_frontier_workspace_bytes(int64_t n_dst, int64_t m) {
    if (n_dst < 0 || m < 0) return 0;
    const int64_t N = n_dst + m, nh = 256 * radix_tiles(N);
    // keys x2 and the rank (int64), the histogram and the scans' tile sums, positions x2 (int32)
    return 8 * (3 * N + nh + scan_blocks(std::max(nh, N)) + 1) + 4 * (2 * N) + 64;
}

extern "C" int dr_frontier_build(const int64_t* dst, int64_t n_dst, const int64_t* nbr, int64_t m, int64_t id_bound, int64_t* src,
                                 int64_t* counts, int32_t* local, void* workspace, int64_t workspace_bytes, dr_stream_t stream) {
    if (n_dst < 0 || m < 0 || n_dst + m >= (1ll << 31)) return DR_EINVAL;
    const int64_t N = n_dst + m;
    if (N == 0) return DR_OK;
    if ((n_dst > 0 && !dst) || (m > 0 && (!nbr || !local)) || !src || !counts || !workspace ||
        workspace_bytes < dr_frontier_workspace_bytes(n_dst, m))
        return DR_EINVAL;
    hipStream_t st = dr_s(stream);
    const uint64_t none = id_bound > 0 ? (uint64_t)id_bound : (uint64_t)INT64_MAX;
    const int64_t tiles = radix_tiles(N), nh = 256 * tiles;
    uint64_t* keys_a = static_cast<uint64_t*>(workspace);
    uint64_t* keys_b = keys_a + N;
    int64_t* rank = reinterpret_cast<int64_t*>(keys_b + N);
    int64_t* hist = rank + N;
    int64_t* tmp = hist + nh;
    int32_t* pos_a = reinterpret_cast<int32_t*>(tmp + scan_blocks(std::max(nh, N)) + 1);
    int32_t* pos_b = pos_a + N;
    const int grid = dr_grid_for(N, 256);
    hipLaunchKernelGGL(frontier_keys_kernel, dim3(grid), dim3(256), 0, st, dst, n_dst, nbr, m, none, keys_a, pos_a, counts);
    const int passes = (key_bits(none) + 7) / 8;
    uint64_t *k_src = keys_a, *k_dst = keys_b;
    int32_t *p_src = pos_a, *p_dst = pos_b;
    for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(radix64_hist_kernel, dim3((unsigned)tiles), dim3(256), 0, st, k_src, N, 8 * p, tiles, hist);
        scan_any(hist, nh, hist, tmp, st);
        hipLaunchKernelGGL(radix64_scatter_kernel, dim3((unsigned)tiles), dim3(256), 0, st, k_src, p_src, N, 8 * p, tiles, hist, k_dst,
                           p_dst);
        std::swap(k_src, k_dst);
        std::swap(p_src, p_dst);
    }
    hipLaunchKernelGGL(frontier_flag_kernel, dim3(grid), dim3(256), 0, st, k_src, p_src, N, n_dst, none, rank);
    scan_any(rank, N, rank, tmp, st);
    hipLaunchKernelGGL(frontier_emit_kernel, dim3(grid), dim3(256), 0, st, k_src, p_src, rank, N, dst, n_dst, none, src, counts, local);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

extern "C" int64_t dr_block_csr_workspace_bytes(int64_t n_dst) {
    if (n_dst < 0) return 0;
    return 8 * (scan_blocks(n_dst + 1) + 1);
}

extern "C" int dr_block_csr(const int32_t* cnt, const int32_t* local, const float* weight, int64_t n_dst, int32_t fanout, int32_t add_self,
                            const int64_t* n_valid, int64_t* row_ptr, int32_t* col, float* val, void* workspace, int64_t workspace_bytes,
                            dr_stream_t stream) {
    if (n_dst < 0 || fanout < 1 || fanout > MAX_FANOUT || (add_self != 0 && add_self != 1)) return DR_EINVAL;
    if (n_dst == 0) return DR_OK;
    if (!cnt || !local || !row_ptr || !col || !val || !workspace || workspace_bytes < dr_block_csr_workspace_bytes(n_dst)) return DR_EINVAL;
    hipStream_t st = dr_s(stream);
    hipLaunchKernelGGL(block_len_kernel, dim3(dr_grid_for(n_dst + 1, 256)), dim3(256), 0, st, cnt, n_dst, (int)fanout, (int)add_self, n_valid,
                       row_ptr);
    scan_any(row_ptr, n_dst + 1, row_ptr, static_cast<int64_t*>(workspace), st);
    hipLaunchKernelGGL(block_fill_kernel, dim3(dr_grid_for(n_dst, 256)), dim3(256), 0, st, cnt, local, weight, n_dst, (int)fanout,
                       (int)add_self, n_valid, row_ptr, col, val);
    DR_CHECK_LAUNCH();
    return DR_OK;
}
