// Streaming confusion histogram behind metrics.py (AUC / Precision / Recall / StreamingAUC): dr_confusion_hist_update.
//
// State: hist[2][T + 1] fp64, row = (label != 0), column = bucket(p) = #{t : p > thresholds[t]} in 0..T.  Every confusion vector of
// tf.keras.metrics.AUC / tf.metrics.auc is a suffix sum of a row (tp[t] = sum_{b > t} hist[1][b]), so one histogram pass replaces the
// T comparisons per example that TensorFlow performs -- and gives the same counts, because the bucket is DEFINED by those comparisons.
//
// Stage 1 (confusion_hist_stage1): a block keeps the thresholds and its partial histogram in LDS (uint32 bins without weights, fp64
// bins with), streams its share of the examples with 16-byte loads, and stores the partial to its slab of the workspace.
//   bucket   guess g = floor(p (T - 1)) + 1 (right for the evenly spaced grid except on or beside a threshold), then the guess is
//            CHECKED against the definition: thresholds ascending => bucket(p) = g  <=>  p > thr[g - 1] and not p > thr[g].  A lane
//            whose guess fails the check bisects the LDS copy for the first t with not (p > thr[t]).  Both paths answer by fp32
//            comparisons with the array that was passed, so the result is exact for any ascending array, grid or not.
//   LDS adds early in training every prediction falls into one or two bins and all 64 lanes of a wave would add to one LDS address.
//            Before the per-lane add, up to PEEL rounds take the first live lane's bin, ballot the lanes that hold the same bin, and
//            let that one lane add the whole group (its population count, or the fp64 sum of its weights); the lanes that remain add
//            for themselves.  Two rounds cover the degenerate case (one bucket x two labels); on spread-out data a round removes
//            about one lane and costs two ballots.
// Stage 2 (confusion_hist_stage2): hist[b] += sum over the slabs in a fixed order (integer sums without weights: exact and
// bit-identical from run to run; fp64 with weights, where only the order of the LDS adds inside a block is free).
#include "dr_common.h"

namespace {

constexpr int HIST_BLOCK = 512;          // threads per stage-1 block
constexpr int HIST_MAX_T = 4096;         // dr_hotpath.h states it
constexpr int HIST_PEEL = 2;
constexpr int64_t HIST_MAX_N = (int64_t)1 << 40;   // a block's uint32 bin holds at most n / grid + HIST_BLOCK * 4 < 2^32 counts

// slabs: fewer for a long histogram (each block stores 2 (T + 1) bins whatever n is)
inline int hist_grid(int64_t n, int32_t T) {
    return dr_grid_for((n + 3) / 4, HIST_BLOCK, 2 * (T + 1) > 2048 ? 256 : 512);
}

typedef float hist_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int hist_bucket(float p, const float* __restrict__ thr, int T) {
    // fmaxf / fminf return the other operand for a NaN: a NaN guesses 0, and passes the check there (NaN > x is false)
    const float q = fminf(fmaxf(floorf(p * (float)(T - 1)) + 1.f, 0.f), (float)T);
    int g = (int)q;
    const bool lo_ok = g == 0 || p > thr[g > 0 ? g - 1 : 0];
    const bool hi_ok = g == T || !(p > thr[g < T ? g : T - 1]);
    if (!(lo_ok && hi_ok)) {
        int lo = 0, hi = T;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (p > thr[mid]) lo = mid + 1;
            else hi = mid;
        }
        g = lo;
    }
    return g;
}

__device__ __forceinline__ double hist_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one example per lane, the whole wave here together (`live` = this lane holds an example)
template <bool WEIGHTED>
__device__ __forceinline__ void hist_add(bool live, int key, float w, unsigned* __restrict__ ibins, double* __restrict__ dbins) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < HIST_PEEL; ++r) {
        const uint64_t rem = __ballot(live);
        if (rem == 0) return;
        const int lead = __ffsll((unsigned long long)rem) - 1;
        const int k0 = __shfl(key, lead, 64);
        const bool same = live && key == k0;
        const uint64_t grp = __ballot(same);
        const int cnt = __popcll(grp);
        if (WEIGHTED) {
            if (cnt < 8) break;                                  // not worth six fp64 shuffles
            const double s = hist_wave_sum(same ? (double)w : 0.0);
            if (lane == lead) atomicAdd(&dbins[k0], s);
        } else {
            if (lane == lead) atomicAdd(&ibins[k0], (unsigned)cnt);
        }
        live = live && !same;
    }
    if (live) {
        if (WEIGHTED) atomicAdd(&dbins[key], (double)w);
        else atomicAdd(&ibins[key], 1u);
    }
}

template <bool WEIGHTED, bool LOGITS>
__device__ __forceinline__ void hist_one(bool live, float p, float y, float w, const float* __restrict__ thr, int T,
                                         unsigned* __restrict__ ibins, double* __restrict__ dbins) {
    if (LOGITS) p = dr_sigmoidf(p);
    const int key = live ? (y != 0.f ? T + 1 : 0) + hist_bucket(p, thr, T) : 0;
    hist_add<WEIGHTED>(live, key, w, ibins, dbins);
}

template <bool WEIGHTED, bool LOGITS>
__global__ __launch_bounds__(HIST_BLOCK) void confusion_hist_stage1(const float* __restrict__ pred, const float* __restrict__ labels,
                                                                    const float* __restrict__ weights, int64_t n,
                                                                    const float* __restrict__ thresholds, int T, int vec,
                                                                    void* __restrict__ slabs) {
    extern __shared__ double hist_lds[];                         // [bins: 2 (T + 1) fp64 or uint32][thresholds: T floats]
    const int nbins = 2 * (T + 1);
    double* dbins = hist_lds;
    unsigned* ibins = reinterpret_cast<unsigned*>(hist_lds);
    float* thr = WEIGHTED ? reinterpret_cast<float*>(dbins + nbins) : reinterpret_cast<float*>(ibins + nbins);
    for (int i = threadIdx.x; i < nbins; i += HIST_BLOCK) {
        if (WEIGHTED) dbins[i] = 0.0;
        else ibins[i] = 0u;
    }
    for (int i = threadIdx.x; i < T; i += HIST_BLOCK) thr[i] = thresholds[i];
    __syncthreads();

    // 16-byte part: vector i holds examples 4 i .. 4 i + 3.  The trip count is the same for every lane of a wave (the ballots in
    // hist_add need the whole wave), the next trip's loads are issued before this trip's examples are binned.
    const int64_t nv = vec ? (n >> 2) : 0;
    const hist_f4* p4 = reinterpret_cast<const hist_f4*>(pred);
    const hist_f4* y4 = reinterpret_cast<const hist_f4*>(labels);
    const hist_f4* w4 = reinterpret_cast<const hist_f4*>(weights);
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * HIST_BLOCK;
    int64_t base = (int64_t)blockIdx.x * HIST_BLOCK + (threadIdx.x - lane);
    const hist_f4 zero = {0.f, 0.f, 0.f, 0.f};
    hist_f4 p = zero, y = zero, w = zero;
    if (base + lane < nv) {
        p = __builtin_nontemporal_load(p4 + base + lane);
        y = __builtin_nontemporal_load(y4 + base + lane);
        if (WEIGHTED) w = __builtin_nontemporal_load(w4 + base + lane);
    }
    while (base < nv) {
        const bool live = base + lane < nv;
        const int64_t next = base + stride;
        hist_f4 pn = zero, yn = zero, wn = zero;
        if (next + lane < nv) {
            pn = __builtin_nontemporal_load(p4 + next + lane);
            yn = __builtin_nontemporal_load(y4 + next + lane);
            if (WEIGHTED) wn = __builtin_nontemporal_load(w4 + next + lane);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) hist_one<WEIGHTED, LOGITS>(live, p[j], y[j], w[j], thr, T, ibins, dbins);
        p = pn; y = yn; w = wn;
        base = next;
    }
    // what the vectors left: the last n % 4 examples, or all of them when a pointer is not 16-byte aligned
    for (int64_t sb = nv * 4 + (int64_t)blockIdx.x * HIST_BLOCK + (threadIdx.x - lane); sb < n; sb += stride) {
        const bool live = sb + lane < n;
        const int64_t i = live ? sb + lane : 0;
        hist_one<WEIGHTED, LOGITS>(live, pred[i], labels[i], WEIGHTED ? weights[i] : 1.f, thr, T, ibins, dbins);
    }
    __syncthreads();
    if (WEIGHTED) {
        double* out = static_cast<double*>(slabs) + (int64_t)blockIdx.x * nbins;
        for (int i = threadIdx.x; i < nbins; i += HIST_BLOCK) out[i] = dbins[i];
    } else {
        unsigned* out = static_cast<unsigned*>(slabs) + (int64_t)blockIdx.x * nbins;
        for (int i = threadIdx.x; i < nbins; i += HIST_BLOCK) out[i] = ibins[i];
    }
}

// hist[b] += sum_g slab[g][b]: 64 bins per block, the slabs dealt to 4 waves round-robin, the 4 partial sums added in a fixed order
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void confusion_hist_stage2(const void* __restrict__ slabs, int nslabs, int nbins,
                                                             double* __restrict__ hist) {
    __shared__ double part[4][64];
    const int b = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    double facc = 0.0;
    unsigned long long iacc = 0;
    if (b < nbins) {
        if (WEIGHTED) {
            const double* s = static_cast<const double*>(slabs);
            for (int g = q; g < nslabs; g += 4) facc += s[(int64_t)g * nbins + b];
        } else {
            const unsigned* s = static_cast<const unsigned*>(slabs);
            for (int g = q; g < nslabs; g += 4) iacc += s[(int64_t)g * nbins + b];
            facc = (double)iacc;                                 // < 2^53: exact
        }
    }
    part[q][threadIdx.x & 63] = facc;
    __syncthreads();
    if (q == 0 && b < nbins) {
        const int l = threadIdx.x;
        hist[b] += (part[0][l] + part[1][l]) + (part[2][l] + part[3][l]);
    }
}

template <bool WEIGHTED, bool LOGITS>
int hist_launch(const float* pred, const float* labels, const float* weights, int64_t n, const float* thresholds, int32_t T,
                double* hist, void* workspace, hipStream_t s) {
    const int nbins = 2 * (T + 1);
    const size_t lds = (size_t)nbins * (WEIGHTED ? 8 : 4) + (size_t)T * 4;
    const int grid = hist_grid(n, T);
    const uintptr_t a = reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(weights);
    const int st = dr_launch<48>(confusion_hist_stage1<WEIGHTED, LOGITS>, dim3(grid), dim3(HIST_BLOCK), lds, s, pred, labels, weights, n,
                                 thresholds, (int)T, (int)((a & 15) == 0), workspace);
    if (st != DR_OK) return st;
    hipLaunchKernelGGL(confusion_hist_stage2<WEIGHTED>, dim3((nbins + 63) / 64), dim3(256), 0, s, workspace, grid, nbins, hist);
    DR_CHECK_LAUNCH();
    return DR_OK;
}

}  // namespace

extern "C" int64_t dr_confusion_hist_workspace_bytes(int64_t n, int32_t num_thresholds) {
    if (n < 0 || num_thresholds < 1 || num_thresholds > HIST_MAX_T) return 0;
    return (int64_t)hist_grid(n, num_thresholds) * 2 * (num_thresholds + 1) * 8;
}

extern "C" int dr_confusion_hist_update(const float* pred, const float* labels, const float* weights, int64_t n,
                                        const float* thresholds, int32_t T, int32_t from_logits, double* hist, void* workspace,
                                        dr_stream_t stream) {
    if (T < 1 || n < 0) return DR_EINVAL;
    if (T > HIST_MAX_T || n > HIST_MAX_N) return DR_ESHAPE;
    if (n == 0) return DR_OK;
    if (!pred || !labels || !hist || !thresholds || !workspace) return DR_EINVAL;
    hipStream_t s = dr_s(stream);
    if (weights) {
        return from_logits ? hist_launch<true, true>(pred, labels, weights, n, thresholds, T, hist, workspace, s)
                           : hist_launch<true, false>(pred, labels, weights, n, thresholds, T, hist, workspace, s);
    }
    return from_logits ? hist_launch<false, true>(pred, labels, weights, n, thresholds, T, hist, workspace, s)
                       : hist_launch<false, false>(pred, labels, weights, n, thresholds, T, hist, workspace, s);
}
