// Guarded optimizer step: one pass over the flat gradient for its global L2 norm and its non-finite count, one workgroup that
// turns them into the step's decision (clip coefficient, skip flag, counters, Adam's bias corrections) in a device-resident
// wn_guard_state, and the three flat updates reading that block.  What it replaces: torch.nn.utils.clip_grad_norm_ over the 123
// parameter tensors plus the optimizer's step (wavenet/train.py:28-42,182) - without the host ever seeing the norm, so the host
// keeps running ahead and the whole step stays legal under stream capture.  No atomics anywhere: every sum has one fixed order and
// the decision is a pure function of (g, n, gscale, the arguments, the state before).
#include "../../include/wavenet_hip.h"
#include "wn_common.h"
#include "wn_kernels.h"
#include "wn_optim.h"

static_assert(sizeof(wn_guard_state) == WN_GUARD_STATE_BYTES, "wn_guard_state: documented size");
static_assert(WN_GUARD_PARTIALS_BYTES == WN_GUARD_NUM_PARTIALS * (sizeof(double) + sizeof(uint32_t)), "partials layout");
#define GUARD_WG 256                                        // threads per workgroup (4 waves), in both kernels below
static_assert(GUARD_WG == WN_GUARD_NUM_PARTIALS, "guard_final_k stages one partial per thread");

// partials: WN_GUARD_NUM_PARTIALS doubles (sum of squares per workgroup), then as many uint32 (non-finite elements per workgroup)
__device__ __forceinline__ double* guard_sums(void* partials) { return (double*)partials; }
__device__ __forceinline__ uint32_t* guard_counts(void* partials) { return (uint32_t*)((double*)partials + WN_GUARD_NUM_PARTIALS); }

// one element: its square in float64 (1e20 does not overflow it, 1e-30 does not vanish), and whether the float32 value the update
// would apply, g * gscale, is finite
__device__ __forceinline__ void guard_elem(float gv, float gscale, double& acc, uint32_t& bad) {
    const double x = (double)gv * (double)gscale;
    acc += x * x;
    bad += isfinite(gv * gscale) ? 0u : 1u;
}

// Fixed grid of WN_GUARD_NUM_PARTIALS workgroups.  g needs 4-byte alignment only: up to three scalar elements in front of the first
// 16-byte boundary, float4 loads grid-strided over the body, up to three scalar elements behind it.
__global__ __launch_bounds__(GUARD_WG) void grad_sumsq_k(const float* __restrict__ g, long n, float gscale, void* __restrict__ partials) {
    __shared__ double s_sum[GUARD_WG / 64];
    __shared__ uint32_t s_bad[GUARD_WG / 64];
    const int tid = threadIdx.x;
    const long gid = (long)blockIdx.x * GUARD_WG + tid;
    const long nthreads = (long)WN_GUARD_NUM_PARTIALS * GUARD_WG;
    long head = (long)(((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    const long nvec = (n - head) >> 2;
    const long tail0 = head + 4 * nvec;                     // first element behind the body; n - tail0 < 4
    double acc = 0.0;
    uint32_t bad = 0;
    if (gid < head) guard_elem(g[gid], gscale, acc, bad);
    const float4* __restrict__ gv = (const float4*)(g + head);
    for (long k = gid; k < nvec; k += nthreads) {
        const float4 q = gv[k];
        guard_elem(q.x, gscale, acc, bad);
        guard_elem(q.y, gscale, acc, bad);
        guard_elem(q.z, gscale, acc, bad);
        guard_elem(q.w, gscale, acc, bad);
    }
    if (gid < n - tail0) guard_elem(g[tail0 + gid], gscale, acc, bad);
    // wave: butterfly (every lane ends with the same sum, the order is fixed by the lane numbers); workgroup: wave 0 .. 3 in order
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        bad += __shfl_xor(bad, o, 64);
    }
    if ((tid & 63) == 0) {
        s_sum[tid >> 6] = acc;
        s_bad[tid >> 6] = bad;
    }
    __syncthreads();
    if (tid == 0) {
        double s = s_sum[0];
        uint32_t b = s_bad[0];
        for (int w = 1; w < GUARD_WG / 64; ++w) {
            s += s_sum[w];
            b += s_bad[w];
        }
        guard_sums(partials)[blockIdx.x] = s;
        guard_counts(partials)[blockIdx.x] = b;
    }
}

// One workgroup: the partials summed in index order, then the decision.  use_partials == 0 (an empty gradient): norm 0.
__global__ __launch_bounds__(GUARD_WG) void guard_final_k(void* __restrict__ partials, int use_partials, float max_norm, int skip_nonfinite,
                                                          float beta1, float beta2, wn_guard_state* __restrict__ state) {
    __shared__ double s_sum[WN_GUARD_NUM_PARTIALS];
    __shared__ uint32_t s_bad[WN_GUARD_NUM_PARTIALS];
    const int tid = threadIdx.x;
    s_sum[tid] = use_partials ? guard_sums(partials)[tid] : 0.0;
    s_bad[tid] = use_partials ? guard_counts(partials)[tid] : 0u;
    __syncthreads();
    if (tid != 0) return;
    double sum = 0.0;
    uint32_t bad = 0;
    for (int k = 0; k < WN_GUARD_NUM_PARTIALS; ++k) {
        sum += s_sum[k];
        bad += s_bad[k];
    }
    const float norm = (float)sqrt(sum);
    const bool broken = bad > 0 || !isfinite(norm);
    const uint32_t skip = (skip_nonfinite && broken) ? 1u : 0u;
    float coef;
    if (broken) {
        coef = __builtin_nanf("");                          // skipped: not read; not skipped: the update turns into NaN, loudly
    } else if (max_norm <= 0.f) {
        coef = 1.0f;
    } else {
        const double c = (double)max_norm / ((double)norm + 1e-6);       // clip_grad_norm_'s rule
        coef = (float)(c < 1.0 ? c : 1.0);
    }
    state->norm = norm;
    state->coef = coef;
    state->nonfinite = bad;
    state->skip = skip;
    if (skip) {
        state->n_skipped = state->n_skipped + 1;            // n_taken, bc1, bc2 stay: the step did not happen
        return;
    }
    const uint64_t t = state->n_taken + 1;
    state->n_taken = t;
    if (coef < 1.0f) state->n_clipped = state->n_clipped + 1;
    state->bc1 = (float)(1.0 - pow((double)beta1, (double)t));
    state->bc2 = (float)(1.0 - pow((double)beta2, (double)t));
}

int wn_launch_grad_guard(const float* g, long n, float gscale, float max_norm, int skip_nonfinite, float beta1, float beta2,
                         void* partials, wn_guard_state* state, hipStream_t st) {
    if (n > 0) {
        hipLaunchKernelGGL(grad_sumsq_k, dim3(WN_GUARD_NUM_PARTIALS), dim3(GUARD_WG), 0, st, g, n, gscale, partials);
        WN_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(guard_final_k, dim3(1), dim3(GUARD_WG), 0, st, partials, n > 0 ? 1 : 0, max_norm, skip_nonfinite, beta1, beta2,
                       state);
    WN_CHECK_LAUNCH();
    return 0;
}

// The guarded updates: the plain kernels' arithmetic (wn_optim.h) on g * gscale * coef; a skipped step returns before it touches
// anything, so parameters and optimizer state stay bit for bit what they were.
__global__ void adam_guarded_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                               float lr, float b1, float b2, float eps, float gscale, const wn_guard_state* __restrict__ state) {
    if (state->skip) return;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    wn_adam_body<true>(p, g, m, v, i, stride, n, lr, b1, b2, eps, state->bc1, state->bc2, gscale, state->coef);
}
// SGD's first step (buf = g) is the first step TAKEN: a skipped first step must not seed the momentum buffer
__global__ void sgd_guarded_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long n, float lr, float momentum,
                              float gscale, const wn_guard_state* __restrict__ state) {
    if (state->skip) return;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    wn_sgd_body<true>(p, g, buf, i, stride, n, lr, momentum, gscale, state->n_taken == 1 ? 1 : 0, state->coef);
}
__global__ void rmsprop_guarded_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq, float* __restrict__ buf,
                                  long n, float lr, float alpha, float eps, float momentum, float gscale,
                                  const wn_guard_state* __restrict__ state) {
    if (state->skip) return;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    wn_rmsprop_body<true>(p, g, sq, buf, i, stride, n, lr, alpha, eps, momentum, gscale, state->coef);
}

static int guard_update_grid(long n) {
    long grid = (n + 255) / 256;
    return (int)(grid > 2048 ? 2048 : grid);
}
int wn_launch_adam_guarded(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, float gscale,
                           const wn_guard_state* state, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(adam_guarded_k, dim3(guard_update_grid(n)), dim3(256), 0, st, p, g, m, v, n, lr, b1, b2, eps, gscale, state);
    WN_CHECK_LAUNCH();
    return 0;
}
int wn_launch_sgd_guarded(float* p, const float* g, float* buf, long n, float lr, float momentum, float gscale,
                          const wn_guard_state* state, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(sgd_guarded_k, dim3(guard_update_grid(n)), dim3(256), 0, st, p, g, buf, n, lr, momentum, gscale, state);
    WN_CHECK_LAUNCH();
    return 0;
}
int wn_launch_rmsprop_guarded(float* p, const float* g, float* sq, float* buf, long n, float lr, float alpha, float eps, float momentum,
                              float gscale, const wn_guard_state* state, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(rmsprop_guarded_k, dim3(guard_update_grid(n)), dim3(256), 0, st, p, g, sq, buf, n, lr, alpha, eps, momentum, gscale,
                       state);
    WN_CHECK_LAUNCH();
    return 0;
}

// EMA shadow of the parameters, behind any of the six updates above and in wn_elem.hip (the arithmetic: wn_optim.h).  state NULL:
// T = t, the caller's count of updates.  Else the decision of the wn_grad_guard before it on the stream: a skipped step leaves the
// shadow bit for bit, a taken one is update number n_taken + t.  Element-wise on 4-byte accesses: ema and p need no common alignment.
__global__ void ema_k(float* __restrict__ ema, const float* __restrict__ p, long n, float decay, int warmup, long t,
                      const wn_guard_state* __restrict__ state) {
    long T = t;
    if (state) {
        if (state->skip) return;
        T = (long)state->n_taken + t;
    }
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    wn_ema_body(ema, p, i, stride, n, wn_ema_weight(decay, warmup, T));
}
int wn_launch_ema(float* ema, const float* p, long n, float decay, int warmup, long t, const wn_guard_state* state, hipStream_t st) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(ema_k, dim3(guard_update_grid(n)), dim3(256), 0, st, ema, p, n, decay, warmup, t, state);
    WN_CHECK_LAUNCH();
    return 0;
}
