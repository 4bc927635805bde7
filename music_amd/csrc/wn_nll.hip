// The PER-TIMESTEP softmax and the true negative log-likelihood over the channel axis of the compact [B][Q][W] logits (wn_step_softmax,
// wn_step_nll in include/wavenet_hip.h): the distribution the decoder samples from, as a training and scoring objective.  The chunk
// softmax of wn_elem.hip / wn_generic.hip runs over 256 consecutive floats of that buffer, i.e. over time, and its loss
// applies a second log-softmax to the probabilities; nothing of either is reproduced here.
//
// The channel axis has stride `pitch` and time is contiguous, so a workgroup owns a tile of 64 columns of one clip: lane = column
// (every global access of a wave is 64 consecutive floats of one channel row), the waves split the q rows RPW apiece and keep them in
// registers, the column max / argmax / target logit and the column sum cross the waves through LDS.  x is read once, dx written once.
// Any W: a clip's base is only 4-byte aligned, so every access is a scalar dword per lane and the last tile of a clip is masked.
// No float atomics: block i sums its tiles in a fixed order into loss_part[i]; the same bits come back on every launch.
//
// WIN (wn_win_step_nll, wn_win_step_softmax): the samplers' window rule as an objective.  A column at stream position p takes the
// softmax over the rows [lo, hi) of pair p mod period alone: the lane picks its pair once per tile, rows outside it enter the
// reductions as -inf (their exp is an exact 0, so probs and dx outside are +0.0 without a second predicate) and what x holds there
// stays behind the window's predicate: it never reaches arithmetic.  WIN = false is the code from before the windows.
//
// WT (wn_wstep_nll): a weight per column, an ignored target, label smoothing, the mean over the weights' sum.  A column is a lane, and
// nothing but the lane's own loss term leaves it (the waves exchange per-lane values only), so a column of weight 0 is skipped by
// predicates on that term and on its stores: what x holds there stays in the lane.  The weight lives in one register of the lane; the
// smoothing's sum of the window's logits is taken from the rows in registers before exp() overwrites them and crosses the waves through
// an LDS array of its own, beside the maximum's (WT instantiations only).  1 / sum of weights comes from den[1], which nll_den_k wrote in
// the launch before: no host read-back.  WT = false is the code from before, instruction for instruction.
#include <type_traits>

#include "wn_common.h"
#include "wn_kernels.h"

struct WnNoWin {};
// the last kernel argument: the window table or nothing, and behind it in the WT instantiations the weights' part
template <bool WIN>
struct WnNllWtArgs : std::conditional_t<WIN, WnNllWin, WnNoWin> {
    const float *weight, *den;
    long ignore;
    float smoothing;
};
template <bool WIN, bool WT>
using WnNllArgs = std::conditional_t<WT, WnNllWtArgs<WIN>, std::conditional_t<WIN, WnNllWin, WnNoWin>>;

// the weight of column col: an exact 0 under an ignored target, which is read for that comparison alone (the two loads are
// independent: the weight's does not wait for the target's, its value is dropped under an ignored target)
__device__ __forceinline__ float nll_weight(const float* __restrict__ weight, const int64_t* __restrict__ target, long ignore, long col) {
    const float wv = weight ? weight[col] : 1.f;
    return target[col] == ignore ? 0.f : wv;
}

// den[0] = the sum of the weights over n columns, den[1] = (float)(1 / that sum) or 0 for a sum of 0; NaN both when a counted weight is
// negative or not finite.  ONE block: every thread sums its strided share in double, the block folds the 1024 shares as a fixed tree.
// The block is bound by the latency of its loads, so a thread keeps eight columns in flight; it still adds them in the order
// i, i + 1024, i + 2048, ..
__global__ __launch_bounds__(1024) void nll_den_k(const float* __restrict__ weight, const int64_t* __restrict__ target, long ignore, long n,
                                                  float* __restrict__ den) {
    __shared__ double s_d[1024];
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    double acc = 0.0;
    bool bad = false;
    long i = threadIdx.x;
    for (; i + 7 * 1024 < n; i += 8 * 1024) {
        float w8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w8[u] = nll_weight(weight, target, ignore, i + u * 1024);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            bad = bad || !(w8[u] >= 0.f && w8[u] <= 3.402823466e38f);
            acc += (double)w8[u];
        }
    }
    for (; i < n; i += 1024) {
        const float wv = nll_weight(weight, target, ignore, i);
        bad = bad || !(wv >= 0.f && wv <= 3.402823466e38f);
        acc += (double)wv;
    }
    s_d[threadIdx.x] = acc;
    if (bad) s_bad = 1;                                          // (every writer stores the same value)
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_d[threadIdx.x] += s_d[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double sum = s_d[0];
        const float nan = __builtin_nanf("");
        den[0] = s_bad ? nan : (float)sum;
        den[1] = s_bad ? nan : (sum == 0.0 ? 0.f : (float)(1.0 / sum));
    }
}

// probabilities go out row-major per time step ([column][q]): a wave turns TR of its rows at a time through a [64][TR + 1] LDS tile
// of its own and writes segments of TR consecutive floats
// Q256: q is 256 and the block has 4 waves of 64 rows (120 registers, no scratch: four blocks per CU, so a grid of up to 1024 blocks
// is resident at once); else q is a run-time value, the block has ceil(q / 64) <= MAXT / 64 waves and rows >= q are masked.
template <int RPW, int TR, bool Q256, int MAXT, bool WIN, bool WT>
__global__ __launch_bounds__(MAXT) void step_nll_k(
        const float* __restrict__ x, long x_bs, int x_pitch, const int64_t* __restrict__ target, float* __restrict__ dx, long dx_bs,
        int dx_pitch, float* __restrict__ probs, float* __restrict__ row_nll, int32_t* __restrict__ row_hit,
        float* __restrict__ loss_part, int w, int q_rt, int tiles_per_clip, long ntiles, float inv_n_arg,
        const WnNllArgs<WIN, WT> win) {
    constexpr int MAXW = MAXT / 64;
    constexpr int TP = TR + 1;
    __shared__ float s_max[MAXW][64], s_sum[MAXW][64], s_xy[64];
    __shared__ int s_arg[MAXW][64];
    __shared__ float s_t[MAXW][64 * TP];
    __shared__ int s_win[WIN ? 2 * WN_WIN_MAX : 1];
    float(*s_sx)[64] = nullptr;
    if constexpr (WT) {
        __shared__ float s_sxw[MAXW][64];
        s_sx = s_sxw;
    }
    const int q = Q256 ? 256 : q_rt;
    // (the wave index through readfirstlane: row offsets are then wave-uniform, a scalar base + the lane's column per access)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
    const int k0 = wave * RPW;
    const float nan = __builtin_nanf("");
    float lacc = 0.f;
    float inv_n = inv_n_arg, eps = 0.f;
    if constexpr (WT) { inv_n = win.den[1]; eps = win.smoothing; }
    if constexpr (WIN) {
        // the table from the kernel arguments into LDS, by constant indices (a lane-indexed read of the arguments would move the
        // table to scratch; a select per pair keeps 32 scalars alive across the tile and spills them)
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < WN_WIN_MAX; ++j) { s_win[j] = win.lo[j]; s_win[WN_WIN_MAX + j] = win.hi[j]; }
        }
        __syncthreads();
    }
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int b = (int)(tile / tiles_per_clip);
        const int c0 = (int)(tile - (long)b * tiles_per_clip) * 64, c = c0 + lane;
        const bool cv = c < w;                                   // columns >= w are neither read nor written
        const long col = (long)b * w + c;
        long y = -1;
        if (cv && target) y = target[col];
        bool bad = (unsigned long)y >= (unsigned long)q;
        int lo = 0, hi = q;
        if constexpr (WIN) {
            // the clip's position mod period without a 64-bit division: p = h 2^32 + l, pow32 = 2^32 mod period (from the host).
            // A negative position poisons the clip's columns and picks no pair.
            const long pb = win.pos ? win.pos[b] : 0;
            const unsigned P = (unsigned)win.period;
            const unsigned base = win.pos0 + (((unsigned)((unsigned long)pb >> 32) % P) * win.pow32 + (unsigned)pb % P) % P;
            const unsigned jw = (base + (unsigned)c) % P;
            if (pb >= 0 && cv) { lo = s_win[jw]; hi = s_win[WN_WIN_MAX + jw]; }
            bad = bad || pb < 0 || y < lo || y >= hi;
        }
        float wv = 1.f, en = 0.f, sm = 0.f;                       // smoothing: eps / n per row of the window, eps / n * sum of its logits
        bool skip = false;
        if constexpr (WT) {
            if (cv) wv = nll_weight(win.weight, target, win.ignore, col);
            skip = wv == 0.f;                                     // (a NaN weight is counted: it poisons the column, and den with it)
        }
        const float* xr = x + b * x_bs + (long)k0 * x_pitch + c0;       // row k0 of this tile, wave-uniform
        float v[RPW];
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
            const int k = k0 + j;
            if constexpr (WIN) v[j] = ((unsigned)(k - lo) < (unsigned)(hi - lo)) ? (cv ? xr[lane] : 0.f) : -INFINITY;      // (hi <= q)
            else v[j] = (Q256 || k < q) ? (cv ? xr[lane] : 0.f) : -INFINITY;
            xr += x_pitch;
        }
        // this wave's max, its first index, and the target's logit if it is one of these rows
        float m = v[0], xy = 0.f;
        int a = 0;
#pragma unroll
        for (int j = 1; j < RPW; ++j)
            if (v[j] > m) { m = v[j]; a = j; }
        int yj = bad ? -1 : (int)y - k0;                          // the target's row among this wave's, if in [0, RPW)
#pragma unroll
        for (int j = 0; j < RPW; ++j)
            if (j == yj) xy = v[j];
        s_max[wave][lane] = m;
        s_arg[wave][lane] = k0 + a;
        if (yj >= 0 && yj < RPW) s_xy[lane] = xy;
        if constexpr (WT) {
            if (eps != 0.f) {                                    // this wave's share of the sum of the window's logits
                float x4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < RPW; ++j)
                    if ((unsigned)(k0 + j - lo) < (unsigned)(hi - lo)) x4[j & 3] += v[j];
                s_sx[wave][lane] = (x4[0] + x4[1]) + (x4[2] + x4[3]);
            }
        }
        // (hides yj's value from the optimiser: it would otherwise keep the RPW compare masks above alive in scalar registers for
        // the gradient loop below, and spill them)
        asm volatile("" : "+v"(yj));
        __syncthreads();
        float M = s_max[0][lane];
        int A = s_arg[0][lane];
        for (int i = 1; i < nw; ++i) {                           // rows ascend with the wave: '>' keeps the first index of a tie
            const float mi = s_max[i][lane];
            if (mi > M) { M = mi; A = s_arg[i][lane]; }
        }
        xy = s_xy[lane];                                         // (never written for a bad target: replaced by NaN below)
        if constexpr (WT) {
            if (eps != 0.f) {
                en = eps / (float)(hi - lo);
                float sx = 0.f;
                for (int i = 0; i < nw; ++i) sx += s_sx[i][lane];
                sm = en * sx;
            }
        }
        float s4[4] = {0.f, 0.f, 0.f, 0.f};                      // four short chains: less rounding than one of RPW terms
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
            v[j] = expf(v[j] - M);
            s4[j & 3] += v[j];
        }
        s_sum[wave][lane] = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        __syncthreads();
        float S = 0.f;
        for (int i = 0; i < nw; ++i) S += s_sum[i][lane];       // the same order in every wave: one S per column
        const float inv = 1.0f / S;
        if (wave == 0 && cv && target) {
            const float nll = bad ? nan : logf(S) + (M - xy);
            if constexpr (WT) {
                if (row_nll) row_nll[col] = skip ? 0.f : nll;
                if (row_hit) row_hit[col] = (!skip && !bad && A == (int)y) ? 1 : 0;
                if (!skip) lacc += wv * (eps != 0.f ? (bad ? nan : logf(S) + (M - (1.f - eps) * xy) - sm) : nll);
            } else {
                if (row_nll) row_nll[col] = nll;
                if (row_hit) row_hit[col] = (!bad && A == (int)y) ? 1 : 0;
                lacc += nll;
            }
        }
        if (dx && cv) {
            float* dr = dx + b * dx_bs + (long)k0 * dx_pitch + c0;
#pragma unroll
            for (int j = 0; j < RPW; ++j) {
                const int k = k0 + j;
                if constexpr (WT) {
                    // (eps == 0: the subtrahends are 1 and 0, and x - 0 is x: the expression above to the bit)
                    const float in = (unsigned)(k - lo) < (unsigned)(hi - lo) ? en : 0.f;
                    const float g = bad ? nan : ((v[j] * inv - (j == yj ? 1.f - eps : 0.f)) - in) * (wv * inv_n);
                    if (Q256 || k < q) dr[lane] = skip ? 0.f : g;
                } else if (Q256 || k < q) dr[lane] = bad ? nan : (v[j] * inv - (j == yj ? 1.f : 0.f)) * inv_n;
                dr += dx_pitch;
            }
        }
        if (probs) {                                             // (a kernel argument: every wave takes this branch or none)
            float* t = s_t[wave];
            const int tc = lane / TR, tr = lane % TR;
#pragma unroll
            for (int p = 0; p < RPW / TR; ++p) {
#pragma unroll
                for (int r = 0; r < TR; ++r) t[lane * TP + r] = v[p * TR + r] * inv;
                __syncthreads();
                const int k = k0 + p * TR + tr;
#pragma unroll
                for (int i = 0; i < TR; ++i) {
                    const int cc = i * (64 / TR) + tc;
                    if (c0 + cc < w && (Q256 || k < q)) probs[((long)b * w + c0 + cc) * q + k] = t[cc * TP + tr];
                }
                __syncthreads();
            }
        }
    }
    if (wave == 0 && loss_part) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lacc += __shfl_xor(lacc, o, 64);
        if (lane == 0) {
            loss_part[blockIdx.x] = lacc * inv_n;
            for (int i = blockIdx.x + gridDim.x; i < WN_CE_PARTIALS; i += gridDim.x) loss_part[i] = 0.f;   // all slots, every call
        }
    }
}

// target NULL: the softmax alone (wn_step_softmax; nothing but probs is written).  win NULL (or of period 0): the instantiations without
// windows.  wt (NULL: none; needs a target): the WT instantiations behind nll_den_k, inv_n unused.  The caller has checked the arguments.
template <bool WIN, bool WT, class Win>
static void step_nll_launch(int grid, dim3 block, hipStream_t st, const float* x, long x_bs, int x_pitch, const int64_t* target, float* dx,
                            long dx_bs, int dx_pitch, float* probs, float* row_nll, int32_t* row_hit, float* loss_part, int w, int q,
                            int tiles_per_clip, long ntiles, float inv_n, const Win& win) {
    if (q == 256)
        hipLaunchKernelGGL((step_nll_k<64, 8, true, 256, WIN, WT>), dim3(grid), block, 0, st, x, x_bs, x_pitch, target, dx, dx_bs, dx_pitch,
                           probs, row_nll, row_hit, loss_part, w, q, tiles_per_clip, ntiles, inv_n, win);
    else if (q <= 512)
        hipLaunchKernelGGL((step_nll_k<64, 8, false, 512, WIN, WT>), dim3(grid), block, 0, st, x, x_bs, x_pitch, target, dx, dx_bs, dx_pitch,
                           probs, row_nll, row_hit, loss_part, w, q, tiles_per_clip, ntiles, inv_n, win);
    else          // (16 waves of 64 rows leave 128 registers a lane: this instantiation alone keeps part of its rows in scratch)
        hipLaunchKernelGGL((step_nll_k<64, 8, false, 1024, WIN, WT>), dim3(grid), block, 0, st, x, x_bs, x_pitch, target, dx, dx_bs, dx_pitch,
                           probs, row_nll, row_hit, loss_part, w, q, tiles_per_clip, ntiles, inv_n, win);
}

int wn_launch_step_nll(const float* x, long x_bs, int x_pitch, const int64_t* target, float* dx, long dx_bs, int dx_pitch, float* probs,
                       float* row_nll, int32_t* row_hit, float* loss_part, int w, int q, int batch, float inv_n, const WnNllWin* win,
                       const WnNllWt* wt, hipStream_t st) {
    if (batch <= 0 || w <= 0) {
        if (loss_part) {
            hipError_t e = hipMemsetAsync(loss_part, 0, WN_CE_PARTIALS * sizeof(float), st);
            if (e != hipSuccess) return wn_set_error(e, __FILE__, __LINE__);
        }
        if (wt && wt->den) {
            hipError_t e = hipMemsetAsync(wt->den, 0, 2 * sizeof(float), st);
            if (e != hipSuccess) return wn_set_error(e, __FILE__, __LINE__);
        }
        return 0;
    }
    const int tiles_per_clip = (w + 63) / 64;
    const long ntiles = (long)batch * tiles_per_clip;
    // a bounded grid whose blocks all take the same number of tiles (+-1), one loss partial per block
    const long rounds = (ntiles + WN_CE_PARTIALS - 1) / WN_CE_PARTIALS;
    const int grid = (int)((ntiles + rounds - 1) / rounds);
    const dim3 block(64 * ((q + 63) / 64));
    if (wt) {
        // the weights' sum first, in a launch of its own: the main kernel reads den[1] behind it on the same stream
        hipLaunchKernelGGL(nll_den_k, dim3(1), dim3(1024), 0, st, wt->weight, target, (long)wt->ignore, (long)batch * w, wt->den);
        WN_CHECK_LAUNCH();
        if (win && win->period > 0) {
            WnNllWtArgs<true> a;
            static_cast<WnNllWin&>(a) = *win;
            a.weight = wt->weight; a.den = wt->den; a.ignore = (long)wt->ignore; a.smoothing = wt->smoothing;
            step_nll_launch<true, true>(grid, block, st, x, x_bs, x_pitch, target, dx, dx_bs, dx_pitch, probs, row_nll, row_hit, loss_part, w,
                                        q, tiles_per_clip, ntiles, 0.f, a);
        } else {
            WnNllWtArgs<false> a;
            a.weight = wt->weight; a.den = wt->den; a.ignore = (long)wt->ignore; a.smoothing = wt->smoothing;
            step_nll_launch<false, true>(grid, block, st, x, x_bs, x_pitch, target, dx, dx_bs, dx_pitch, probs, row_nll, row_hit, loss_part,
                                         w, q, tiles_per_clip, ntiles, 0.f, a);
        }
    } else if (win && win->period > 0)
        step_nll_launch<true, false>(grid, block, st, x, x_bs, x_pitch, target, dx, dx_bs, dx_pitch, probs, row_nll, row_hit, loss_part, w, q,
                              tiles_per_clip, ntiles, inv_n, *win);
    else
        step_nll_launch<false, false>(grid, block, st, x, x_bs, x_pitch, target, dx, dx_bs, dx_pitch, probs, row_nll, row_hit, loss_part, w,
                                      q, tiles_per_clip, ntiles, inv_n, WnNoWin());
    WN_CHECK_LAUNCH();
    return 0;
}
