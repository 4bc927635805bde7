// The ONE copy of the flat optimizers' arithmetic, shared by the plain kernels (wn_elem.hip: adam_k, sgd_k, rmsprop_k) and the
// guarded ones (wn_guard.hip).  GUARDED only adds the clip coefficient to the gradient's scale; with GUARDED false the bodies are
// the plain kernels' loops as they always were (coef is not read).  i / stride: the calling kernel's first element and grid stride
// (taken in the kernel itself, where the compiler knows the workgroup size is uniform).  Below the optimizers: the exponential moving
// average of the parameters (wn_ema_flat, wn_guard.hip) that follows any of them.
#pragma once
#include <hip/hip_runtime.h>

// torch.optim.Adam: bc1 = 1 - b1^t, bc2 = 1 - b2^t
template <bool GUARDED>
__device__ __forceinline__ void wn_adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, long i, long stride, long n, float lr, float b1, float b2, float eps, float bc1,
                                             float bc2, float gscale, float coef) {
    const float step = lr / bc1, rs = 1.0f / sqrtf(bc2);
    for (; i < n; i += stride) {
        float gi = g[i] * gscale;
        if (GUARDED) gi *= coef;
        float mi = b1 * m[i] + (1.0f - b1) * gi;
        float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= step * mi / (sqrtf(vi) * rs + eps);
    }
}

//   SGD      buf = first ? g : momentum * buf + g ;  p -= lr * buf            (momentum == 0: p -= lr * g, buf untouched)
template <bool GUARDED>
__device__ __forceinline__ void wn_sgd_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long i, long stride,
                                            long n, float lr, float momentum, float gscale, int first, float coef) {
    for (; i < n; i += stride) {
        float gi = g[i] * gscale;
        if (GUARDED) gi *= coef;
        if (momentum != 0.f) {
            gi = first ? gi : buf[i] * momentum + gi;
            buf[i] = gi;
        }
        p[i] += -lr * gi;
    }
}

//   RMSprop  sq = alpha * sq + (1 - alpha) * g * g ; avg = sqrt(sq) + eps ;
//            momentum > 0: buf = momentum * buf + g / avg ; p -= lr * buf     else  p -= lr * g / avg
template <bool GUARDED>
__device__ __forceinline__ void wn_rmsprop_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq,
                                                float* __restrict__ buf, long i, long stride, long n, float lr, float alpha, float eps, float momentum,
                                                float gscale, float coef) {
    for (; i < n; i += stride) {
        float gi = g[i] * gscale;
        if (GUARDED) gi *= coef;
        const float s = sq[i] * alpha + ((1.0f - alpha) * gi) * gi;
        sq[i] = s;
        const float avg = sqrtf(s) + eps;
        if (momentum > 0.f) {
            const float b = buf[i] * momentum + gi / avg;
            buf[i] = b;
            p[i] += -lr * b;
        } else {
            p[i] += -lr * (gi / avg);
        }
    }
}

// EMA shadow weights: torch.optim.swa_utils.get_ema_avg_fn's lerp rule, ema += (1 - d_eff) * (p - ema), with TensorFlow's
// num_updates warm-up d_eff = min(decay, (1 + T) / (10 + T)).  The weight is formed in double from the float decay and rounded
// once (T below 1 counts as 1: an offset that went wrong must not divide by zero).
__device__ __forceinline__ float wn_ema_weight(float decay, int warmup, long T) {
    double d = (double)decay;
    if (warmup) {
        const double tt = (double)(T < 1 ? 1 : T);
        const double wu = (1.0 + tt) / (10.0 + tt);
        d = wu < d ? wu : d;
    }
    return 1.0f - (float)d;
}
__device__ __forceinline__ void wn_ema_body(float* __restrict__ ema, const float* __restrict__ p, long i, long stride, long n, float w) {
    for (; i < n; i += stride) {
        const float e = ema[i];
        ema[i] = e + w * (p[i] - e);
    }
}
