// The LEARNED conditioning projections of the autoencoder (wn_cond_proj_fwd / wn_cond_proj_bwd in include/wavenet_hip.h): the N + 1
// 1x1 convs of the pooled encoding, Conv1d(Bw -> 2 Dd) under every decoder block and Conv1d(Bw -> Sd) under connection_1
// (wavenet_autoencoder/model1.py:178-179, 216-217), as registered parameters of the flat buffer.  All stages are ONE product: the
// R = N 2Dd + Sd weight rows of every stage stacked, against the C = B Le columns (clip, frame) of the encoding.
//
//   forward    out[r][col] = bias[r] + sum_k W[r][k] enc[k][col]          M = R, N = C,  K = Bw     (cond_gemm_k<0>)
//   dW, db     dW[r][k]   = sum_col d[r][col] enc[k][col], db[r] = sum_col d[r][col]   M = R, N = Bw, K = C      (cond_gemm_k<1>)
//   d enc      denc[k][col] = sum_r W[r][k] d[r][col]                     M = Bw, N = C, K = R      (cond_denc_k)
//
// `out` and `d` live in the layouts the block kernels read and write (per clip [N][B][2CH][Le], rows [f | g]; clip pairs
// [N][B/2][4CH][Le], rows [f: A B | g: A B]) and in [B][Sd][Le] for the final stage; W and bias are read from (dW, db written to)
// the flat parameter (gradient) buffer at the stages' offsets.  fp32 FMA, a fixed summation order, no atomics: the same bits on
// every launch.  The first two are a 32 x 64 LDS-tiled product (K in steps of 16, a 2 x 4 register tile per thread); d enc has few
// outputs and a long K (Bw = 64 against R = 4096 at config 4), so each workgroup splits K over its 16 waves - lane = k (W rows are
// read whole, every lane of a wave reads the same d: a broadcast load) - and adds the 16 partial tiles through LDS in wave order.
#include "wn_condproj.h"

namespace {

constexpr int DCT = 8, DNW = 16;              // cond_denc_k: columns per workgroup, waves (K splits) per workgroup

// denc[b][k][l] = sum_r W[r][k] d[r][b][l]: workgroup = 64 values of k (the lanes) x DCT columns; wave w sums rows [w R/16, (w+1) R/16)
__global__ __launch_bounds__(64 * DNW) void cond_denc_k(WnCondProj p) {
    __shared__ float s_part[DNW][DCT][64];
    __shared__ long s_cd[DCT], s_cf[DCT], s_ce[DCT];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int R = p.n_stages * 2 * p.dd + p.sd, C = p.batch * p.le;
    const int k = blockIdx.y * 64 + lane, col0 = blockIdx.x * DCT;
    if (threadIdx.x < DCT) {
        // (a column behind the last one reads column col0's values; its sums are never stored)
        const int col = col0 + (int)threadIdx.x < C ? col0 + (int)threadIdx.x : col0;
        const int b = col / p.le, l = col - b * p.le;
        s_cd[threadIdx.x] = tab_col(p, p.d_pair, b, l);
        s_cf[threadIdx.x] = (long)b * p.sd * p.le + l;
        s_ce[threadIdx.x] = (long)b * p.bw * p.le + l;
    }
    __syncthreads();
    const int per = (R + DNW - 1) / DNW;
    const int r_lo = wave * per, r_hi = min(R, r_lo + per);
    float acc[DCT];
#pragma unroll
    for (int j = 0; j < DCT; ++j) acc[j] = 0.f;
    // the block stages' rows, then the final stage's: within either the column offsets are loop constants, read from LDS once
    const int n2 = p.n_stages * 2 * p.dd;
    {
        long co[DCT];
#pragma unroll
        for (int j = 0; j < DCT; ++j) co[j] = s_cd[j];
        const int r_b = min(r_hi, n2);
        int i = r_lo / (2 * p.dd), c = r_lo - i * 2 * p.dd;
#pragma unroll 4
        for (int r = r_lo; r < r_b; ++r) {
            const float w = k < p.bw ? p.flat[w_row(p, i, c) + k] : 0.f;
            const float* src = p.d_tab + tab_row(p, p.d_pair, i, c);
#pragma unroll
            for (int j = 0; j < DCT; ++j) acc[j] = fmaf(w, src[co[j]], acc[j]);
            if (++c == 2 * p.dd) { c = 0; ++i; }
        }
    }
    {
        long co[DCT];
#pragma unroll
        for (int j = 0; j < DCT; ++j) co[j] = s_cf[j];
#pragma unroll 4
        for (int r = max(r_lo, n2); r < r_hi; ++r) {
            const int c = r - n2;
            const float w = k < p.bw ? p.flat[p.wf_off + (long)c * p.bw + k] : 0.f;
            const float* src = p.d_enf + (long)c * p.le;
#pragma unroll
            for (int j = 0; j < DCT; ++j) acc[j] = fmaf(w, src[co[j]], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < DCT; ++j) s_part[wave][j][lane] = acc[j];
    __syncthreads();
    for (int o = threadIdx.x; o < DCT * 64; o += 64 * DNW) {
        const int j = o >> 6, ln = o & 63, kk = blockIdx.y * 64 + ln;
        float s = s_part[0][j][ln];
        for (int w = 1; w < DNW; ++w) s += s_part[w][j][ln];
        if (kk < p.bw && col0 + j < C) p.d_enc[s_ce[j] + (long)kk * p.le] = s;
    }
}

}  // namespace

// The callers (wn_api.hip) have checked the arguments.
int wn_launch_cond_proj_fwd(const WnCondProj& p, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const long R = (long)p.n_stages * 2 * p.dd + p.sd, C = (long)p.batch * p.le;
    const int tiles_n = (int)((C + TN - 1) / TN);
    const long gemm_blocks = (R + TM - 1) / TM * tiles_n;
    const long pad = (long)p.n_stages * p.batch * 2 * (p.ch - p.dd) * p.le;
    const long pad_blocks = pad ? std::min<long>((pad + 1023) / 1024, 256) : 0;
    if (gemm_blocks + pad_blocks > 0x7fffffffL) return wn_set_error_msg(-4, "wn_cond_proj_fwd: the product has too many tiles for one grid");
    hipLaunchKernelGGL(cond_gemm_k<0>, dim3((unsigned)(gemm_blocks + pad_blocks)), dim3(256), 0, st, p, tiles_n, (int)gemm_blocks);
    WN_CHECK_LAUNCH();
    return 0;
}

int wn_launch_cond_proj_bwd(const WnCondProj& p, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const long R = (long)p.n_stages * 2 * p.dd + p.sd;
    const int tiles_n = (p.bw + TN - 1) / TN;
    const long gemm_blocks = (R + TM - 1) / TM * tiles_n;
    if (gemm_blocks > 0x7fffffffL || !wn_cond_denc_fits(p))
        return wn_set_error_msg(-4, "wn_cond_proj_bwd: the product has too many tiles for one grid");
    hipLaunchKernelGGL(cond_gemm_k<1>, dim3((unsigned)gemm_blocks), dim3(256), 0, st, p, tiles_n, (int)gemm_blocks);
    WN_CHECK_LAUNCH();
    return wn_launch_cond_denc(p, st);
}

// d enc alone: the second launch of wn_cond_proj_bwd, and of wn_gcond_proj_bwd (wn_gcond.hip) - the same kernel, the same bits
bool wn_cond_denc_fits(const WnCondProj& p) {
    return ((long)p.batch * p.le + DCT - 1) / DCT <= 0x7fffffffL && (p.bw + 63) / 64 <= 65535;
}
int wn_launch_cond_denc(const WnCondProj& p, hipStream_t st) {
    const long col_tiles = ((long)p.batch * p.le + DCT - 1) / DCT;
    hipLaunchKernelGGL(cond_denc_k, dim3((unsigned)col_tiles, (p.bw + 63) / 64), dim3(64 * DNW), 0, st, p);
    WN_CHECK_LAUNCH();
    return 0;
}
