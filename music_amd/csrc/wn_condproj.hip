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
#include "wn_common.h"
#include "wn_kernels.h"

namespace {

constexpr int TM = 32, TN = 64, KT = 16;      // product tile of cond_gemm_k, 256 threads
constexpr int AP = TM + 1, BP = TN + 4;       // LDS row pitches: A written k-fastest (odd pitch), B read as float4 (16-byte rows)
constexpr int DCT = 8, DNW = 16;              // cond_denc_k: columns per workgroup, waves (K splits) per workgroup

// row r of the stacked product: its stage (N = the final one) and the reference's row c inside it
__device__ __forceinline__ void row_of(const WnCondProj& p, int r, int& i, int& c) {
    const int n2 = p.n_stages * 2 * p.dd;
    if (r < n2) { i = r / (2 * p.dd); c = r - i * 2 * p.dd; }
    else { i = p.n_stages; c = r - n2; }
}
__device__ __forceinline__ long w_row(const WnCondProj& p, int i, int c) {
    return (i < p.n_stages ? p.w_off + i * p.stage_stride : p.wf_off) + (long)c * p.bw;
}
__device__ __forceinline__ long b_row(const WnCondProj& p, int i, int c) {
    return (i < p.n_stages ? p.b_off + i * p.stage_stride : p.bf_off) + c;
}
// element (stage i, reference row c, clip b, frame l) of a block table = tab_row + tab_col: gate rows c < Dd behind the filter rows
__device__ __forceinline__ long tab_row(const WnCondProj& p, int pair, int i, int c) {
    const int rows = pair ? 4 * p.ch : 2 * p.ch, nt = pair ? p.batch / 2 : p.batch;
    const int row = c < p.dd ? (pair ? 2 * p.ch : p.ch) + c : c - p.dd;
    return ((long)i * nt * rows + row) * p.le;
}
__device__ __forceinline__ long tab_col(const WnCondProj& p, int pair, int b, int l) {
    const int rows = pair ? 4 * p.ch : 2 * p.ch;
    return pair ? ((long)(b >> 1) * rows + (b & 1) * p.ch) * p.le + l : (long)b * rows * p.le + l;
}

// MODE 0: the forward tables; MODE 1: dW and db into flat_grad.  Blocks behind the product's tiles (MODE 0) write the padding rows.
template <int MODE>
__global__ __launch_bounds__(256) void cond_gemm_k(WnCondProj p, int tiles_n, int gemm_blocks) {
    __shared__ float As[KT][AP];
    __shared__ __attribute__((aligned(16))) float Bs[KT][BP];
    const int t = threadIdx.x;
    const int R = p.n_stages * 2 * p.dd + p.sd, C = p.batch * p.le;
    if (MODE == 0 && (int)blockIdx.x >= gemm_blocks) {
        // rows [Dd, CH) of every CH-row group of every table: zeros (the same index formula serves both layouts)
        const int pr = p.ch - p.dd;
        const long per = (long)pr * p.le, total = (long)p.n_stages * p.batch * 2 * per;
        for (long e = (long)(blockIdx.x - gemm_blocks) * 256 + t; e < total; e += (long)(gridDim.x - gemm_blocks) * 256) {
            const long g = e / per, o = e - g * per;
            const long dst = g * p.ch * p.le + (long)p.dd * p.le + o;
            if (p.tab) p.tab[dst] = 0.f;
            if (p.tab_pair) p.tab_pair[dst] = 0.f;
        }
        return;
    }
    const int m0 = (blockIdx.x / tiles_n) * TM, n0 = (blockIdx.x % tiles_n) * TN;
    const int Nn = MODE == 0 ? C : p.bw, K = MODE == 0 ? p.bw : C;
    const int ty = t >> 4, tx = t & 15;
    // the loaders: A rows t / 16 (+16), k = t % 16;  B (MODE 0): k = t / 64 (+4 ..), n = t % 64;  (MODE 1): kk = t % 16, n = t / 16 (+16 ..)
    const int ak = t & 15;
    long a_base[2];            // MODE 0: the row's weight offset; MODE 1: its gradient row's offset (-1: no such row)
    int a_fin[2];
    for (int q = 0; q < 2; ++q) {
        const int r = m0 + (t >> 4) + 16 * q;
        a_base[q] = -1; a_fin[q] = 0;
        if (r < R) {
            int i, c;
            row_of(p, r, i, c);
            a_fin[q] = i == p.n_stages;
            a_base[q] = MODE == 0 ? w_row(p, i, c) : (a_fin[q] ? (long)c * p.le : tab_row(p, p.d_pair, i, c));
        }
    }
    long b_base = -1;          // MODE 0: column n0 + t % 64 of the encoding
    if (MODE == 0) {
        const int col = n0 + (t & 63);
        if (col < C) { const int b = col / p.le; b_base = (long)b * p.bw * p.le + (col - b * p.le); }
    }
    float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, bsum[2] = {0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += KT) {
        const int kk = k0 + ak;
        if (MODE == 0) {
            for (int q = 0; q < 2; ++q)
                As[ak][(t >> 4) + 16 * q] = (a_base[q] >= 0 && kk < K) ? p.flat[a_base[q] + kk] : 0.f;
            for (int q = 0; q < 4; ++q) {
                const int k = k0 + (t >> 6) + 4 * q;
                Bs[(t >> 6) + 4 * q][t & 63] = (b_base >= 0 && k < K) ? p.enc[b_base + (long)k * p.le] : 0.f;
            }
        } else {
            // column kk = (clip b, frame l): the gradient's and the encoding's offsets of it
            long cd = -1, cf = 0, ce = 0;
            if (kk < K) {
                const int b = kk / p.le, l = kk - b * p.le;
                cd = tab_col(p, p.d_pair, b, l);
                cf = (long)b * p.sd * p.le + l;
                ce = (long)b * p.bw * p.le + l;
            }
            for (int q = 0; q < 2; ++q)
                As[ak][(t >> 4) + 16 * q] = (a_base[q] >= 0 && cd >= 0) ? (a_fin[q] ? p.d_enf[a_base[q] + cf] : p.d_tab[a_base[q] + cd]) : 0.f;
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + (t >> 4) + 16 * q;
                Bs[ak][(t >> 4) + 16 * q] = (cd >= 0 && n < Nn) ? p.enc[ce + (long)n * p.le] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const float a0 = As[k][2 * ty], a1 = As[k][2 * ty + 1];
            const float4 b = *reinterpret_cast<const float4*>(&Bs[k][4 * tx]);
            acc[0][0] = fmaf(a0, b.x, acc[0][0]); acc[0][1] = fmaf(a0, b.y, acc[0][1]);
            acc[0][2] = fmaf(a0, b.z, acc[0][2]); acc[0][3] = fmaf(a0, b.w, acc[0][3]);
            acc[1][0] = fmaf(a1, b.x, acc[1][0]); acc[1][1] = fmaf(a1, b.y, acc[1][1]);
            acc[1][2] = fmaf(a1, b.z, acc[1][2]); acc[1][3] = fmaf(a1, b.w, acc[1][3]);
            if (MODE == 1) { bsum[0] += a0; bsum[1] += a1; }
        }
        __syncthreads();
    }
    for (int q = 0; q < 2; ++q) {
        const int r = m0 + 2 * ty + q;
        if (r >= R) continue;
        int i, c;
        row_of(p, r, i, c);
        if (MODE == 1) {
            const long wo = w_row(p, i, c);
            for (int j = 0; j < 4; ++j)
                if (n0 + 4 * tx + j < Nn) p.flat_grad[wo + n0 + 4 * tx + j] = acc[q][j];
            if (n0 == 0 && tx == 0) p.flat_grad[b_row(p, i, c)] = bsum[q];
            continue;
        }
        const float bias = p.flat[b_row(p, i, c)];
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + 4 * tx + j;
            if (col >= C) continue;
            const int b = col / p.le, l = col - b * p.le;
            const float v = acc[q][j] + bias;
            if (i == p.n_stages) p.enf[((long)b * p.sd + c) * p.le + l] = v;
            else {
                if (p.tab) p.tab[tab_row(p, 0, i, c) + tab_col(p, 0, b, l)] = v;
                if (p.tab_pair) p.tab_pair[tab_row(p, 1, i, c) + tab_col(p, 1, b, l)] = v;
            }
        }
    }
}

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
    const long R = (long)p.n_stages * 2 * p.dd + p.sd, C = (long)p.batch * p.le;
    const int tiles_n = (p.bw + TN - 1) / TN;
    const long gemm_blocks = (R + TM - 1) / TM * tiles_n;
    const long col_tiles = (C + DCT - 1) / DCT;
    if (gemm_blocks > 0x7fffffffL || col_tiles > 0x7fffffffL || (p.bw + 63) / 64 > 65535)
        return wn_set_error_msg(-4, "wn_cond_proj_bwd: the product has too many tiles for one grid");
    hipLaunchKernelGGL(cond_gemm_k<1>, dim3((unsigned)gemm_blocks), dim3(256), 0, st, p, tiles_n, (int)gemm_blocks);
    WN_CHECK_LAUNCH();
    hipLaunchKernelGGL(cond_denc_k, dim3((unsigned)col_tiles, (p.bw + 63) / 64), dim3(64 * DNW), 0, st, p);
    WN_CHECK_LAUNCH();
    return 0;
}
