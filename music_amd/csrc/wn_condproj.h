// What wn_condproj.hip (the learned projections) and wn_gcond.hip (the same with a global class term) share: the index rules of the
// flat buffers and the block tables, and the 32 x 64 LDS-tiled product kernel both build their forward tables and weight gradients with.
// GC = false is the learned projections' product alone: every GC branch is compiled out of it.
#pragma once
#include "wn_common.h"
#include "wn_kernels.h"

namespace {

constexpr int TM = 32, TN = 64, KT = 16;      // product tile of cond_gemm_k, 256 threads
constexpr int AP = TM + 1, BP = TN + 4;       // LDS row pitches: A written k-fastest (odd pitch), B read as float4 (16-byte rows)

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
// row (stage i, reference row c) of the global projections G: [ge] floats of flat / flat_grad
__device__ __forceinline__ long g_row(const WnCondProj& p, const WnGcond& g, int i, int c) {
    return (i < p.n_stages ? g.gw_off + i * g.gstage_stride : g.gwf_off) + (long)c * g.ge;
}
// clip b's embedding row in flat, or -1: its class lies outside [0, n_cls) and nothing is read for it
__device__ __forceinline__ long emb_row(const WnGcond& g, int b) {
    const int m = g.cls[b];
    return m >= 0 && m < g.n_cls ? g.emb_off + (long)m * g.ge : -1;
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
// GC, MODE 0: a second reduction, over the ge channels of G and of each column's clip's embedding row, in an accumulator of its own:
// out = (bias + sum_k W enc) + sum_e G emb.  GC, MODE 1: the column tiles behind dW's are dG's, the same rows of d against emb[cls[b]].
// The global term's arguments are a parameter pack of none (GC = false: the learned projections' kernel, its arguments unchanged) or one.
__device__ __forceinline__ WnGcond gcond_of() { return WnGcond{}; }
__device__ __forceinline__ const WnGcond& gcond_of(const WnGcond& g) { return g; }
template <int MODE, class... G>
__global__ __launch_bounds__(256) void cond_gemm_k(WnCondProj p, int tiles_n, int gemm_blocks, G... gs) {
    constexpr bool GC = sizeof...(G) > 0;
    const WnGcond g = gcond_of(gs...);
    __shared__ float As[KT][AP];
    __shared__ __attribute__((aligned(16))) float Bs[KT][BP];
    const int t = threadIdx.x;
    const int R = p.n_stages * 2 * p.dd + p.sd, C = p.batch * p.le;
    if (MODE == 0 && (int)blockIdx.x >= gemm_blocks) {
        // rows [Dd, CH) of every CH-row group of every table: zeros (the same index formula serves both layouts)
        const int pr = p.ch - p.dd;
        const long per = (long)pr * p.le, total = (long)p.n_stages * p.batch * 2 * per;
        for (long e = (long)(blockIdx.x - gemm_blocks) * 256 + t; e < total; e += (long)(gridDim.x - gemm_blocks) * 256) {
            const long gi = e / per, o = e - gi * per;
            const long dst = gi * p.ch * p.le + (long)p.dd * p.le + o;
            if (p.tab) p.tab[dst] = 0.f;
            if (p.tab_pair) p.tab_pair[dst] = 0.f;
        }
        return;
    }
    const int tn = blockIdx.x % tiles_n, tiles_w = (p.bw + TN - 1) / TN;
    const bool gt = GC && MODE == 1 && tn >= tiles_w;          // a tile of dG
    const int m0 = (blockIdx.x / tiles_n) * TM, n0 = (gt ? tn - tiles_w : tn) * TN;
    const int Nn = MODE == 0 ? C : gt ? g.ge : p.bw, K = MODE == 0 ? p.bw : C;
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
                ce = gt ? emb_row(g, b) : (long)b * p.bw * p.le + l;
            }
            for (int q = 0; q < 2; ++q)
                As[ak][(t >> 4) + 16 * q] = (a_base[q] >= 0 && cd >= 0) ? (a_fin[q] ? p.d_enf[a_base[q] + cf] : p.d_tab[a_base[q] + cd]) : 0.f;
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + (t >> 4) + 16 * q;
                if (gt) Bs[ak][(t >> 4) + 16 * q] = (cd >= 0 && n < Nn) ? (ce >= 0 ? p.flat[ce + n] : __builtin_nanf("")) : 0.f;
                else Bs[ak][(t >> 4) + 16 * q] = (cd >= 0 && n < Nn) ? p.enc[ce + (long)n * p.le] : 0.f;
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
    float gacc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (GC && MODE == 0) {
        // the global term: A = G's rows, B[e][col] = emb[cls[clip of col]][e] (NaN where the class is out of range: nothing is read)
        long ga[2], ge_base = -1;
        bool col_ok = false;
        for (int q = 0; q < 2; ++q) {
            const int r = m0 + (t >> 4) + 16 * q;
            ga[q] = -1;
            if (r < R) { int i, c; row_of(p, r, i, c); ga[q] = g_row(p, g, i, c); }
        }
        {
            const int col = n0 + (t & 63);
            if (col < C) { col_ok = true; ge_base = emb_row(g, col / p.le); }
        }
        for (int k0 = 0; k0 < g.ge; k0 += KT) {
            const int kk = k0 + ak;
            for (int q = 0; q < 2; ++q)
                As[ak][(t >> 4) + 16 * q] = (ga[q] >= 0 && kk < g.ge) ? p.flat[ga[q] + kk] : 0.f;
            for (int q = 0; q < 4; ++q) {
                const int k = k0 + (t >> 6) + 4 * q;
                Bs[(t >> 6) + 4 * q][t & 63] = (col_ok && k < g.ge) ? (ge_base >= 0 ? p.flat[ge_base + k] : __builtin_nanf("")) : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const float a0 = As[k][2 * ty], a1 = As[k][2 * ty + 1];
                const float4 b = *reinterpret_cast<const float4*>(&Bs[k][4 * tx]);
                gacc[0][0] = fmaf(a0, b.x, gacc[0][0]); gacc[0][1] = fmaf(a0, b.y, gacc[0][1]);
                gacc[0][2] = fmaf(a0, b.z, gacc[0][2]); gacc[0][3] = fmaf(a0, b.w, gacc[0][3]);
                gacc[1][0] = fmaf(a1, b.x, gacc[1][0]); gacc[1][1] = fmaf(a1, b.y, gacc[1][1]);
                gacc[1][2] = fmaf(a1, b.z, gacc[1][2]); gacc[1][3] = fmaf(a1, b.w, gacc[1][3]);
            }
            __syncthreads();
        }
    }
    for (int q = 0; q < 2; ++q) {
        const int r = m0 + 2 * ty + q;
        if (r >= R) continue;
        int i, c;
        row_of(p, r, i, c);
        if (MODE == 1) {
            const long wo = gt ? g_row(p, g, i, c) : w_row(p, i, c);
            for (int j = 0; j < 4; ++j)
                if (n0 + 4 * tx + j < Nn) p.flat_grad[wo + n0 + 4 * tx + j] = acc[q][j];
            if (!gt && n0 == 0 && tx == 0) p.flat_grad[b_row(p, i, c)] = bsum[q];
            continue;
        }
        const float bias = p.flat[b_row(p, i, c)];
        for (int j = 0; j < 4; ++j) {
            const int col = n0 + 4 * tx + j;
            if (col >= C) continue;
            const int b = col / p.le, l = col - b * p.le;
            const float v = GC ? (acc[q][j] + bias) + gacc[q][j] : acc[q][j] + bias;
            if (i == p.n_stages) p.enf[((long)b * p.sd + c) * p.le + l] = v;
            else {
                if (p.tab) p.tab[tab_row(p, 0, i, c) + tab_col(p, 0, b, l)] = v;
                if (p.tab_pair) p.tab_pair[tab_row(p, 1, i, c) + tab_col(p, 1, b, l)] = v;
            }
        }
    }
}

}  // namespace
