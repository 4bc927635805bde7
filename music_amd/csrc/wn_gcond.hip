// The learned conditioning projections WITH a global class term (wn_gcond_proj_fwd / wn_gcond_proj_bwd in include/wavenet_hip.h):
// clip b of class cls[b] gains, in every stage's table, G_i emb[cls[b]] - constant over the clip's frames (VQ-VAE's speaker id, van
// den Oord et al. 2017, section 4.3; NSynth's instrument and pitch).  G_i [2 Dd][E] per block and G_f [Sd][E] stack to R rows like W.
//
//   forward    out[r][col] = (bias[r] + sum_k W[r][k] enc[k][col]) + sum_e G[r][e] emb[cls[b(col)]][e]      (cond_gemm_k<0, WnGcond>)
//   dW, db, dG dG[r][e]    = sum_col d[r][col] emb[cls[b(col)]][e]: column tiles behind dW's, the same rows     (cond_gemm_k<1, WnGcond>)
//   d enc      the learned projections' kernel, unchanged                                                        (wn_launch_cond_denc)
//   d emb      demb[m][e]  = sum_{b: cls[b] = m, ascending} sum_r G[r][e] (sum_l d[r][b][l])                      (gcond_demb_k)
//
// The products are wn_condproj.h's kernel with the global term's arguments.  d emb has n_cls E outputs and a long K (R Le per clip):
// one workgroup per class walks its clips in ascending order; per clip its 1024 threads first reduce R rows over the frames into LDS
// (one row each, a chunk of 1024 rows at a time, beside the offset of that row of G), then wave w takes rows [64 w, 64 w + 64) of the
// chunk against G - lane = e (+ 64 j: E <= 512 is 8 accumulators), G's rows read whole, the row sum a broadcast out of LDS, the loop
// free of branches so that 16 rows' loads are in flight together (a workgroup per class is few compute units: the launch is bound by
// the loads each keeps in flight) - and the 16 waves' partials are added through LDS in wave order.  fp32 FMA, a fixed summation
// order, no atomics: the same bits on every launch.  A class outside [0, n_cls) is never used as an index: the forward's columns of
// that clip and its share of dG become NaN, d emb (which has no row for it) ignores the clip.
//
// The global term ALONE (wn_gclass_fwd / wn_gclass_bwd: a class-conditional WaveNet has no encoding, its tables one column per clip):
//   forward    tab[.][b] = sum_e G[r][e] emb[cls[b]][e], the padding rows' zeros and enf in one launch: a thread per (table row, clip)
//              runs cond_gemm_k's second reduction - e ascending from +0, one FMA each - so the bits are that kernel's       (gclass_fwd_k)
//   dG         dG[r][e]  = sum_b d[r][b] emb[cls[b]][e], b ascending: a thread per (r, e), cond_gemm_k<1>'s dG tile            (gclass_dg_k)
//   d emb      gcond_demb_k with le = 1
#include "wn_condproj.h"

namespace {

constexpr int GRC = 1024, GNW = GRC / 64;     // gcond_demb_k: rows per chunk = threads, waves
constexpr int GJ = WN_GCOND_MAX_E / 64;       // accumulators per lane

// 64 rows of G against their row sums, NJ = ceil(ge / 64) accumulators per lane.  No branch in the loop - a lane behind ge reads
// element ge - 1 and its sums are never stored - so the loads of a group of rows are in flight together.
template <int NJ>
__device__ __forceinline__ void demb_rows(const float* flat, const float* s_row, const long* s_go, int lane, int ge, float* acc) {
    int e[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) e[j] = min(lane + 64 * j, ge - 1);
#pragma unroll 16
    for (int q = 0; q < 64; ++q) {
        const float sv = s_row[q];
        const float* gr = flat + s_go[q];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = fmaf(gr[e[j]], sv, acc[j]);
    }
}

__global__ __launch_bounds__(GRC) void gcond_demb_k(WnCondProj p, WnGcond g) {
    __shared__ float s_row[GRC];
    __shared__ long s_go[GRC];
    __shared__ float s_part[GNW][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int R = p.n_stages * 2 * p.dd + p.sd, m = blockIdx.x;
    float acc[GJ];
#pragma unroll
    for (int j = 0; j < GJ; ++j) acc[j] = 0.f;
    for (int b = 0; b < p.batch; ++b) {
        if (g.cls[b] != m) continue;                          // (the same for every thread of the workgroup)
        for (int r0 = 0; r0 < R; r0 += GRC) {
            // thread t: row r0 + t of clip b summed over its frames, and where that row of G starts - both into LDS
            const int r = r0 + (int)threadIdx.x;
            float s = 0.f;
            long go = g.gw_off;                               // (a row behind the last one: 0 x G's first row, which every class reads anyway)
            if (r < R) {
                int i, c;
                row_of(p, r, i, c);
                go = g_row(p, g, i, c);
                const float* src = i == p.n_stages ? p.d_enf + ((long)b * p.sd + c) * p.le
                                                   : p.d_tab + tab_row(p, p.d_pair, i, c) + tab_col(p, p.d_pair, b, 0);
#pragma unroll 8
                for (int l = 0; l < p.le; ++l) s += src[l];
            }
            s_row[threadIdx.x] = s;
            s_go[threadIdx.x] = go;
            __syncthreads();
            // wave w: rows [64 w, 64 w + 64) of the chunk against G
            switch ((g.ge + 63) / 64) {                       // (uniform)
                case 1: demb_rows<1>(p.flat, s_row + wave * 64, s_go + wave * 64, lane, g.ge, acc); break;
                case 2: demb_rows<2>(p.flat, s_row + wave * 64, s_go + wave * 64, lane, g.ge, acc); break;
                case 3: demb_rows<3>(p.flat, s_row + wave * 64, s_go + wave * 64, lane, g.ge, acc); break;
                case 4: demb_rows<4>(p.flat, s_row + wave * 64, s_go + wave * 64, lane, g.ge, acc); break;
                default: demb_rows<GJ>(p.flat, s_row + wave * 64, s_go + wave * 64, lane, g.ge, acc); break;
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int j = 0; j < GJ; ++j) {
        if (64 * j >= g.ge) break;                            // (uniform)
        s_part[wave][lane] = acc[j];
        __syncthreads();
        if (wave == 0 && lane + 64 * j < g.ge) {
            float s = s_part[0][lane];
            for (int w = 1; w < GNW; ++w) s += s_part[w][lane];
            p.flat_grad[g.emb_off + (long)m * g.ge + lane + 64 * j] = s;
        }
        __syncthreads();
    }
}

// The global term alone, le = 1.  Thread (rt, b): row rt of the 2 ch rows of stage rt / (2 ch) - filter half first, as the tables
// have them - or, behind the stages, row rt - n_stages 2 ch of enf; clips fastest, so that a wave reads few rows of G.
__global__ __launch_bounds__(256) void gclass_fwd_k(WnCondProj p, WnGcond g, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int b = (int)(idx % p.batch), rt = (int)(idx / p.batch), nt = p.n_stages * 2 * p.ch;
    int i = p.n_stages, c = rt - nt, half = 0, cc = 0;
    if (rt < nt) {
        i = rt / (2 * p.ch);
        const int rr = rt - i * 2 * p.ch;
        half = rr / p.ch; cc = rr - half * p.ch;
        c = half ? cc : p.dd + cc;                            // the reference's row: gate rows [0, dd), filter rows [dd, 2 dd)
    }
    float acc = 0.f;
    if (i == p.n_stages || cc < p.dd) {
        const float* gr = p.flat + g_row(p, g, i, c);
        const long er = emb_row(g, b);
        const float* em = p.flat + (er >= 0 ? er : 0);
#pragma unroll 8
        for (int e = 0; e < g.ge; ++e) acc = fmaf(gr[e], er >= 0 ? em[e] : __builtin_nanf(""), acc);
    }
    if (i == p.n_stages) { p.enf[(long)b * p.sd + c] = acc; return; }
    if (p.tab) p.tab[((long)i * p.batch + b) * 2 * p.ch + half * p.ch + cc] = acc;
    if (p.tab_pair) p.tab_pair[((long)i * (p.batch / 2) + (b >> 1)) * 4 * p.ch + half * 2 * p.ch + (b & 1) * p.ch + cc] = acc;
}

// dG: thread (r, e), e fastest (the embedding rows and the stores coalesce); clips in ascending order
__global__ __launch_bounds__(256) void gclass_dg_k(WnCondProj p, WnGcond g, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int e = (int)(idx % g.ge), r = (int)(idx / g.ge);
    int i, c;
    row_of(p, r, i, c);
    const float* src = i == p.n_stages ? p.d_enf + c : p.d_tab + tab_row(p, p.d_pair, i, c);
    float acc = 0.f;
    for (int b = 0; b < p.batch; ++b) {
        const float d = i == p.n_stages ? src[(long)b * p.sd] : src[tab_col(p, p.d_pair, b, 0)];
        const long er = emb_row(g, b);
        acc = fmaf(d, er >= 0 ? p.flat[er + e] : __builtin_nanf(""), acc);
    }
    p.flat_grad[g_row(p, g, i, c) + e] = acc;
}

}  // namespace

// The callers (wn_api.hip) have checked the arguments.
int wn_launch_gclass_fwd(const WnCondProj& p, const WnGcond& g, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const long total = ((long)p.n_stages * 2 * p.ch + p.sd) * p.batch, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) return wn_set_error_msg(-4, "wn_gclass_fwd: the tables have too many elements for one grid");
    hipLaunchKernelGGL(gclass_fwd_k, dim3((unsigned)blocks), dim3(256), 0, st, p, g, total);
    WN_CHECK_LAUNCH();
    return 0;
}

int wn_launch_gclass_bwd(const WnCondProj& p, const WnGcond& g, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const long total = ((long)p.n_stages * 2 * p.dd + p.sd) * g.ge, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) return wn_set_error_msg(-4, "wn_gclass_bwd: the projections have too many elements for one grid");
    hipLaunchKernelGGL(gclass_dg_k, dim3((unsigned)blocks), dim3(256), 0, st, p, g, total);
    WN_CHECK_LAUNCH();
    hipLaunchKernelGGL(gcond_demb_k, dim3((unsigned)g.n_cls), dim3(GRC), 0, st, p, g);
    WN_CHECK_LAUNCH();
    return 0;
}

int wn_launch_gcond_proj_fwd(const WnCondProj& p, const WnGcond& g, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const long R = (long)p.n_stages * 2 * p.dd + p.sd, C = (long)p.batch * p.le;
    const int tiles_n = (int)((C + TN - 1) / TN);
    const long gemm_blocks = (R + TM - 1) / TM * tiles_n;
    const long pad = (long)p.n_stages * p.batch * 2 * (p.ch - p.dd) * p.le;
    const long pad_blocks = pad ? std::min<long>((pad + 1023) / 1024, 256) : 0;
    if (gemm_blocks + pad_blocks > 0x7fffffffL) return wn_set_error_msg(-4, "wn_gcond_proj_fwd: the product has too many tiles for one grid");
    hipLaunchKernelGGL((cond_gemm_k<0, WnGcond>), dim3((unsigned)(gemm_blocks + pad_blocks)), dim3(256), 0, st, p, tiles_n, (int)gemm_blocks, g);
    WN_CHECK_LAUNCH();
    return 0;
}

int wn_launch_gcond_proj_bwd(const WnCondProj& p, const WnGcond& g, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const long R = (long)p.n_stages * 2 * p.dd + p.sd;
    const int tiles_n = (p.bw + TN - 1) / TN + (g.ge + TN - 1) / TN;
    const long gemm_blocks = (R + TM - 1) / TM * tiles_n;
    if (gemm_blocks > 0x7fffffffL || !wn_cond_denc_fits(p))
        return wn_set_error_msg(-4, "wn_gcond_proj_bwd: the product has too many tiles for one grid");
    hipLaunchKernelGGL((cond_gemm_k<1, WnGcond>), dim3((unsigned)gemm_blocks), dim3(256), 0, st, p, tiles_n, (int)gemm_blocks, g);
    WN_CHECK_LAUNCH();
    if (int rc = wn_launch_cond_denc(p, st)) return rc;
    hipLaunchKernelGGL(gcond_demb_k, dim3((unsigned)g.n_cls), dim3(GRC), 0, st, p, g);
    WN_CHECK_LAUNCH();
    return 0;
}
