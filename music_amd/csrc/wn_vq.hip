// The vector-quantised bottleneck of the autoencoder (wn_vq_fwd / wn_vq_bwd / wn_vq_lookup in include/wavenet_hip.h): every pooled
// frame e[b][:, l] of enc [B][Bw][Le] is replaced by its nearest row of the codebook c [K][Bw], a parameter of the flat buffer.
//
//   forward   dist(frame, k) = sum_j (e_j - c_kj)^2 (the difference form: no cancellation), idx = the FIRST argmin over k,
//             q = c[idx] in enc's layout, counts[k] = frames of code k, loss_part = per-workgroup sums of the best distances / (C Bw)
//   backward  d_e = d_q + c_enc (e - q)   (straight-through + commitment),   d_c[k] = c_cb sum_{frames of k, ascending} (c_k - e)
//   lookup    q = c[idx] from given codes; an index outside [0, K) gives a NaN frame and raises *bad, it is never dereferenced
//
// The work is small and sits between encoder and decoder (C K Bw = 200 x 512 x 64 at config 4): few launches, every codebook row
// read once per workgroup and coalesced.  Forward: a workgroup stages FT frames in LDS, its NWV waves deal the codes out round-robin
// (ascending inside a wave, four per pass), lanes run along j; the FT per-lane sums of a code are folded over the wave by a transposing butterfly
// (7 exchanges for 4 sums instead of 24) that leaves frame f's distance in lanes [16 f, 16 f + 16); a strict < keeps the first
// minimum of a wave, and the waves' (distance, index) pairs are merged through LDS in wave order, lexicographically - the tie rule.
// Backward: one launch; the leading workgroups own 4 codes each (a wave per code walks idx in ascending frame order, 64 frames
// per ballot, and adds the matching frames: no scatter, no atomics), the others form d_e elementwise.  fp32, a fixed summation
// order, no float atomics: the same bits at every launch.  counts uses integer atomics on a buffer cleared by a memset node.
//
// EMA mode (wn_vq_bwd_stats / wn_vq_ema_update): the codebook follows the running mean of its frames instead of a gradient.
//   stats     the backward's launch with the code workgroups adding e instead of c_k - e: stat = [n | s], the frames per code (as
//             floats) and their sums in ascending frame order; the codebook's rows of flat_grad become exactly 0
//   update    N' = g N + (1 - g) n, m' = g m + (1 - g) s, c' = m' / Nhat with the usage smoothed by eps; a code whose N' fell
//             below `restart` takes the batch mean s / n of a donor (the d-th dead code, ascending, the d-th code by n descending).
// Two launches: ONE workgroup ranks the K codes (counting ranks over LDS) and writes only the scratch `work`; then a wave per code
// rewrites its own rows of state and codebook from them - no workgroup reads what another writes, so the update is in place.
//
// Residual chain (wn_rvq_*): S codebooks of K rows, stage s quantises what the stages before it left over (r_0 = e, r_s+1 = r_s - q_s),
// the decoder sees q_0 + ... + q_S-1.  Frames are independent, so the chain is ONE launch per direction: rvq_fwd_k loops the stages
// over a staged tile with the search and merge of vq_fwd_k, rvq_bwd_k / rvq_bwd_stats_k give every (stage, code) a wave with the walk
// of vq_bwd_k, and the EMA update's two launches take the stage as a second grid dimension.  The device functions are shared, so at
// S = 1 every output has the bits of the wn_vq_* entry.
//
// Quantiser dropout (wn_rvq_fwd_n / wn_rvq_bwd_n / wn_rvq_bwd_stats_n / wn_rvq_lookup_n): a stage count n_b per clip, frame fr of clip b is
// active in stage s iff s < n_b (clamped to [1, S] on the device).  Clips of different n share a 4-frame tile whenever Le % 4 != 0, so
// the stage count is a property of the FRAME inside rvq_fwd_n_k: the tile's stage loop runs to the largest n of its frames (read from
// LDS behind a barrier: the same bound in every thread, the barriers inside the loop stay uniform), an inactive frame keeps its
// residual and running q untouched, gets idx = -1 and adds nothing to counts or the stage's loss partial, whose denominator stays
// C Bw.  The backward needs new element workgroups only (the sum over the ACTIVE stages' residuals): idx = -1 matches no code in
// vq_code_walk, so the (stage, code) waves cover exactly the active frames as they are.  With every n = S the statements are the
// chain's: the same bits in every output.
#include <limits>
#include "../../include/wavenet_hip.h"
#include "wn_common.h"
#include "wn_kernels.h"

namespace {

constexpr int FT = 4;              // frames per tile of vq_fwd_k (the butterfly below is written for 4)
constexpr int NWV = 8;             // its waves per workgroup
constexpr int CU = 4;              // codes a wave takes per pass
constexpr int MAXW = 512;          // bw <= 512: 8 values of j per lane
constexpr int NJ = MAXW / 64;
constexpr int CWV = 4;             // vq_bwd_k: waves = codes per workgroup

// frame fr = (clip b, pooled frame l): the offset of its element j = 0 in [B][Bw][Le]; element j sits j * le floats behind it
__device__ __forceinline__ long frame_base(int fr, int bw, int le) {
    const int b = fr / le;
    return (long)b * bw * le + (fr - b * le);
}

// v0..v3: this lane's partial sums of frames 0..3 -> the sum over all 64 lanes of frame (lane >> 4), in every lane of that group
__device__ __forceinline__ float fold4(float v0, float v1, float v2, float v3, int lane) {
    const bool up = lane & 32;
    const float a = (up ? v2 : v0) + __shfl_xor(up ? v0 : v2, 32);     // lower half: frames 0, 1; upper half: frames 2, 3
    const float b = (up ? v3 : v1) + __shfl_xor(up ? v1 : v3, 32);
    const bool odd = lane & 16;
    float c = (odd ? b : a) + __shfl_xor(odd ? a : b, 16);
    c += __shfl_xor(c, 8);
    c += __shfl_xor(c, 4);
    c += __shfl_xor(c, 2);
    c += __shfl_xor(c, 1);
    return c;
}

// The search of one staged tile: this wave's codes k = wave, wave + NWV, ... of the K rows at cb against the FT frames in s_e.  Leaves
// the best (distance, index) of frame lane >> 4 over this wave's codes in bd / bi (the first minimum: codes ascend inside a wave).
// CU codes per pass, so that their loads and their (dependent) butterflies overlap; a code behind the last one reads row K - 1 and is
// left out of the comparison
__device__ __forceinline__ void vq_tile_search(const float* cb, int K, int bw, int nj, const float (*s_e)[MAXW], int lane, int wave,
                                               float& bd, int& bi) {
    bd = std::numeric_limits<float>::infinity();
    bi = 0;
    for (int k0 = wave; k0 < K; k0 += CU * NWV) {
        const float* row[CU];
        float v[CU][FT];
#pragma unroll
        for (int u = 0; u < CU; ++u) {
            row[u] = cb + (long)min(k0 + u * NWV, K - 1) * bw;
#pragma unroll
            for (int f = 0; f < FT; ++f) v[u][f] = 0.f;
        }
        for (int i = 0; i < nj; ++i) {
            const int j = i * 64 + lane;
            if (j < bw) {
                const float e0 = s_e[0][j], e1 = s_e[1][j], e2 = s_e[2][j], e3 = s_e[3][j];
#pragma unroll
                for (int u = 0; u < CU; ++u) {
                    const float c = row[u][j];
                    const float d0 = e0 - c, d1 = e1 - c, d2 = e2 - c, d3 = e3 - c;
                    v[u][0] = fmaf(d0, d0, v[u][0]); v[u][1] = fmaf(d1, d1, v[u][1]);
                    v[u][2] = fmaf(d2, d2, v[u][2]); v[u][3] = fmaf(d3, d3, v[u][3]);
                }
            }
        }
        float d[CU];
#pragma unroll
        for (int u = 0; u < CU; ++u) d[u] = fold4(v[u][0], v[u][1], v[u][2], v[u][3], lane);
#pragma unroll
        for (int u = 0; u < CU; ++u) {                     // codes ascend inside a wave: the first minimum stays
            const int k = k0 + u * NWV;
            if (k < K && d[u] < bd) { bd = d[u]; bi = k; }
        }
    }
}

// The waves' pairs of a tile -> the winner of frame t (thread t < FT; behind the barrier that follows the waves' writes), in wave
// order, lexicographically - the tie rule; it stays in s_bd[0][t] / s_bi[0][t] for the threads behind the next barrier
__device__ __forceinline__ int vq_tile_merge(float (*s_bd)[FT], int (*s_bi)[FT], int t) {
    float d = s_bd[0][t];
    int ix = s_bi[0][t];
    for (int w = 1; w < NWV; ++w) {
        const float dw = s_bd[w][t];
        const int iw = s_bi[w][t];
        if (dw < d || (dw == d && iw < ix)) { d = dw; ix = iw; }
    }
    s_bd[0][t] = d;
    s_bi[0][t] = ix;
    return ix;
}

// (frame fastest: neighbouring threads touch neighbouring l of one row of enc / q_out)
__device__ __forceinline__ void vq_tile_stage(const WnVq& p, int f0, int C, float (*s_e)[MAXW], int t) {
    for (int o = t; o < FT * p.bw; o += 64 * NWV) {
        const int j = o / FT, f = o % FT;
        s_e[f][j] = f0 + f < C ? p.enc[frame_base(f0 + f, p.bw, p.le) + (long)j * p.le] : 0.f;
    }
}

__global__ __launch_bounds__(64 * NWV) void vq_fwd_k(WnVq p, float inv_n) {
    __shared__ float s_e[FT][MAXW];
    __shared__ float s_bd[NWV][FT];
    __shared__ int s_bi[NWV][FT];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int C = p.batch * p.le, tiles = (C + FT - 1) / FT, nj = (p.bw + 63) >> 6;
    const float* cb = p.flat + p.cb_off;
    float loss = 0.f;                                      // thread 0: this workgroup's best distances, in frame order
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int f0 = tile * FT;
        vq_tile_stage(p, f0, C, s_e, t);
        __syncthreads();
        float bd;                                          // of frame lane >> 4, over this wave's codes
        int bi;
        vq_tile_search(cb, p.K, p.bw, nj, s_e, lane, wave, bd, bi);
        if ((lane & 15) == 0) { s_bd[wave][lane >> 4] = bd; s_bi[wave][lane >> 4] = bi; }
        __syncthreads();
        if (t < FT) {
            const int ix = vq_tile_merge(s_bd, s_bi, t);
            if (f0 + t < C) {
                p.idx[f0 + t] = ix;
                if (p.counts) atomicAdd(&p.counts[ix], 1);
            }
        }
        __syncthreads();
        if (t == 0)
            for (int f = 0; f < FT; ++f)
                if (f0 + f < C) loss += s_bd[0][f];
        for (int o = t; o < FT * p.bw; o += 64 * NWV) {
            const int j = o / FT, f = o % FT;
            if (f0 + f < C) p.q_out[frame_base(f0 + f, p.bw, p.le) + (long)j * p.le] = cb[(long)s_bi[0][f] * p.bw + j];
        }
        __syncthreads();                                   // the next tile overwrites s_e, s_bd and s_bi
    }
    if (t == 0) p.loss_part[blockIdx.x] = loss * inv_n;    // every partial is rewritten at every call (a workgroup without a tile: 0)
}

// The residual chain (wn_rvq_fwd): the tile is staged once, the S stages loop inside the workgroup.  Stage s searches ITS K rows for the
// staged residual r_s with vq_fwd_k's search and merge, then every thread subtracts the winning row from the residual in place
// (r_s+1 = r_s - q_s, handed to the backward as res[s]) and adds it onto the running q (q_0 + q_1 + ..., ascending).  idx [S][C],
// counts [S][K], loss_part [S][WN_VQ_PARTIALS].  A frame behind C is staged as zeros and chooses some row of [0, K): nothing of it is written.
__global__ __launch_bounds__(64 * NWV) void rvq_fwd_k(WnVq p, float inv_n) {
    __shared__ float s_e[FT][MAXW];                        // the residual r_s
    __shared__ float s_q[FT][MAXW];                        // q_0 + ... + q_s
    __shared__ float s_bd[NWV][FT];
    __shared__ int s_bi[NWV][FT];
    __shared__ float s_loss[WN_RVQ_MAX_S];                 // thread 0: per stage, this workgroup's best distances in frame order
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int C = p.batch * p.le, tiles = (C + FT - 1) / FT, nj = (p.bw + 63) >> 6;
    const long total = (long)C * p.bw, rows = (long)p.K * p.bw;
    if (t < WN_RVQ_MAX_S) s_loss[t] = 0.f;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int f0 = tile * FT;
        vq_tile_stage(p, f0, C, s_e, t);
        __syncthreads();
        for (int s = 0; s < p.S; ++s) {
            const float* cb = p.flat + p.cb_off + s * rows;
            float bd;
            int bi;
            vq_tile_search(cb, p.K, p.bw, nj, s_e, lane, wave, bd, bi);
            if ((lane & 15) == 0) { s_bd[wave][lane >> 4] = bd; s_bi[wave][lane >> 4] = bi; }
            __syncthreads();
            if (t < FT) {
                const int ix = vq_tile_merge(s_bd, s_bi, t);
                if (f0 + t < C) {
                    p.idx[(long)s * C + f0 + t] = ix;
                    if (p.counts) atomicAdd(&p.counts[s * p.K + ix], 1);
                }
            }
            __syncthreads();
            if (t == 0) {
                float loss = s_loss[s];
                for (int f = 0; f < FT; ++f)
                    if (f0 + f < C) loss += s_bd[0][f];
                s_loss[s] = loss;
            }
            const bool last = s == p.S - 1;
            for (int o = t; o < FT * p.bw; o += 64 * NWV) {
                const int j = o / FT, f = o % FT;
                const float c = cb[(long)s_bi[0][f] * p.bw + j];
                const float r = s_e[f][j] - c;
                const float q = s ? s_q[f][j] + c : c;
                s_e[f][j] = r;
                s_q[f][j] = q;
                if (f0 + f < C) {
                    const long at = frame_base(f0 + f, p.bw, p.le) + (long)j * p.le;
                    p.res[s * total + at] = r;
                    if (last) p.q_out[at] = q;
                }
            }
            __syncthreads();                               // the next stage reads s_e and overwrites s_bd and s_bi; so does the next tile
        }
    }
    if (t < p.S) p.loss_part[t * WN_VQ_PARTIALS + blockIdx.x] = s_loss[t] * inv_n;
}

// a clip's stage count as the _n kernels use it: whatever the array holds, a value of [1, S] - never a bound unchecked
__device__ __forceinline__ int nstage_of(const int32_t* nstage, int b, int S) { return min(max(nstage[b], 1), S); }

// Quantiser dropout (wn_rvq_fwd_n): rvq_fwd_k with a stage count per clip, frame fr of clip b is ACTIVE in stage s iff s < n_b.  An
// active frame gets rvq_fwd_k's arithmetic, an inactive one idx = -1, no count, no loss, and its residual and running q stay as they
// are (res[s] = the carried r_n, so the buffer holds no uninitialised floats); q_out is written behind the frame's last active stage.
// The stage loop runs to the maximum n of the tile's frames - s_n is read behind a barrier, so every thread forms the same bound and
// the barriers inside the loop stay uniform -; the stages behind it only hand out -1 and the carried residual.  A frame behind C has
// n = 0.  With every n = S each statement below is rvq_fwd_k's: the same bits in every output.
__global__ __launch_bounds__(64 * NWV) void rvq_fwd_n_k(WnVq p, const int32_t* __restrict__ nstage, float inv_n) {
    __shared__ float s_e[FT][MAXW];                        // the residual r_s
    __shared__ float s_q[FT][MAXW];                        // q_0 + ... + q_s
    __shared__ float s_bd[NWV][FT];
    __shared__ int s_bi[NWV][FT];
    __shared__ int s_n[FT];                                // the stage counts of the tile's frames
    __shared__ float s_loss[WN_RVQ_MAX_S];
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int C = p.batch * p.le, tiles = (C + FT - 1) / FT, nj = (p.bw + 63) >> 6;
    const long total = (long)C * p.bw, rows = (long)p.K * p.bw;
    if (t < WN_RVQ_MAX_S) s_loss[t] = 0.f;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int f0 = tile * FT;
        vq_tile_stage(p, f0, C, s_e, t);
        if (t < FT) s_n[t] = f0 + t < C ? nstage_of(nstage, (f0 + t) / p.le, p.S) : 0;
        __syncthreads();
        const int n_max = max(max(s_n[0], s_n[1]), max(s_n[2], s_n[3]));
        for (int s = 0; s < n_max; ++s) {
            const float* cb = p.flat + p.cb_off + s * rows;
            float bd;
            int bi;
            vq_tile_search(cb, p.K, p.bw, nj, s_e, lane, wave, bd, bi);
            if ((lane & 15) == 0) { s_bd[wave][lane >> 4] = bd; s_bi[wave][lane >> 4] = bi; }
            __syncthreads();
            if (t < FT) {
                const int ix = vq_tile_merge(s_bd, s_bi, t);
                if (f0 + t < C) {
                    const bool on = s < s_n[t];
                    p.idx[(long)s * C + f0 + t] = on ? ix : -1;
                    if (on && p.counts) atomicAdd(&p.counts[s * p.K + ix], 1);
                }
            }
            __syncthreads();
            if (t == 0) {
                float loss = s_loss[s];
                for (int f = 0; f < FT; ++f)
                    if (s < s_n[f]) loss += s_bd[0][f];
                s_loss[s] = loss;
            }
            for (int o = t; o < FT * p.bw; o += 64 * NWV) {
                const int j = o / FT, f = o % FT, n = s_n[f];
                float r = s_e[f][j];
                if (s < n) {
                    const float c = cb[(long)s_bi[0][f] * p.bw + j];
                    r -= c;
                    const float q = s ? s_q[f][j] + c : c;
                    s_e[f][j] = r;
                    s_q[f][j] = q;
                    if (s == n - 1) p.q_out[frame_base(f0 + f, p.bw, p.le) + (long)j * p.le] = q;
                }
                if (f0 + f < C) p.res[s * total + frame_base(f0 + f, p.bw, p.le) + (long)j * p.le] = r;
            }
            __syncthreads();                               // the next stage reads s_e and overwrites s_bd and s_bi; so does the next tile
        }
        if (n_max < p.S) {                                 // the stages no frame of this tile takes part in
            for (int s = n_max; s < p.S; ++s) {
                if (t < FT && f0 + t < C) p.idx[(long)s * C + f0 + t] = -1;
                for (int o = t; o < FT * p.bw; o += 64 * NWV) {
                    const int j = o / FT, f = o % FT;
                    if (f0 + f < C) p.res[s * total + frame_base(f0 + f, p.bw, p.le) + (long)j * p.le] = s_e[f][j];
                }
            }
            __syncthreads();                               // the next tile overwrites s_e and s_n
        }
    }
    if (t < p.S) p.loss_part[t * WN_VQ_PARTIALS + blockIdx.x] = s_loss[t] * inv_n;
}

// element o of [B][Bw][Le] -> its frame (b * le + l) and its j
__device__ __forceinline__ void elem_of(long o, int bw, int le, int& fr, int& j) {
    const long bj = o / le;
    const int l = (int)(o - bj * le), b = (int)(bj / bw);
    j = (int)(bj - (long)b * bw);
    fr = b * le + l;
}

// the element workgroups of the backward launches (blocks [code_blocks, gridDim.x)): d_e = d_q + c_enc (e - q); every element is read
// and then written by one thread (d_enc may be d_q)
__device__ __forceinline__ void vq_bwd_elems(const WnVq& p, float c_enc, int code_blocks) {
    const float* cb = p.flat + p.cb_off;
    const long total = (long)p.batch * p.le * p.bw, step = (long)(gridDim.x - code_blocks) * (64 * CWV);
    for (long o = (long)(blockIdx.x - code_blocks) * (64 * CWV) + threadIdx.x; o < total; o += step) {
        int fr, j;
        elem_of(o, p.bw, p.le, fr, j);
        const int ix = p.idx[fr];
        const float q = (unsigned)ix < (unsigned)p.K ? cb[(long)ix * p.bw + j] : std::numeric_limits<float>::quiet_NaN();
        p.d_enc[o] = fmaf(c_enc, p.enc[o] - q, p.d_q[o]);
    }
}

// A code's wave (lanes along j) walks idx in ascending frame order, 64 frames per ballot, and adds the frames that chose k from src
// [B][Bw][Le]: GRAD ? c_k - frame : frame.  Returns the number of those frames.  An idx outside [0, K) matches no code.
template <bool GRAD>
__device__ __forceinline__ int vq_code_walk(const int32_t* idx, const float* src, int k, int C, int bw, int le, const float (&ck)[NJ],
                                            float (&acc)[NJ], int lane) {
    int n = 0;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int ix = c0 + lane < C ? idx[c0 + lane] : -1;
        unsigned long long m = __ballot(ix == k);
        n += __popcll(m);
        while (m) {                                        // the matching frames of these 64, in ascending order
            const int f = c0 + __ffsll(m) - 1;
            m &= m - 1;
            const float* e = src + frame_base(f, bw, le);
#pragma unroll
            for (int i = 0; i < NJ; ++i) {
                const int j = i * 64 + lane;
                if (i * 64 < bw && j < bw) acc[i] += GRAD ? ck[i] - e[(long)j * le] : e[(long)j * le];
            }
        }
    }
    return n;
}

// gradient mode, the wave of code k: grad[k] = c_cb sum (c_k - frame) over its frames of src (a code no frame chose: exactly 0);
// cb and grad: this stage's K rows
__device__ __forceinline__ void vq_code_grad(const int32_t* idx, const float* src, const float* cb, float* grad, float c_cb, int k, int C,
                                             int bw, int le, int lane) {
    float ck[NJ], acc[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = i * 64 + lane;
        ck[i] = j < bw ? cb[(long)k * bw + j] : 0.f;
        acc[i] = 0.f;
    }
    vq_code_walk<true>(idx, src, k, C, bw, le, ck, acc, lane);
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = i * 64 + lane;
        if (j < bw) grad[(long)k * bw + j] = c_cb * acc[i];
    }
}

// EMA mode, the wave of code k: stat = [n (K floats) | s (K rows of bw)] of this stage, every entry written; grad[k]: exactly 0
__device__ __forceinline__ void vq_code_stats(const int32_t* idx, const float* src, float* stat, float* grad, int k, int K, int C, int bw,
                                              int le, int lane) {
    float acc[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) acc[i] = 0.f;
    const int n = vq_code_walk<false>(idx, src, k, C, bw, le, acc, acc, lane);
    if (lane == 0) stat[k] = (float)n;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = i * 64 + lane;
        if (j < bw) {
            stat[K + (long)k * bw + j] = acc[i];
            grad[(long)k * bw + j] = 0.f;
        }
    }
}

__global__ __launch_bounds__(64 * CWV) void vq_bwd_k(WnVq p, float c_enc, float c_cb, int code_blocks) {
    if ((int)blockIdx.x >= code_blocks) return vq_bwd_elems(p, c_enc, code_blocks);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.x * CWV + wave;
    if (k >= p.K) return;
    vq_code_grad(p.idx, p.enc, p.flat + p.cb_off, p.flat_grad + p.cb_off, c_cb, k, p.batch * p.le, p.bw, p.le, lane);
}

// EMA mode's backward: the element workgroups of vq_bwd_k as they are; a code's wave adds its frames e (ascending, as there) and counts them
__global__ __launch_bounds__(64 * CWV) void vq_bwd_stats_k(WnVq p, float c_enc, int code_blocks, float* __restrict__ stat) {
    if ((int)blockIdx.x >= code_blocks) return vq_bwd_elems(p, c_enc, code_blocks);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.x * CWV + wave;
    if (k >= p.K) return;
    vq_code_stats(p.idx, p.enc, stat, p.flat_grad + p.cb_off, k, p.K, p.batch * p.le, p.bw, p.le, lane);
}

// ---- the residual chain's backward (wn_rvq_bwd / wn_rvq_bwd_stats): S x code_blocks leading workgroups, a wave per (stage, code) on that
// stage's idx and its input r_s (enc for stage 0, res[s - 1] behind it); the element workgroups form d_e = d_q + c_enc (r_1 + ... + r_S),
// the sum in ascending stage order (at S = 1: e - q, vq_bwd_elems' expression); an idx outside [0, K) in any stage: NaN, never dereferenced
__device__ __forceinline__ void rvq_bwd_elems(const WnVq& p, float c_enc, int first_block) {
    const int C = p.batch * p.le;
    const long total = (long)C * p.bw, step = (long)(gridDim.x - first_block) * (64 * CWV);
    for (long o = (long)(blockIdx.x - first_block) * (64 * CWV) + threadIdx.x; o < total; o += step) {
        int fr, j;
        elem_of(o, p.bw, p.le, fr, j);
        bool ok = true;
        float sum = 0.f;
        for (int s = 0; s < p.S; ++s) {
            ok = ok && (unsigned)p.idx[(long)s * C + fr] < (unsigned)p.K;
            const float r = p.res[s * total + o];
            sum = s ? sum + r : r;
        }
        p.d_enc[o] = fmaf(c_enc, ok ? sum : std::numeric_limits<float>::quiet_NaN(), p.d_q[o]);
    }
}

// the (stage, code) of a leading workgroup's wave: false where the wave has no code
__device__ __forceinline__ bool rvq_code_of(const WnVq& p, int code_blocks, int& s, int& k, const float*& src) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    s = blockIdx.x / code_blocks;
    k = (blockIdx.x - s * code_blocks) * CWV + wave;
    src = s ? p.res + (s - 1) * ((long)p.batch * p.le * p.bw) : p.enc;
    return k < p.K;
}

__global__ __launch_bounds__(64 * CWV) void rvq_bwd_k(WnVq p, float c_enc, float c_cb, int code_blocks) {
    if ((int)blockIdx.x >= p.S * code_blocks) return rvq_bwd_elems(p, c_enc, p.S * code_blocks);
    int s, k;
    const float* src;
    if (!rvq_code_of(p, code_blocks, s, k, src)) return;
    const long at = p.cb_off + (long)s * p.K * p.bw;
    const int C = p.batch * p.le;
    vq_code_grad(p.idx + (long)s * C, src, p.flat + at, p.flat_grad + at, c_cb, k, C, p.bw, p.le, threadIdx.x & 63);
}

__global__ __launch_bounds__(64 * CWV) void rvq_bwd_stats_k(WnVq p, float c_enc, int code_blocks, float* __restrict__ stat) {
    if ((int)blockIdx.x >= p.S * code_blocks) return rvq_bwd_elems(p, c_enc, p.S * code_blocks);
    int s, k;
    const float* src;
    if (!rvq_code_of(p, code_blocks, s, k, src)) return;
    const int C = p.batch * p.le;
    vq_code_stats(p.idx + (long)s * C, src, stat + (long)s * p.K * (p.bw + 1), p.flat_grad + p.cb_off + (long)s * p.K * p.bw, k, p.K, C,
                  p.bw, p.le, threadIdx.x & 63);
}

// ---- quantiser dropout's backward (wn_rvq_bwd_n / wn_rvq_bwd_stats_n).  The code waves are the ones above: an inactive frame's idx is
// -1, which vq_code_walk matches with no code, so a stage's rows cover exactly its active frames.  The element workgroups sum the
// ACTIVE stages only, d_e = d_q + c_enc (r_1 + ... + r_n), ascending - rvq_bwd_elems' expressions, so n = S gives its bits -, NaN iff
// an active stage's idx lies outside [0, K); an inactive idx is not looked at
__device__ __forceinline__ void rvq_bwd_elems_n(const WnVq& p, const int32_t* nstage, float c_enc, int first_block) {
    const int C = p.batch * p.le;
    const long total = (long)C * p.bw, step = (long)(gridDim.x - first_block) * (64 * CWV);
    for (long o = (long)(blockIdx.x - first_block) * (64 * CWV) + threadIdx.x; o < total; o += step) {
        int fr, j;
        elem_of(o, p.bw, p.le, fr, j);
        const int n = nstage_of(nstage, fr / p.le, p.S);
        bool ok = true;
        float sum = 0.f;
        for (int s = 0; s < n; ++s) {
            ok = ok && (unsigned)p.idx[(long)s * C + fr] < (unsigned)p.K;
            const float r = p.res[s * total + o];
            sum = s ? sum + r : r;
        }
        p.d_enc[o] = fmaf(c_enc, ok ? sum : std::numeric_limits<float>::quiet_NaN(), p.d_q[o]);
    }
}

__global__ __launch_bounds__(64 * CWV) void rvq_bwd_n_k(WnVq p, const int32_t* __restrict__ nstage, float c_enc, float c_cb, int code_blocks) {
    if ((int)blockIdx.x >= p.S * code_blocks) return rvq_bwd_elems_n(p, nstage, c_enc, p.S * code_blocks);
    int s, k;
    const float* src;
    if (!rvq_code_of(p, code_blocks, s, k, src)) return;
    const long at = p.cb_off + (long)s * p.K * p.bw;
    const int C = p.batch * p.le;
    vq_code_grad(p.idx + (long)s * C, src, p.flat + at, p.flat_grad + at, c_cb, k, C, p.bw, p.le, threadIdx.x & 63);
}

__global__ __launch_bounds__(64 * CWV) void rvq_bwd_stats_n_k(WnVq p, const int32_t* __restrict__ nstage, float c_enc, int code_blocks,
                                                              float* __restrict__ stat) {
    if ((int)blockIdx.x >= p.S * code_blocks) return rvq_bwd_elems_n(p, nstage, c_enc, p.S * code_blocks);
    int s, k;
    const float* src;
    if (!rvq_code_of(p, code_blocks, s, k, src)) return;
    const int C = p.batch * p.le;
    vq_code_stats(p.idx + (long)s * C, src, stat + (long)s * p.K * (p.bw + 1), p.flat_grad + p.cb_off + (long)s * p.K * p.bw, k, p.K, C,
                  p.bw, p.le, threadIdx.x & 63);
}

// ---- the EMA update.  Both launches form N' with THIS expression, so a code's N' has the same bits in either
__device__ __forceinline__ float ema_mix(float g, float omg, float old, float fresh) { return fmaf(omg, fresh, g * old); }

// the scratch of wn_vq_ema_update (WN_VQ_EMA_WORK_BYTES): what the ranking launch hands the row launch
struct VqEmaWork {
    float tot;                     // sum of N' (per wave by butterfly, the waves in ascending order)
    int32_t restarted, left;       // dead codes that found a donor / that did not
    int32_t pad;
    int32_t donor[WN_VQ_MAX_K];    // per code: the code whose batch mean it takes, or -1
};
static_assert(sizeof(VqEmaWork) == WN_VQ_EMA_WORK, "the scratch's documented size");

// ONE workgroup, thread k = code k.  Reads the old N and stat, writes only `work`.  Dead codes (N' < restart) rank by index: a prefix
// count over ballots.  Donors (not dead, n_k >= 2) rank by (n descending, index ascending): key[k] = n_k (an integer below 2^32) above
// the 10 bits of 1023 - k, 0 for every other code - no two donors share a key, so a donor's rank is the number of larger keys: a
// counting rank, every donor walks the K keys in LDS two at a time (all lanes read one address: a broadcast; the keys behind K are 0).
// blockIdx.y = the stage of a residual chain (wn_rvq_ema_update; 0 alone for wn_vq_ema_update): its own block of stat and state
// (`stride` floats each) and its own VqEmaWork - codes and donors are ranked within the stage.
__global__ __launch_bounds__(WN_VQ_MAX_K) void vq_ema_rank_k(const float* __restrict__ stat, const float* __restrict__ state,
                                                             VqEmaWork* __restrict__ work, int K, long stride, float g, float omg,
                                                             float restart, const wn_guard_state* __restrict__ guard) {
    __shared__ __attribute__((aligned(16))) unsigned long long s_key[WN_VQ_MAX_K];
    __shared__ int s_donor[WN_VQ_MAX_K];
    __shared__ float s_tot[WN_VQ_MAX_K / 64];
    __shared__ int s_dead[WN_VQ_MAX_K / 64], s_don[WN_VQ_MAX_K / 64];
    if (guard && guard->skip) return;
    stat += blockIdx.y * stride;
    state += blockIdx.y * stride;
    work += blockIdx.y;
    const int k = threadIdx.x, lane = k & 63, wave = k >> 6;
    float n = 0.f, N1 = 0.f;
    bool dead = false, don = false;
    if (k < K) {
        n = stat[k];
        N1 = ema_mix(g, omg, state[k], n);
        dead = restart > 0.f && N1 < restart;
        don = !dead && n >= 2.f;
    }
    const unsigned long long key = don ? ((unsigned long long)(unsigned)fminf(n, 4294967040.f) << 10) | (unsigned)(WN_VQ_MAX_K - 1 - k) : 0ull;
    s_key[k] = key;
    float t = N1;
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    const unsigned long long b_dead = __ballot(dead), b_don = __ballot(don);
    if (lane == 0) {
        s_tot[wave] = t;
        s_dead[wave] = __popcll(b_dead);
        s_don[wave] = __popcll(b_don);
    }
    __syncthreads();
    int n_dead = 0, n_donor = 0, rank = 0;                 // the sizes of the two kinds; this code's rank among its kind
    for (int w = 0; w < WN_VQ_MAX_K / 64; ++w) {
        n_dead += s_dead[w];
        n_donor += s_don[w];
        if (w < wave) rank += s_dead[w];
    }
    rank += __popcll(b_dead & ((1ull << lane) - 1ull));
    if (don) {
        rank = 0;
        const ulonglong2* key2 = (const ulonglong2*)s_key;
#pragma unroll 8
        for (int j2 = 0; j2 < (K + 1) >> 1; ++j2) {
            const ulonglong2 v = key2[j2];
            rank += (v.x > key) + (v.y > key);
        }
        s_donor[rank] = k;
    }
    __syncthreads();
    if (k < K) work->donor[k] = (dead && rank < n_donor) ? s_donor[rank] : -1;
    if (k == 0) {
        float tot = s_tot[0];
        for (int w = 1; w < (K + 63) / 64; ++w) tot += s_tot[w];
        const int r = n_dead < n_donor ? n_dead : n_donor;
        work->tot = tot;
        work->restarted = r;
        work->left = n_dead - r;
    }
}

// A wave per code, lanes along j: its own N and m row of state and its own codebook row, rewritten in place; work and stat are read only.
// blockIdx.y = the stage, as above: its K rows of the codebook, its blocks of stat and state, its work and its info[2]
__global__ __launch_bounds__(64 * CWV) void vq_ema_rows_k(float* __restrict__ cb, const float* __restrict__ stat, float* __restrict__ state,
                                                          const VqEmaWork* __restrict__ work, int32_t* __restrict__ info, int K, int bw,
                                                          float g, float omg, float eps, const wn_guard_state* __restrict__ guard) {
    if (guard && guard->skip) return;
    cb += (long)blockIdx.y * K * bw;
    stat += (long)blockIdx.y * K * (bw + 1);
    state += (long)blockIdx.y * K * (bw + 1);
    work += blockIdx.y;
    if (info) info += 2 * blockIdx.y;
    if (info && blockIdx.x == 0 && threadIdx.x == 0) {
        info[0] += work->restarted;
        info[1] = work->left;
    }
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.x * CWV + wave;
    if (k >= K) return;
    const int donor = work->donor[k];
    float* m = state + K + (long)k * bw;
    if ((unsigned)donor < (unsigned)K) {                   // restarted: the donor's batch mean, with usage 1
        const float nd = stat[donor];
        const float* sd = stat + K + (long)donor * bw;
        for (int j = lane; j < bw; j += 64) {
            const float c = sd[j] / nd;
            m[j] = c;
            cb[(long)k * bw + j] = c;
        }
        if (lane == 0) state[k] = 1.f;
        return;
    }
    const float N1 = ema_mix(g, omg, state[k], stat[k]);
    const float tot = work->tot;
    const float nhat = (N1 + eps) / (tot + (float)K * eps) * tot;
    const float* s = stat + K + (long)k * bw;
    for (int j = lane; j < bw; j += 64) {
        const float m1 = ema_mix(g, omg, m[j], s[j]);
        m[j] = m1;
        cb[(long)k * bw + j] = m1 / nhat;
    }
    if (lane == 0) state[k] = N1;                          // (behind the wave's reads of it: one wave, program order)
}

// q = c_0[idx_0] + c_1[idx_1] + ... over the first `stages` stages, ascending (one stage: wn_vq_lookup); idx [stages][frames], cb: K rows per stage
__global__ __launch_bounds__(256) void vq_lookup_k(const int32_t* idx, const float* cb, float* q_out, int32_t* bad, int K, int bw, int le,
                                                   long total, int stages, long frames) {
    for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
        int fr, j;
        elem_of(o, bw, le, fr, j);
        bool ok = true;
        float q = 0.f;
        for (int s = 0; s < stages; ++s) {
            const int ix = idx[s * frames + fr];
            const bool in = (unsigned)ix < (unsigned)K;
            const float c = in ? cb[((long)s * K + ix) * bw + j] : 0.f;
            q = s ? q + c : c;
            ok = ok && in;
        }
        q_out[o] = ok ? q : std::numeric_limits<float>::quiet_NaN();
        if (!ok && bad) *bad = 1;                          // (every writer stores the same value)
    }
}

// per-clip stage counts (wn_rvq_lookup_n): q = the sum of the first n_b stages' rows, ascending; idx [S][frames].  An n_b outside [1, S]
// or an ACTIVE idx outside [0, K): a NaN frame and *bad, nothing dereferenced; an inactive idx is not looked at
__global__ __launch_bounds__(256) void vq_lookup_n_k(const int32_t* idx, const int32_t* nstage, const float* cb, float* q_out, int32_t* bad,
                                                     int S, int K, int bw, int le, long total, long frames) {
    for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
        int fr, j;
        elem_of(o, bw, le, fr, j);
        const int n_raw = nstage[fr / le];
        bool ok = n_raw >= 1 && n_raw <= S;
        const int n = ok ? n_raw : 0;
        float q = 0.f;
        for (int s = 0; s < n; ++s) {
            const int ix = idx[s * frames + fr];
            const bool in = (unsigned)ix < (unsigned)K;
            const float c = in ? cb[((long)s * K + ix) * bw + j] : 0.f;
            q = s ? q + c : c;
            ok = ok && in;
        }
        q_out[o] = ok ? q : std::numeric_limits<float>::quiet_NaN();
        if (!ok && bad) *bad = 1;                          // (every writer stores the same value)
    }
}

}  // namespace

// The callers (wn_api.hip) have checked the arguments.
int wn_launch_vq_fwd(const WnVq& p, hipStream_t st) {
    if (p.batch <= 0) return 0;
    if (p.counts) {
        hipError_t e = hipMemsetAsync(p.counts, 0, sizeof(int32_t) * p.K, st);
        if (e != hipSuccess) return wn_set_error(e, __FILE__, __LINE__);
    }
    const double n = (double)p.batch * p.le * p.bw;
    hipLaunchKernelGGL(vq_fwd_k, dim3(WN_VQ_PARTIALS), dim3(64 * NWV), 0, st, p, (float)(1.0 / n));
    WN_CHECK_LAUNCH();
    return 0;
}

int wn_launch_vq_bwd(const WnVq& p, float beta, float g_scale, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const double s = 2.0 / ((double)p.batch * p.le * p.bw);
    const int code_blocks = (p.K + CWV - 1) / CWV;
    const long total = (long)p.batch * p.le * p.bw;
    const int elem_blocks = (int)std::min<long>((total + 64 * CWV - 1) / (64 * CWV), 256);
    hipLaunchKernelGGL(vq_bwd_k, dim3(code_blocks + elem_blocks), dim3(64 * CWV), 0, st, p, (float)((double)g_scale * beta * s),
                       (float)((double)g_scale * s), code_blocks);
    WN_CHECK_LAUNCH();
    return 0;
}

int wn_launch_vq_bwd_stats(const WnVq& p, float beta, float g_scale, float* stat, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const double s = 2.0 / ((double)p.batch * p.le * p.bw);
    const int code_blocks = (p.K + CWV - 1) / CWV;
    const long total = (long)p.batch * p.le * p.bw;
    const int elem_blocks = (int)std::min<long>((total + 64 * CWV - 1) / (64 * CWV), 256);
    hipLaunchKernelGGL(vq_bwd_stats_k, dim3(code_blocks + elem_blocks), dim3(64 * CWV), 0, st, p, (float)((double)g_scale * beta * s),
                       code_blocks, stat);
    WN_CHECK_LAUNCH();
    return 0;
}

int wn_launch_vq_ema_update(float* flat, long cb_off, const float* stat, float* state, void* work, int32_t* info, int S, int K, int bw,
                            float decay, float eps, float restart, const wn_guard_state* guard, hipStream_t st) {
    const float omg = (float)(1.0 - (double)decay);
    hipLaunchKernelGGL(vq_ema_rank_k, dim3(1, S), dim3(WN_VQ_MAX_K), 0, st, stat, state, (VqEmaWork*)work, K, (long)K * (bw + 1), decay, omg,
                       restart, guard);
    WN_CHECK_LAUNCH();
    hipLaunchKernelGGL(vq_ema_rows_k, dim3((K + CWV - 1) / CWV, S), dim3(64 * CWV), 0, st, flat + cb_off, stat, state,
                       (const VqEmaWork*)work, info, K, bw, decay, omg, eps, guard);
    WN_CHECK_LAUNCH();
    return 0;
}

int wn_launch_vq_lookup(const int32_t* idx, const float* flat, long cb_off, float* q_out, int32_t* bad, int stages, int K, int bw, int le,
                        int batch, hipStream_t st) {
    if (batch <= 0) return 0;
    if (bad) {
        hipError_t e = hipMemsetAsync(bad, 0, sizeof(int32_t), st);
        if (e != hipSuccess) return wn_set_error(e, __FILE__, __LINE__);
    }
    const long total = (long)batch * le * bw;
    hipLaunchKernelGGL(vq_lookup_k, dim3((unsigned)std::min<long>((total + 255) / 256, 1024)), dim3(256), 0, st, idx, flat + cb_off, q_out, bad,
                       K, bw, le, total, stages, (long)batch * le);
    WN_CHECK_LAUNCH();
    return 0;
}

// ---- the residual chain (p.S stages; p.idx [S][C], p.counts [S][K], p.res [S][B][Bw][Le], p.loss_part [S][WN_VQ_PARTIALS])
int wn_launch_rvq_fwd(const WnVq& p, hipStream_t st) {
    if (p.batch <= 0) return 0;
    if (p.counts) {
        hipError_t e = hipMemsetAsync(p.counts, 0, sizeof(int32_t) * p.S * p.K, st);
        if (e != hipSuccess) return wn_set_error(e, __FILE__, __LINE__);
    }
    const double n = (double)p.batch * p.le * p.bw;
    hipLaunchKernelGGL(rvq_fwd_k, dim3(WN_VQ_PARTIALS), dim3(64 * NWV), 0, st, p, (float)(1.0 / n));
    WN_CHECK_LAUNCH();
    return 0;
}

// (the scalars and the element workgroups' count: as wn_launch_vq_bwd forms them)
int wn_launch_rvq_bwd(const WnVq& p, float beta, float g_scale, float* stat, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const double s = 2.0 / ((double)p.batch * p.le * p.bw);
    const int code_blocks = (p.K + CWV - 1) / CWV;
    const long total = (long)p.batch * p.le * p.bw;
    const int elem_blocks = (int)std::min<long>((total + 64 * CWV - 1) / (64 * CWV), 256);
    const dim3 grid(p.S * code_blocks + elem_blocks);
    const float c_enc = (float)((double)g_scale * beta * s);
    if (stat)
        hipLaunchKernelGGL(rvq_bwd_stats_k, grid, dim3(64 * CWV), 0, st, p, c_enc, code_blocks, stat);
    else
        hipLaunchKernelGGL(rvq_bwd_k, grid, dim3(64 * CWV), 0, st, p, c_enc, (float)((double)g_scale * s), code_blocks);
    WN_CHECK_LAUNCH();
    return 0;
}

// ---- quantiser dropout (nstage: batch int32 stage counts on the device): the launches above with the _n kernels, the same grids
int wn_launch_rvq_fwd_n(const WnVq& p, const int32_t* nstage, hipStream_t st) {
    if (p.batch <= 0) return 0;
    if (p.counts) {
        hipError_t e = hipMemsetAsync(p.counts, 0, sizeof(int32_t) * p.S * p.K, st);
        if (e != hipSuccess) return wn_set_error(e, __FILE__, __LINE__);
    }
    const double n = (double)p.batch * p.le * p.bw;        // the FIXED denominator: vq_loss is the batch expectation
    hipLaunchKernelGGL(rvq_fwd_n_k, dim3(WN_VQ_PARTIALS), dim3(64 * NWV), 0, st, p, nstage, (float)(1.0 / n));
    WN_CHECK_LAUNCH();
    return 0;
}

int wn_launch_rvq_bwd_n(const WnVq& p, const int32_t* nstage, float beta, float g_scale, float* stat, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const double s = 2.0 / ((double)p.batch * p.le * p.bw);
    const int code_blocks = (p.K + CWV - 1) / CWV;
    const long total = (long)p.batch * p.le * p.bw;
    const int elem_blocks = (int)std::min<long>((total + 64 * CWV - 1) / (64 * CWV), 256);
    const dim3 grid(p.S * code_blocks + elem_blocks);
    const float c_enc = (float)((double)g_scale * beta * s);
    if (stat)
        hipLaunchKernelGGL(rvq_bwd_stats_n_k, grid, dim3(64 * CWV), 0, st, p, nstage, c_enc, code_blocks, stat);
    else
        hipLaunchKernelGGL(rvq_bwd_n_k, grid, dim3(64 * CWV), 0, st, p, nstage, c_enc, (float)((double)g_scale * s), code_blocks);
    WN_CHECK_LAUNCH();
    return 0;
}

int wn_launch_vq_lookup_n(const int32_t* idx, const int32_t* nstage, const float* flat, long cb_off, float* q_out, int32_t* bad, int S, int K,
                          int bw, int le, int batch, hipStream_t st) {
    if (batch <= 0) return 0;
    if (bad) {
        hipError_t e = hipMemsetAsync(bad, 0, sizeof(int32_t), st);
        if (e != hipSuccess) return wn_set_error(e, __FILE__, __LINE__);
    }
    const long total = (long)batch * le * bw;
    hipLaunchKernelGGL(vq_lookup_n_k, dim3((unsigned)std::min<long>((total + 255) / 256, 1024)), dim3(256), 0, st, idx, nstage, flat + cb_off,
                       q_out, bad, S, K, bw, le, total, (long)batch * le);
    WN_CHECK_LAUNCH();
    return 0;
}
