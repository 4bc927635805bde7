// The vector-quantised bottleneck of the autoencoder (the wn_vq_* and wn_rvq_* entries of include/wavenet_hip.h): every pooled frame
// e[b][:, l] of enc [B][Bw][Le] is replaced by its nearest row of a codebook c [K][Bw], a parameter of the flat buffer - or, in a
// residual chain, by the sum of S such rows.  ONE kernel family: a forward, a backward and a lookup template, the EMA update's two
// kernels, four launchers.
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
// The templates' parameters (compile-time: the forms do not cost the same registers and LDS, tools/kres.sh shows each instantiation):
//   CHAIN   the residual chain (wn_rvq_*, chosen by WnVq::res != NULL, at S = 1 too): S codebooks of K rows, stage s quantises what the
//           stages before it left over (r_0 = e, r_s+1 = r_s - q_s), the decoder sees q_0 + ... + q_S-1.  Frames are independent, so the
//           chain is still ONE launch per direction: the forward loops the stages over its staged tile, the backward gives every
//           (stage, code) a wave, the EMA update's two launches take the stage as a second grid dimension.  Without it (wn_vq_*) there
//           is one stage, no res, no running q; the statements are shared, so at S = 1 the chain has the one-stage entries' bits.
//   NST     quantiser dropout (wn_rvq_*_n, WnVq::nstage != NULL; the chain only): a stage count n_b per clip, frame fr of clip b is
//           active in stage s iff s < n_b (clamped to [1, S] on the device; the lookup does not clamp, it flags).  Clips of different n
//           share a 4-frame tile whenever Le % 4 != 0, so the stage count is a property of the FRAME in the forward: the tile's stage
//           loop runs to the largest n of its frames (read from LDS behind a barrier: the same bound in every thread, the barriers
//           inside the loop stay uniform), an inactive frame keeps its residual and running q untouched, gets idx = -1 and adds
//           nothing to counts or the stage's loss partial, whose denominator stays C Bw.  The backward's element workgroups sum the
//           ACTIVE stages' residuals; idx = -1 matches no code in vq_code_walk, so the (stage, code) waves cover exactly the active
//           frames as they are.  With every n = S the statements are the chain's: the same bits in every output.
//   STATS   (backward) EMA mode, wn_*_bwd_stats* / wn_*_ema_update: the codebook follows the running mean of its frames instead of a
//           gradient.  The code workgroups add e instead of c_k - e: stat = [n | s], the frames per code (as floats) and their sums in
//           ascending frame order; the codebook's rows of flat_grad become exactly 0.
//
// The EMA update: N' = g N + (1 - g) n, m' = g m + (1 - g) s, c' = m' / Nhat with the usage smoothed by eps; a code whose N' fell
// below `restart` takes the batch mean s / n of a donor (the d-th dead code, ascending, the d-th code by n descending).  Two launches:
// ONE workgroup per stage ranks the K codes (counting ranks over LDS) and writes only the scratch `work`; then a wave per code
// rewrites its own rows of state and codebook from them - no workgroup reads what another writes, so the update is in place.
#include <limits>
#include "../../include/wavenet_hip.h"
#include "wn_common.h"
#include "wn_kernels.h"

namespace {

constexpr int FT = 4;              // frames per tile of the forward (the butterfly below is written for 4)
constexpr int NWV = 8;             // its waves per workgroup
constexpr int CU = 4;              // codes a wave takes per pass
constexpr int MAXW = 512;          // bw <= 512: 8 values of j per lane
constexpr int NJ = MAXW / 64;
constexpr int CWV = 4;             // the backward: waves = codes per workgroup

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

// a clip's stage count as the forward and the backward use it: whatever the array holds, a value of [1, S] - never a bound unchecked
__device__ __forceinline__ int nstage_of(const int32_t* nstage, int b, int S) { return min(max(nstage[b], 1), S); }

// The forward of every entry: a tile of FT frames is staged once, then per stage: search, publish, merge, loss, write back.
//   <false, false>  wn_vq_fwd: one stage (p.S is not read), q_out = the winning rows; no s_q / s_loss / s_n, no res
//   <true, false>   wn_rvq_fwd: stage s searches ITS K rows for the staged residual r_s, then every thread subtracts the winning row from
//                   the residual in place (r_s+1 = r_s - q_s, handed to the backward as res[s]) and adds it onto the running q (q_0 +
//                   q_1 + ..., ascending).  idx [S][C], counts [S][K], loss_part [S][WN_VQ_PARTIALS]
//   <true, true>    wn_rvq_fwd_n: frame fr of clip b is ACTIVE in stage s iff s < n_b.  An active frame gets the chain's arithmetic, an
//                   inactive one idx = -1, no count, no loss, and its residual and running q stay as they are (res[s] = the carried
//                   r_n, so the buffer holds no uninitialised floats); q_out is written behind the frame's last active stage.  The
//                   stage loop runs to the maximum n of the tile's frames - s_n is read behind a barrier, so every thread forms the
//                   same bound and the barriers inside the loop stay uniform -; the stages behind it only hand out -1 and the carried
//                   residual.  A frame behind C has n = 0.  With every n = S each statement is the chain's: the same bits everywhere.
// A frame behind C is staged as zeros and chooses some row of [0, K): nothing of it is written.
template <bool CHAIN, bool NST>
__global__ __launch_bounds__(64 * NWV) void vq_fwd_k(WnVq p, float inv_n) {
    static_assert(CHAIN || !NST, "stage counts belong to the chain");
    __shared__ float s_e[FT][MAXW];                        // the frames; in a chain the residual r_s
    __shared__ float s_q[FT][MAXW];                        // CHAIN: q_0 + ... + q_s
    __shared__ float s_bd[NWV][FT];
    __shared__ int s_bi[NWV][FT];
    __shared__ int s_n[FT];                                // NST: the stage counts of the tile's frames
    __shared__ float s_loss[WN_RVQ_MAX_S];                 // CHAIN, thread 0: per stage, this workgroup's best distances in frame order
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int C = p.batch * p.le, tiles = (C + FT - 1) / FT, nj = (p.bw + 63) >> 6;
    const int S = CHAIN ? p.S : 1;
    const long total = (long)C * p.bw, rows = (long)p.K * p.bw;
    // (formed out here, not beside its use: the one-stage form sits at 72 VGPRs, the last count with 7 waves per SIMD, and with the base
    // formed inside the tile loop, or a 64-bit sum as its idx offset, the compiler gives up the search's four loads in flight to stay
    // there - 1.2x to 1.75x the time.  tools/kres.sh: 72 VGPRs is the good schedule, 66 the serialised one)
    const float* const cb0 = p.flat + p.cb_off;
    float loss = 0.f;                                      // !CHAIN, thread 0: what s_loss[0] would hold
    if constexpr (CHAIN)
        if (t < WN_RVQ_MAX_S) s_loss[t] = 0.f;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int f0 = tile * FT;
        vq_tile_stage(p, f0, C, s_e, t);
        if constexpr (NST)
            if (t < FT) s_n[t] = f0 + t < C ? nstage_of(p.nstage, (f0 + t) / p.le, S) : 0;
        __syncthreads();
        int n_max = S;
        if constexpr (NST) n_max = max(max(s_n[0], s_n[1]), max(s_n[2], s_n[3]));
        for (int s = 0; s < n_max; ++s) {
            const float* cb = cb0 + s * rows;
            float bd;                                      // of frame lane >> 4, over this wave's codes
            int bi;
            vq_tile_search(cb, p.K, p.bw, nj, s_e, lane, wave, bd, bi);
            if ((lane & 15) == 0) { s_bd[wave][lane >> 4] = bd; s_bi[wave][lane >> 4] = bi; }
            __syncthreads();
            if (t < FT) {
                const int ix = vq_tile_merge(s_bd, s_bi, t);
                if (f0 + t < C) {
                    bool on = true;
                    if constexpr (NST) on = s < s_n[t];
                    p.idx[CHAIN ? (long)s * C + f0 + t : f0 + t] = on ? ix : -1;          // (one stage: a 32-bit sum, see cb0)
                    if (on && p.counts) atomicAdd(&p.counts[s * p.K + ix], 1);
                }
            }
            __syncthreads();
            if (t == 0) {
                if constexpr (CHAIN) loss = s_loss[s];
                for (int f = 0; f < FT; ++f) {
                    bool on = f0 + f < C;
                    if constexpr (NST) on = s < s_n[f];
                    if (on) loss += s_bd[0][f];
                }
                if constexpr (CHAIN) s_loss[s] = loss;
            }
            for (int o = t; o < FT * p.bw; o += 64 * NWV) {
                const int j = o / FT, f = o % FT;
                if constexpr (!CHAIN) {
                    if (f0 + f < C) p.q_out[frame_base(f0 + f, p.bw, p.le) + (long)j * p.le] = cb[(long)s_bi[0][f] * p.bw + j];
                } else {
                    int n = S;
                    if constexpr (NST) n = s_n[f];
                    float r = s_e[f][j], q = 0.f;
                    if (s < n) {
                        const float c = cb[(long)s_bi[0][f] * p.bw + j];
                        r -= c;
                        q = s ? s_q[f][j] + c : c;
                        s_e[f][j] = r;
                        s_q[f][j] = q;
                        if constexpr (NST)                 // (s < n: a frame in front of C)
                            if (s == n - 1) p.q_out[frame_base(f0 + f, p.bw, p.le) + (long)j * p.le] = q;
                    }
                    if (f0 + f < C) {
                        const long at = frame_base(f0 + f, p.bw, p.le) + (long)j * p.le;
                        p.res[s * total + at] = r;
                        if constexpr (!NST)
                            if (s == S - 1) p.q_out[at] = q;
                    }
                }
            }
            __syncthreads();                               // the next stage reads s_e and overwrites s_bd and s_bi; so does the next tile
        }
        if constexpr (NST) {
            if (n_max < S) {                               // the stages no frame of this tile takes part in
                for (int s = n_max; s < S; ++s) {
                    if (t < FT && f0 + t < C) p.idx[(long)s * C + f0 + t] = -1;
                    for (int o = t; o < FT * p.bw; o += 64 * NWV) {
                        const int j = o / FT, f = o % FT;
                        if (f0 + f < C) p.res[s * total + frame_base(f0 + f, p.bw, p.le) + (long)j * p.le] = s_e[f][j];
                    }
                }
                __syncthreads();                           // the next tile overwrites s_e and s_n
            }
        }
    }
    // every partial is rewritten at every call (a workgroup without a tile: 0)
    if constexpr (CHAIN) {
        if (t < S) p.loss_part[t * WN_VQ_PARTIALS + blockIdx.x] = s_loss[t] * inv_n;
    } else {
        if (t == 0) p.loss_part[blockIdx.x] = loss * inv_n;
    }
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

// the chain's element workgroups: d_e = d_q + c_enc (r_1 + ... + r_n), the residuals of the frame's n stages in ascending order (at
// S = 1: e - q, vq_bwd_elems' expression), n = S, with NST the clip's stage count: the ACTIVE stages only, so n = S gives the chain's
// bits.  An idx outside [0, K) in one of those stages: NaN, never dereferenced; an inactive idx is not looked at
template <bool NST>
__device__ __forceinline__ void rvq_bwd_elems(const WnVq& p, float c_enc, int first_block) {
    const int C = p.batch * p.le;
    const long total = (long)C * p.bw, step = (long)(gridDim.x - first_block) * (64 * CWV);
    for (long o = (long)(blockIdx.x - first_block) * (64 * CWV) + threadIdx.x; o < total; o += step) {
        int fr, j;
        elem_of(o, p.bw, p.le, fr, j);
        int n = p.S;
        if constexpr (NST) n = nstage_of(p.nstage, fr / p.le, p.S);
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

// the (stage, code) of a leading workgroup's wave and the stage's input r_s (enc for stage 0, res[s - 1] behind it): false where the
// wave has no code
template <bool CHAIN>
__device__ __forceinline__ bool rvq_code_of(const WnVq& p, int code_blocks, int& s, int& k, const float*& src) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    s = CHAIN ? blockIdx.x / code_blocks : 0;
    k = (blockIdx.x - s * code_blocks) * CWV + wave;
    src = s ? p.res + (s - 1) * ((long)p.batch * p.le * p.bw) : p.enc;
    return k < p.K;
}

// The backward of every entry, one launch: S x code_blocks leading workgroups (S = 1 without CHAIN: wn_vq_bwd*, where p.S and p.res are
// not read), a wave per (stage, code) on that stage's idx and its input; the workgroups behind them form d_e elementwise.  STATS (EMA
// mode, `stat` [S][K (bw + 1)]): a code's wave adds its frames and counts them, the codebook's rows of flat_grad become 0.  NST
// (quantiser dropout) changes the element workgroups alone: an inactive frame's idx is -1, which vq_code_walk matches with no code, so
// a stage's rows cover exactly its active frames as they are.
template <bool CHAIN, bool NST, bool STATS>
__global__ __launch_bounds__(64 * CWV) void vq_bwd_k(WnVq p, float c_enc, float c_cb, int code_blocks, float* __restrict__ stat) {
    static_assert(CHAIN || !NST, "stage counts belong to the chain");
    const int first_elem = CHAIN ? p.S * code_blocks : code_blocks;
    if ((int)blockIdx.x >= first_elem) {
        if constexpr (CHAIN) return rvq_bwd_elems<NST>(p, c_enc, first_elem);
        else return vq_bwd_elems(p, c_enc, first_elem);
    }
    int s, k;
    const float* src;
    if (!rvq_code_of<CHAIN>(p, code_blocks, s, k, src)) return;
    const long at = p.cb_off + (long)s * p.K * p.bw;
    const int C = p.batch * p.le, lane = threadIdx.x & 63;
    const int32_t* idx = p.idx + (long)s * C;
    if constexpr (STATS) vq_code_stats(idx, src, stat + (long)s * p.K * (p.bw + 1), p.flat_grad + at, k, p.K, C, p.bw, p.le, lane);
    else vq_code_grad(idx, src, p.flat + at, p.flat_grad + at, c_cb, k, C, p.bw, p.le, lane);
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

// q = c_0[idx_0] + c_1[idx_1] + ... over the first n stages, ascending; idx [.][frames], cb: K rows per stage.  n = `stages` (1:
// wn_vq_lookup); with NST (wn_rvq_lookup_n) the clip's stage count, which is NOT clamped: an n_b outside [1, stages] gives a NaN frame and
// *bad, as does an ACTIVE idx outside [0, K) in either form; nothing of it is dereferenced, an inactive idx is not looked at
template <bool NST>
__global__ __launch_bounds__(256) void vq_lookup_k(const int32_t* idx, const int32_t* nstage, const float* cb, float* q_out, int32_t* bad,
                                                   int stages, int K, int bw, int le, long total, long frames) {
    for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
        int fr, j;
        elem_of(o, bw, le, fr, j);
        bool ok = true;
        int n = stages;
        if constexpr (NST) {
            const int n_raw = nstage[fr / le];
            ok = n_raw >= 1 && n_raw <= stages;
            n = ok ? n_raw : 0;
        }
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

// The callers (wn_api.hip) have checked the arguments.  p.res != NULL: the residual chain over p.S stages (an entry's choice - wn_rvq_*
// at S = 1 is the chain); NULL: one stage, p.S is not read.  p.nstage != NULL (the chain alone): stage counts per clip.
static int vq_stages(const WnVq& p) { return p.res ? p.S : 1; }

int wn_launch_vq_fwd(const WnVq& p, hipStream_t st) {
    if (p.batch <= 0) return 0;
    if (p.counts) {
        hipError_t e = hipMemsetAsync(p.counts, 0, sizeof(int32_t) * vq_stages(p) * p.K, st);
        if (e != hipSuccess) return wn_set_error(e, __FILE__, __LINE__);
    }
    const double n = (double)p.batch * p.le * p.bw;        // with stage counts too, the FIXED denominator: vq_loss is the batch expectation
    const auto k = !p.res ? vq_fwd_k<false, false> : p.nstage ? vq_fwd_k<true, true> : vq_fwd_k<true, false>;
    hipLaunchKernelGGL(k, dim3(WN_VQ_PARTIALS), dim3(64 * NWV), 0, st, p, (float)(1.0 / n));
    WN_CHECK_LAUNCH();
    return 0;
}

template <bool STATS>
static auto vq_bwd_kernel(const WnVq& p) {
    return !p.res ? vq_bwd_k<false, false, STATS> : p.nstage ? vq_bwd_k<true, true, STATS> : vq_bwd_k<true, false, STATS>;
}

// stat != NULL: the stats form (EMA mode)
int wn_launch_vq_bwd(const WnVq& p, float beta, float g_scale, float* stat, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const long total = (long)p.batch * p.le * p.bw;
    const double s = 2.0 / (double)total;
    const int code_blocks = (p.K + CWV - 1) / CWV;
    const int elem_blocks = (int)std::min<long>((total + 64 * CWV - 1) / (64 * CWV), 256);
    hipLaunchKernelGGL(stat ? vq_bwd_kernel<true>(p) : vq_bwd_kernel<false>(p), dim3(vq_stages(p) * code_blocks + elem_blocks), dim3(64 * CWV),
                       0, st, p, (float)((double)g_scale * beta * s), (float)((double)g_scale * s), code_blocks, stat);
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

// nstage NULL: q = the sum of the first `stages` stages' rows (1: the plain lookup); else `stages` = S and every clip takes its own count
int wn_launch_vq_lookup(const int32_t* idx, const int32_t* nstage, const float* flat, long cb_off, float* q_out, int32_t* bad, int stages,
                        int K, int bw, int le, int batch, hipStream_t st) {
    if (batch <= 0) return 0;
    if (bad) {
        hipError_t e = hipMemsetAsync(bad, 0, sizeof(int32_t), st);
        if (e != hipSuccess) return wn_set_error(e, __FILE__, __LINE__);
    }
    const long total = (long)batch * le * bw;
    hipLaunchKernelGGL(nstage ? vq_lookup_k<true> : vq_lookup_k<false>, dim3((unsigned)std::min<long>((total + 255) / 256, 1024)), dim3(256), 0,
                       st, idx, nstage, flat + cb_off, q_out, bad, stages, K, bw, le, total, (long)batch * le);
    WN_CHECK_LAUNCH();
    return 0;
}

