// The tables of a PHASE-conditioned WaveNet (wn_phase_tab_fwd / wn_phase_tab_bwd in include/wavenet_hip.h): a code prior over a
// residual-VQ token stream knows which stage it is at from the stream position alone, p mod P, so the stage is conditioning, not part
// of the token.  The model owns one learned column per phase: T_i [2 Dd][P] per block (gate rows first, like G_i) and T_f [Sd][P].
// Clip b, whose first target sits at stream position pos[b], reads them through a table of P frames in the TILE mode of the block
// kernels (frame = (t - t_lo) mod P); stage i's frame l is the parameter's column (l + pos[b] + rot[i]) mod P - rot[i] carries the
// stage's own t_lo, so that the kernels that read the tables stay as they are.
//
//   forward    tab_i[b][row][l] = (class column of clip b +) T_i[c][(l + pos[b] + rot[i]) mod P]; padding rows exact zeros; enf alike.
//              A thread per element of the per-clip table, frames fastest: its stores to `tab` are one contiguous run, those to
//              `tab_pair` runs of ch P floats (>= 128 bytes), whatever P is - no thread owns a row of an odd number of floats.
//              The parameter's row of P floats is read out of the cache.                                              (phase_fwd_k)
//   backward   dT_i[c][s] = sum_b d_en_i[b][c][(s - pos[b] - rot[i]) mod P], b ascending from +0: a thread per (row, s), s fastest,
//              the stores of a stage one run; behind them, a thread per le = 1 element sums its P frames in ascending l (the sums
//              wn_gclass_bwd consumes: one formula serves the per-clip and the pair layout, both are [..][rows][P]).   (phase_bwd_k)
//
// fp32, a fixed order, no atomics: the same bits at every launch.  No LDS.  A negative pos[b] is never used as an index: the forward
// turns that clip's rows into NaN, the backward its share of every dT.
#include "wn_common.h"
#include "wn_kernels.h"

namespace {

// (pos + rot) mod P, the mathematical one, in [0, P); pos >= 0 here
__device__ __forceinline__ int phase_shift(const WnPhase& p, int b, int i) {
    const int pm = (int)(p.pos[b] % p.period);
    const int rm = ((p.rot[i] % p.period) + p.period) % p.period;
    return (pm + rm) % p.period;
}
// row (stage i, reference row c) of the phase tables: [period] floats of flat / flat_grad
__device__ __forceinline__ long phase_row(const WnPhase& p, int i, int c) {
    return (i < p.n_stages ? p.pw_off + i * p.pstage_stride : p.pwf_off) + (long)c * p.period;
}

__global__ __launch_bounds__(256) void phase_fwd_k(WnPhase p, long n_tab, long total) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int P = p.period;
    if (e >= n_tab) {                                           // enf [batch][sd][P]
        const long o = e - n_tab;
        const int l = (int)(o % P), c = (int)((o / P) % p.sd), b = (int)(o / ((long)P * p.sd));
        float v = __builtin_nanf("");
        if (p.pos[b] >= 0) v = p.flat[phase_row(p, p.n_stages, c) + (l + phase_shift(p, b, p.n_stages)) % P];
        if (p.add_enf) v = p.add_enf[(long)b * p.sd + c] + v;
        p.enf[o] = v;
        return;
    }
    // element e of the per-clip tables [n_stages][batch][2 ch][P]: rows [f | g], each half padded to ch
    const int l = (int)(e % P);
    long r = e / P;
    const int cc = (int)(r % p.ch); r /= p.ch;
    const int half = (int)(r % 2); r /= 2;
    const int b = (int)(r % p.batch), i = (int)(r / p.batch);
    const long one = ((long)i * p.batch + b) * 2 * p.ch + half * p.ch + cc;                                  // its le = 1 elements
    const long two = ((long)i * (p.batch / 2) + (b >> 1)) * 4 * p.ch + half * 2 * p.ch + (b & 1) * p.ch + cc;
    float v = 0.f, vp = 0.f;
    if (cc < p.dd) {
        const int c = half ? cc : p.dd + cc;                   // the reference's row: gate rows [0, dd), filter rows [dd, 2 dd)
        float t = __builtin_nanf("");
        if (p.pos[b] >= 0) t = p.flat[phase_row(p, i, c) + (l + phase_shift(p, b, i)) % P];
        v = vp = t;
        if (p.add_enf) {
            if (p.tab) v = p.add_tab[one] + t;
            if (p.tab_pair) vp = p.add_pair[two] + t;
        }
    }
    if (p.tab) p.tab[e] = v;
    if (p.tab_pair) p.tab_pair[two * P + l] = vp;
}

__global__ __launch_bounds__(256) void phase_bwd_k(WnPhase p, long n_par, long n_sum_tab, long total) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int P = p.period;
    if (e >= n_par) {                                           // the frame sums, le = 1 layouts (only with sum_tab / sum_enf)
        const long o = e - n_par;
        const float* src = o < n_sum_tab ? p.d_tab + o * P : p.d_enf + (o - n_sum_tab) * P;
        float s = 0.f;
        for (int l = 0; l < P; ++l) s += src[l];
        if (o < n_sum_tab) p.sum_tab[o] = s; else p.sum_enf[o - n_sum_tab] = s;
        return;
    }
    const int s = (int)(e % P), r = (int)(e / P), n2 = p.n_stages * 2 * p.dd;
    int i = p.n_stages, c = r - n2;
    if (r < n2) { i = r / (2 * p.dd); c = r - i * 2 * p.dd; }
    const int rows = p.d_pair ? 4 * p.ch : 2 * p.ch, nt = p.d_pair ? p.batch / 2 : p.batch;
    const int row = c < p.dd ? (p.d_pair ? 2 * p.ch : p.ch) + c : c - p.dd;            // gate rows behind the filter rows
    float acc = 0.f;
    for (int b = 0; b < p.batch; ++b) {
        float d = __builtin_nanf("");
        if (p.pos[b] >= 0) {
            const int l = (s - phase_shift(p, b, i) + P) % P;
            d = i == p.n_stages ? p.d_enf[((long)b * p.sd + c) * P + l]
              : p.d_pair ? p.d_tab[(((long)i * nt + (b >> 1)) * rows + row + (b & 1) * p.ch) * P + l]
                         : p.d_tab[(((long)i * nt + b) * rows + row) * P + l];
        }
        acc += d;
    }
    p.flat_grad[phase_row(p, i, c) + s] = acc;
}

}  // namespace

// The callers (wn_api.hip) have checked the arguments.
int wn_launch_phase_tab_fwd(const WnPhase& p, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const long n_tab = (long)p.n_stages * p.batch * 2 * p.ch * p.period, total = n_tab + (long)p.batch * p.sd * p.period;
    const long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) return wn_set_error_msg(-4, "wn_phase_tab_fwd: the tables have too many elements for one grid");
    hipLaunchKernelGGL(phase_fwd_k, dim3((unsigned)blocks), dim3(256), 0, st, p, n_tab, total);
    WN_CHECK_LAUNCH();
    return 0;
}

int wn_launch_phase_tab_bwd(const WnPhase& p, hipStream_t st) {
    if (p.batch <= 0) return 0;
    const long n_par = ((long)p.n_stages * 2 * p.dd + p.sd) * p.period;
    const long n_sum_tab = p.sum_tab ? (long)p.n_stages * p.batch * 2 * p.ch : 0, n_sum = p.sum_tab ? n_sum_tab + (long)p.batch * p.sd : 0;
    const long total = n_par + n_sum, blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffL) return wn_set_error_msg(-4, "wn_phase_tab_bwd: the tables have too many elements for one grid");
    hipLaunchKernelGGL(phase_bwd_k, dim3((unsigned)blocks), dim3(256), 0, st, p, n_par, n_sum_tab, total);
    WN_CHECK_LAUNCH();
    return 0;
}
