// C ABI of libwavenet_hip.so (declared in include/wavenet_hip.h): argument marshalling only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/wavenet_hip.h"
#include "wn_common.h"
#include "wn_kernels.h"

static_assert(WN_COND_IDX_PAD == WN_PQ_IDX_PAD, "public and kernel-side pad of the bucket bytes differ");
static thread_local char g_err[512] = "";

int wn_set_error(hipError_t e, const char* file, int line) {
    snprintf(g_err, sizeof(g_err), "HIP error %d (%s) at %s:%d", (int)e, hipGetErrorString(e), file, line);
    return -1;
}
int wn_tile_origin(int t_lo) { return t_lo & ~63; }       // 64 samples = two 128-byte lines of a row (29.7 -> 27.3 us per forward block)

// compute units of the current device (all devices of a node are the same part: asked once)
int wn_num_cus() {
    static std::atomic<int> cus{0};
    int v = cus.load(std::memory_order_relaxed);
    if (v > 0) return v;
    int dev = 0;
    hipDeviceProp_t pr;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&pr, dev) != hipSuccess || pr.multiProcessorCount <= 0) return 256;
    cus.store(pr.multiProcessorCount, std::memory_order_relaxed);
    return pr.multiProcessorCount;
}

int wn_xcd_swizzle_enabled() { return 1; }                 // the XCD-aware block remap is always on (speed only: wn_common.h)

int wn_set_error_msg(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

// Required pointers of a call that has work to do: a NULL one is reported (-4, the argument's name in wn_last_error) before anything is
// launched - the alternative is a memory fault on the device, which takes the caller's process with it.
static int wn_null_error(const char* fn, const char* names, int which) {
    const char* b = names;
    for (int i = 0; i < which && *b; ++b)
        if (*b == ',') ++i;
    while (*b == ' ') ++b;
    int len = 0;
    while (b[len] && b[len] != ',') ++len;
    snprintf(g_err, sizeof(g_err), "%s: argument '%.*s' must not be NULL", fn, len, b);
    return -4;
}
#define WN_REQUIRE(fn, ...)                                                          \
    do {                                                                             \
        const void* wn_req_[] = {__VA_ARGS__};                                       \
        for (int wn_i_ = 0; wn_i_ < (int)(sizeof(wn_req_) / sizeof(wn_req_[0])); ++wn_i_) \
            if (!wn_req_[wn_i_]) return wn_null_error(fn, #__VA_ARGS__, wn_i_);      \
    } while (0)

static_assert(WN_F16X3 == WN_MODE_F16X3 && WN_F16X1 == WN_MODE_F16X1 && WN_BF16X3 == WN_MODE_BF16X3 &&
              WN_BF16X1 == WN_MODE_BF16X1, "mode enums out of sync");
static_assert(WN_CE_NUM_PARTIALS == WN_CE_PARTIALS, "partials out of sync");
static_assert(WN_VQ_NUM_PARTIALS == WN_VQ_PARTIALS && WN_VQ_MAX_CODES == WN_DEC_MAX_Q, "vq constants out of sync");
static_assert(WN_VQ_MAX_CODES == WN_VQ_MAX_K && WN_VQ_EMA_WORK_BYTES == WN_VQ_EMA_WORK, "vq ema constants out of sync");
static_assert(WN_RVQ_MAX_STAGES == WN_RVQ_MAX_S, "rvq constants out of sync");

// ---- cached-queue decode: the ONE call path behind the eight exported decode entries (wn_decode .. wn_decode_batch_samp,
// wn_win_decode_batch and wn_cfg_decode_batch)------------------------------------------------------------------------------------------------------
// Every entry forwards its arguments (and the defaults of those it does not take) to decode_checked with the checks it applies:
enum : unsigned {
    DEC_FW = 1,       // takes filter_width: it, Q and the note / history pointers are checked, under the entry's own name
    DEC_COND = 2,     // takes conditioning tables: corrected recurrence only; le, n_layers and the schedule arrays are checked
    DEC_SAMP = 4,     // takes top_k / top_p: the scalar form's filters are checked
    DEC_WIN = 8,      // takes a sampling-window table: its period, pairs and position are checked against Q
    DEC_CFG = 16,     // takes a guidance table: the rows are (conditional, unconditional) pairs - an even count, with conditioning tables
};

static int decode_refuse(const char* fn, const char* text) {
    snprintf(g_err, sizeof(g_err), "%s: %s", fn, text);
    return -4;
}

// A host window table (lo0, hi0, lo1, hi1, ..: win_period pairs) and the stream position of the call's first step or row, checked
// under the entry's name `fn` and copied into the kernel-argument form: the position arrives reduced mod the period.
static int win_checked(const char* fn, const int32_t* win_host, int win_period, int64_t win_pos0, int Q, int& period, int& pos0,
                       int (&lo)[WN_WIN_MAX], int (&hi)[WN_WIN_MAX]) {
    if (win_period < 0 || win_period > WN_WIN_MAX) return decode_refuse(fn, "'win_period' must be 0 (no windows) .. 16 pairs");
    if (win_period > 0 && !win_host) return decode_refuse(fn, "'win_host' is NULL with win_period > 0");
    for (int j = 0; j < win_period; ++j)
        if (win_host[2 * j] < 0 || win_host[2 * j + 1] > Q || win_host[2 * j] >= win_host[2 * j + 1]) {
            snprintf(g_err, sizeof(g_err), "%s: 'win_host' pair %d is (%d, %d): every window needs 0 <= lo < hi <= Q", fn, j,
                     (int)win_host[2 * j], (int)win_host[2 * j + 1]);
            return -4;
        }
    if (win_pos0 < 0) return decode_refuse(fn, "'win_pos0' (stream position of the first step) must be >= 0");
    period = win_period;
    pos0 = win_period > 0 ? (int)(win_pos0 % win_period) : 0;
    for (int j = 0; j < win_period; ++j) { lo[j] = win_host[2 * j]; hi[j] = win_host[2 * j + 1]; }
    return 0;
}

// Makes every refusal of a decode call, in the one order all entries share, then fills WnDecodeArgs and launches.  `fn`: the calling
// entry; `sync_ustride`: uint64 words of hand-off scratch per utterance.  The checks every entry applies report as "wn_decode".
static int decode_checked(const char* fn, unsigned checks, int64_t sync_ustride, int filter_width, int n_layers, int R, int D, int S,
                          int Q, const int32_t* dilations_host, const int64_t* q_off_host, float* queues, const float* w_causal,
                          const float* b_causal, const float* w_layers, int64_t layer_stride, const float* b_layers,
                          const float* w_p1, const float* b_p1, const float* w_p2, const float* b_p2, const float* note0,
                          const float* prev0, float* note_out, float* prev_out, const int32_t* forced, int32_t* codes_out,
                          float* probs_out, int64_t step0, int n_steps, int push_input, uint64_t* sync, int n_utt,
                          int64_t queues_ustride, float temperature, uint64_t seed, const uint16_t* pk, int64_t pk_fg0,
                          int64_t pk_d0, int64_t pk_lstride, int64_t pk_skip, int64_t pk_p1, int64_t pk_p2, const float* cond_fg,
                          int64_t cond_fg_ustride, const float* cond_p1, int64_t cond_p1_ustride, const int32_t* c_shift_host,
                          const int32_t* c_q_host, int le, int64_t pos0, const wn_sampling* samp, int top_k, float top_p,
                          const int32_t* win_host, int win_period, int64_t win_pos0, const float* guidance, wn_stream_t stream) {
    const bool layers_ok = n_layers >= 1 && n_layers <= WN_DEC_MAX_LAYERS;
    if ((checks & DEC_SAMP) && !samp) {   // (a table's entries are normalised on the device: out of range = filter off)
        if (!(top_p >= 0.0f)) return decode_refuse(fn, "'top_p' must be a number >= 0 (0 or >= 1: no nucleus filter)");
        if (top_k < 0) return decode_refuse(fn, "'top_k' must be >= 0 (0 or >= Q: no top-k filter)");
    }
    if ((checks & DEC_FW) && filter_width < 1) return decode_refuse(fn, "filter_width must be >= 1");
    if (!push_input) {
        if (checks & DEC_COND) return decode_refuse(fn, "conditioned decode exists for the corrected recurrence only; pass push_input = 1");
        if ((checks & DEC_FW) && filter_width != 2)
            return decode_refuse(fn, "the as-written queue push (push_input = 0) exists for filter_width 2 only; pass push_input = 1 "
                                     "(the corrected recurrence)");
    }
    if ((checks & DEC_COND) && le < 1) return decode_refuse(fn, "le (columns of a conditioning table) must be >= 1");
    if ((checks & DEC_FW) && (Q < 1 || Q > WN_DEC_MAX_Q)) return decode_refuse(fn, "1 <= Q <= 1024 quantisation channels");
    if (checks & DEC_COND) {              // (the schedule arrays hold n_layers + 1 entries: the layer count is checked first)
        if (!layers_ok) return decode_refuse(fn, "1..64 layers supported");
        if (cond_fg || cond_p1) {
            if (!c_shift_host || !c_q_host)
                return decode_refuse(fn, "a conditioning table needs the schedule arrays 'c_shift_host' and 'c_q_host' (n_layers + 1 "
                                         "entries each)");
            for (int i = 0; i <= n_layers; ++i)
                if (c_q_host[i] < 0) return decode_refuse(fn, "c_q[i] must be >= 0 (stretch factor, or 0 = tile)");
        }
    }
    if ((checks & DEC_FW) && n_utt > 0 && n_steps > 0) {
        WN_REQUIRE(fn, note0, note_out, codes_out);
        if (filter_width > 1) WN_REQUIRE(fn, prev0, prev_out);
    }
    WnDecodeArgs a;
    memset(&a, 0, sizeof(a));
    if (checks & DEC_WIN) {               // (Q is in range here: DEC_WIN comes with DEC_FW)
        const int rc = win_checked(fn, win_host, win_period, win_pos0, Q, a.win_period, a.win_pos0, a.win_lo, a.win_hi);
        if (rc) return rc;
    }
    if ((checks & DEC_CFG) && guidance) {
        if (n_utt > 0 && (n_utt & 1))
            return decode_refuse(fn, "'guidance' makes the rows (conditional, unconditional) pairs: 'n_utt' must be even");
        if (!cond_fg && !cond_p1)
            return decode_refuse(fn, "'guidance' needs the conditioning tables 'cond_fg' / 'cond_p1' (without them both members of a "
                                     "pair are the same model)");
    }
    if (n_utt <= 0) return 0;
    if (!layers_ok) return decode_refuse("wn_decode", "1..64 layers supported");
    WN_REQUIRE("wn_decode", dilations_host, q_off_host);              // (host arrays, read right here)
    if (n_steps > 0) WN_REQUIRE("wn_decode", queues, w_causal, w_layers, w_p1, w_p2, sync);
    a.n_layers = n_layers; a.R = R; a.D = D; a.S = S; a.Q = Q; a.fw = filter_width;
    for (int i = 0; i < n_layers; ++i) { a.dil[i] = dilations_host[i]; a.q_off[i] = q_off_host[i]; }
    a.queues = queues; a.w_causal = w_causal; a.b_causal = b_causal; a.w_layers = w_layers; a.layer_stride = layer_stride;
    a.b_layers = b_layers; a.w_p1 = w_p1; a.b_p1 = b_p1; a.w_p2 = w_p2; a.b_p2 = b_p2;
    a.note0 = note0; a.prev0 = prev0; a.note_out = note_out; a.prev_out = prev_out; a.forced = forced;
    a.codes_out = codes_out; a.probs_out = probs_out; a.step0 = step0; a.n_steps = n_steps; a.push_input = push_input;
    a.dbg = 0;
    a.sync = reinterpret_cast<unsigned long long*>(sync);
    a.sync_ustride = sync_ustride;
    a.n_utt = n_utt; a.queues_ustride = queues_ustride;
    a.sample = temperature > 0.0f ? 1 : 0; a.inv_temp = temperature > 0.0f ? 1.0f / temperature : 1.0f; a.seed = seed;
    a.samp = reinterpret_cast<const WnSampling*>(samp); a.top_k = top_k; a.top_p = top_p;
    a.pk_skip = -1;
    a.cond_fg = cond_fg; a.cond_fg_ustride = cond_fg_ustride; a.cond_p1 = cond_p1; a.cond_p1_ustride = cond_p1_ustride;
    a.le = le; a.pos0 = pos0;
    a.guidance = (checks & DEC_CFG) ? guidance : nullptr;
    if (cond_fg || cond_p1)
        for (int i = 0; i <= n_layers; ++i) { a.c_shift[i] = c_shift_host[i]; a.c_q[i] = c_q_host[i]; }
    // the matrix-core kernel needs all of pk (chain, skip, post-processing: 64 / 64 / 256 / 256 channels); biases are fine
    const bool any_bias = b_layers || b_causal || b_p1 || b_p2;
    const bool post_pk = (S == 256 || S == 512) && Q == 256 && pk_skip >= 0 && pk_p1 >= 0 && pk_p2 >= 0;
    if (pk && R == 64 && D == 64 && (post_pk || !any_bias)) {
        a.pk = pk; a.pk_fg0 = pk_fg0; a.pk_d0 = pk_d0; a.pk_lstride = pk_lstride;
        if (post_pk) { a.pk_skip = pk_skip; a.pk_p1 = pk_p1; a.pk_p2 = pk_p2; }
    }
    return wn_launch_decode(a, (hipStream_t)stream);
}

// The two sampler entries' one body: the refusals under the entry's name `fn`, then the launch (`win`: the entry takes a table).
// `logits_u`, `guidance`: the guided entry's second matrix and per-row scales (guidance NULL: the plain sampler on `logits`).
static int sample_checked(const char* fn, bool win, const float* logits, int64_t n, int Q, int64_t ld, const wn_sampling* samp,
                          float temperature, uint64_t seed, int top_k, float top_p, int64_t step0, const float* u, int32_t* codes,
                          float* probs, const int32_t* win_host, int win_period, int64_t win_pos0, wn_stream_t stream,
                          const float* logits_u = nullptr, const float* guidance = nullptr) {
    if (Q < 1 || Q > WN_DEC_MAX_Q) return decode_refuse(fn, "1 <= 'Q' <= 1024 entries per row");
    if (n < 0) return decode_refuse(fn, "'n' (rows) must be >= 0");
    if (ld < Q) return decode_refuse(fn, "'ld' (row stride) must be >= Q");
    if (!samp) {
        if (!(top_p >= 0.0f)) return decode_refuse(fn, "'top_p' must be a number >= 0 (0 or >= 1: no nucleus filter)");
        if (top_k < 0) return decode_refuse(fn, "'top_k' must be >= 0 (0 or >= Q: no top-k filter)");
    }
    WnWin w;
    memset(&w, 0, sizeof(w));
    if (win) {
        const int rc = win_checked(fn, win_host, win_period, win_pos0, Q, w.period, w.pos0, w.lo, w.hi);
        if (rc) return rc;
    }
    if (n == 0) return 0;
    WN_REQUIRE(fn, logits, codes);
    if (guidance) {
        WN_REQUIRE(fn, logits_u);
        return wn_launch_cfg_sample_logits(logits, logits_u, guidance, (long)n, Q, (long)ld, reinterpret_cast<const WnSampling*>(samp),
                                           temperature, seed, top_k, top_p, (long)step0, u, codes, probs, w, (hipStream_t)stream);
    }
    return wn_launch_sample_logits(logits, (long)n, Q, (long)ld, reinterpret_cast<const WnSampling*>(samp), temperature, seed, top_k,
                                   top_p, (long)step0, u, codes, probs, w, (hipStream_t)stream);
}

extern "C" {

int wn_version(void) { return WN_ABI_VERSION; }
const char* wn_last_error(void) { return g_err; }

int wn_pack_weights(const float* flat, const int32_t* idx, uint16_t* out, int n, int mode, wn_stream_t stream) {
    if (n % 512 != 0) return wn_set_error_msg(-4, "wn_pack_weights: n must be a multiple of 512");
    if (n > 0) WN_REQUIRE("wn_pack_weights", flat, idx, out);
    return wn_launch_pack(flat, idx, out, n, wn_mode_is_bf16(mode), wn_mode_ns(mode), (hipStream_t)stream);
}

int wn_chan_gemm(const float* in0, const float* in1, int64_t in_bstride, int in_pitch, int in_lo, int in_hi,
                 int shift0, int shift1, int ks0, int ks1, const uint16_t* wpack, int mt, int m_valid,
                 float* out, int64_t out_bstride, int out_pitch, int out_shift, const float* bias,
                 const float* resid, int64_t resid_bstride, int resid_pitch, int resid_lo,
                 const float* mask, int64_t mask_bstride, int mask_pitch,
                 int t_lo, int t_hi, int relu_in, int batch, int mode, wn_stream_t stream) {
    if (ks0 <= 0 || (ks1 > 0 && !in1) || mt <= 0) return wn_set_error_msg(-4, "wn_chan_gemm: bad shape");
    if (batch > 0 && t_hi > t_lo) WN_REQUIRE("wn_chan_gemm", in0, wpack, out);
    WnGemmArgs a;
    memset(&a, 0, sizeof(a));
    a.in0 = in0; a.in1 = ks1 > 0 ? in1 : nullptr; a.in_bstride = in_bstride; a.in_pitch = in_pitch; a.in_lo = in_lo; a.in_hi = in_hi;
    a.shift0 = shift0; a.shift1 = shift1; a.ks0 = ks0; a.ks1 = ks1 > 0 ? ks1 : 0; a.wpack = wpack; a.mt = mt; a.m_valid = m_valid;
    a.out = out; a.out_bstride = out_bstride; a.out_pitch = out_pitch; a.out_shift = out_shift; a.bias = bias;
    a.resid = resid; a.resid_bstride = resid_bstride; a.resid_pitch = resid_pitch; a.resid_lo = resid_lo;
    a.mask = mask; a.mask_bstride = mask_bstride; a.mask_pitch = mask_pitch;
    a.t_lo = t_lo; a.t_hi = t_hi; a.relu_in = relu_in;
    return wn_launch_gemm(a, batch, mode, (hipStream_t)stream);
}

int wn_skip_epilogue_fwd(const float* z, int64_t z_bstride, int pitch, int ks_skip, const uint16_t* w_skip, const float* bias_skip,
                         float* u, float* h, int64_t s_bstride, const uint16_t* w_p1c, const float* bias_p1,
                         const uint16_t* w_p2c, const float* bias_p2, float* o, int64_t o_bstride, int o_pitch,
                         int s_valid, int q_valid, int t_lo, int t_hi, int batch, int mode, wn_stream_t stream) {
    if (pitch % 4 != 0) return wn_set_error_msg(-4, "wn_skip_epilogue_fwd: pitch must be a multiple of 4");
    if (s_valid <= 0 || s_valid > 256 || q_valid <= 0 || q_valid > 256)
        return wn_set_error_msg(-4, "wn_skip_epilogue_fwd: at most 256 skip and 256 quantisation channels (wn_chan_gemm covers the rest)");
    if (batch > 0 && t_hi > t_lo) WN_REQUIRE("wn_skip_epilogue_fwd", z, w_skip, u, h, w_p1c, w_p2c, o);
    WnEpiFwdArgs a;
    memset(&a, 0, sizeof(a));
    a.z = z; a.z_bstride = z_bstride; a.pitch = pitch; a.ks_skip = ks_skip; a.w_skip = w_skip; a.bias_s = bias_skip;
    a.u = u; a.h = h; a.s_bstride = s_bstride; a.w_p1c = w_p1c; a.bias_1 = bias_p1; a.w_p2c = w_p2c; a.bias_2 = bias_p2;
    a.o = o; a.o_bstride = o_bstride; a.o_pitch = o_pitch; a.s_valid = s_valid; a.q_valid = q_valid; a.t_lo = t_lo; a.t_hi = t_hi;
    return wn_launch_skip_epilogue_fwd(a, batch, mode, (hipStream_t)stream);
}

int wn_skip_epilogue_bwd(const float* d_o, int64_t o_bstride, int o_pitch, const float* h, const float* u, int64_t s_bstride, int pitch,
                         float* d_h, float* d_u, float* d_z, int64_t z_bstride, const uint16_t* w_p2T, const uint16_t* w_p1Tc,
                         const uint16_t* w_skipTc, int mt_z, int z_valid, int s_valid, int t_lo, int t_hi, int batch, int mode,
                         wn_stream_t stream) {
    if (pitch % 4 != 0) return wn_set_error_msg(-4, "wn_skip_epilogue_bwd: pitch must be a multiple of 4");
    if (s_valid <= 0 || s_valid > 256) return wn_set_error_msg(-4, "wn_skip_epilogue_bwd: at most 256 skip channels");
    if (batch > 0 && t_hi > t_lo) WN_REQUIRE("wn_skip_epilogue_bwd", d_o, h, u, d_h, d_u, d_z, w_p2T, w_p1Tc, w_skipTc);
    WnEpiBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.d_o = d_o; a.o_bstride = o_bstride; a.o_pitch = o_pitch; a.h = h; a.u = u; a.s_bstride = s_bstride; a.pitch = pitch;
    a.d_h = d_h; a.d_u = d_u; a.d_z = d_z; a.z_bstride = z_bstride; a.w_p2T = w_p2T; a.w_p1Tc = w_p1Tc; a.w_skipTc = w_skipTc;
    a.mt_z = mt_z; a.z_valid = z_valid; a.s_valid = s_valid; a.t_lo = t_lo; a.t_hi = t_hi;
    return wn_launch_skip_epilogue_bwd(a, batch, mode, (hipStream_t)stream);
}

int wn_enc_resblock_fwd(const float* x_in, float* x_out, float* h_out, int64_t x_bstride, int64_t h_bstride, int pitch,
                        const uint16_t* wdil, const uint16_t* wd, const float* bias_dil, const float* bias_d, int n_h,
                        int n_d, int ch, int d, int t_lo, int t_hi, int batch, int mode, wn_stream_t stream) {
    if (pitch % 4 != 0) return wn_set_error_msg(-4, "wn_enc_resblock_fwd: pitch must be a multiple of 4");
    if (t_lo < d + 1) return wn_set_error_msg(-4, "wn_enc_resblock_fwd: t_lo must be >= d + 1");
    if (batch > 0 && t_hi > t_lo) WN_REQUIRE("wn_enc_resblock_fwd", x_in, x_out, h_out, wdil, wd);
    WnResArgs a;
    memset(&a, 0, sizeof(a));
    a.x_in = x_in; a.x_out = x_out; a.z_out = h_out; a.x_bstride = x_bstride; a.z_bstride = h_bstride; a.pitch = pitch;
    a.wfg = wdil; a.wd = wd; a.bias_f = bias_dil; a.bias_g = nullptr; a.bias_d = bias_d; a.n_f = n_h; a.n_d = n_d;
    a.d = d; a.t_lo = t_lo; a.t_hi = t_hi; a.z_lo = t_lo; a.write_x = 1;
    return wn_launch_enc_resblock_fwd(a, ch, batch, mode, (hipStream_t)stream);
}

int wn_resblock_fwd(const float* x_in, float* x_out, float* z_out, int64_t x_bstride, int64_t z_bstride,
                    int pitch, const uint16_t* wfg, const uint16_t* wd, const float* bias_f,
                    const float* bias_g, const float* bias_d, int n_f, int n_d, int ch, int d,
                    int t_lo, int t_hi, int z_lo, int write_x, const float* cond, int64_t cond_bstride,
                    int cond_pitch, int cond_mode, int cond_le, int cond_q, const uint16_t* cond_pack,
                    int64_t cond_pack_bstride, const uint8_t* cond_idx, int64_t z_half_stride, int batch, int mode,
                    wn_stream_t stream) {
    if (pitch % 4 != 0) return wn_set_error_msg(-4, "wn_resblock_fwd: pitch must be a multiple of 4");
    if (cond && (cond_le <= 0 || (cond_mode == 1 && cond_q <= 0) || (cond_mode != 1 && cond_mode != 2)))
        return wn_set_error_msg(-4, "wn_resblock_fwd: bad conditioning arguments");
    if (t_lo < d + 1) return wn_set_error_msg(-4, "wn_resblock_fwd: t_lo must be >= d + 1");
    if (batch > 0 && t_hi > t_lo) {
        WN_REQUIRE("wn_resblock_fwd", x_in, wfg, wd, z_out);
        if (write_x) WN_REQUIRE("wn_resblock_fwd", x_out);
    }
    WnResArgs a;
    memset(&a, 0, sizeof(a));
    a.x_in = x_in; a.x_out = x_out; a.z_out = z_out; a.x_bstride = x_bstride; a.z_bstride = z_bstride; a.pitch = pitch;
    a.wfg = wfg; a.wd = wd; a.bias_f = bias_f; a.bias_g = bias_g; a.bias_d = bias_d; a.n_f = n_f; a.n_d = n_d;
    a.d = d; a.t_lo = t_lo; a.t_hi = t_hi; a.z_lo = z_lo; a.write_x = write_x;
    a.cond = cond; a.cond_bstride = cond_bstride; a.cond_pitch = cond_pitch; a.cond_mode = cond_mode;
    a.cond_le = cond_le; a.cond_q = cond_q;
    if (cond && cond_pack && cond_idx) { a.cond_pack = cond_pack; a.cond_pack_bstride = cond_pack_bstride; a.cond_idx = cond_idx; }
    if (z_half_stride && ch != 64) return wn_set_error_msg(-4, "wn_resblock_fwd: z_half_stride is for two 32-channel clips on the 64-channel block");
    a.z_half = z_half_stride;
    return wn_launch_resblock_fwd(a, ch, batch, mode, (hipStream_t)stream);
}

int wn_resblock_bwd(const float* x_in, const float* dy, const float* dz, float* dfg, float* z,
                    int64_t x_bstride, int64_t dz_bstride, int64_t dfg_bstride, int64_t z_bstride,
                    int pitch, const uint16_t* wfg, const uint16_t* wdT, const float* bias_f,
                    const float* bias_g, int n_f, int ch, int d, int t_lo, int t_hi, int z_lo,
                    const float* cond, int64_t cond_bstride, int cond_pitch, int cond_mode, int cond_le, int cond_q,
                    int batch, int mode_fwd, int mode_bwd, wn_stream_t stream) {
    if (pitch % 4 != 0) return wn_set_error_msg(-4, "wn_resblock_bwd: pitch must be a multiple of 4");
    if (batch > 0 && t_hi > t_lo) {
        WN_REQUIRE("wn_resblock_bwd", x_in, dz, dfg, wfg);
        if (dy) WN_REQUIRE("wn_resblock_bwd", wdT);
    }
    WnResBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.x_in = x_in; a.dy = dy; a.dz = dz; a.dfg = dfg; a.z = z;
    a.x_bstride = x_bstride; a.dz_bstride = dz_bstride; a.dfg_bstride = dfg_bstride; a.z_bstride = z_bstride; a.pitch = pitch;
    a.wfg = wfg; a.wdT = wdT; a.bias_f = bias_f; a.bias_g = bias_g; a.n_f = n_f;
    a.d = d; a.t_lo = t_lo; a.t_hi = t_hi; a.z_lo = z_lo;
    a.cond = cond; a.cond_bstride = cond_bstride; a.cond_pitch = cond_pitch; a.cond_mode = cond_mode;
    a.cond_le = cond_le; a.cond_q = cond_q;
    return wn_launch_resblock_bwd(a, ch, batch, mode_fwd, mode_bwd, (hipStream_t)stream);
}

int wn_wgrad(const float* a_, int64_t a_bstride, int a_pitch, int a_shift, int a_cols,
             const float* b0, const float* b1, int64_t b_bstride, int b_pitch, int b_shift0,
             int b_shift1, int b_cols, int nt_per_tap, int mt, int relu_b, float* c, int ldc,
             int64_t c_slab_stride, int t_lo, int t_hi, int chunk, int batch, int mode, wn_stream_t stream) {
    if (c_slab_stride < (int64_t)mt * 16 * ldc) return wn_set_error_msg(-4, "wn_wgrad: slab stride smaller than C");
    if (batch > 0 && t_hi > t_lo) WN_REQUIRE("wn_wgrad", a_, b0, c);
    WnWgradArgs a;
    memset(&a, 0, sizeof(a));
    a.a = a_; a.a_bstride = a_bstride; a.a_pitch = a_pitch; a.a_shift = a_shift; a.a_cols = a_cols;
    a.b0 = b0; a.b1 = b1; a.b_bstride = b_bstride; a.b_pitch = b_pitch; a.b_shift0 = b_shift0; a.b_shift1 = b_shift1; a.b_cols = b_cols;
    a.nt_per_tap = nt_per_tap; a.mt = mt; a.relu_b = relu_b; a.c = c; a.ldc = ldc; a.c_slab_stride = c_slab_stride;
    a.t_lo = t_lo; a.t_hi = t_hi; a.chunk = chunk;
    return wn_launch_wgrad(a, batch, mode, (hipStream_t)stream);
}

int wn_wgrad_slabs(int t_lo, int t_hi, int chunk, int batch) { return wn_wgrad_num_slabs(t_lo, t_hi, chunk, batch); }

int wn_reduce_slabs(const int64_t* desc, int n_ops, int64_t total_vec, const float* slab, float* out, wn_stream_t stream) {
    if (n_ops > 0 && total_vec > 0) WN_REQUIRE("wn_reduce_slabs", desc, slab, out);
    return wn_launch_reduce_slabs(reinterpret_cast<const long*>(desc), n_ops, total_vec, slab, out, (hipStream_t)stream);
}

int wn_bias_grad(const float* a, int64_t a_bstride, int a_pitch, int a_shift, int rows, int t_lo,
                 int t_hi, int batch, float* out, wn_stream_t stream) {
    if (batch > 0 && t_hi > t_lo && rows > 0) WN_REQUIRE("wn_bias_grad", a, out);
    return wn_launch_bias_grad(a, a_bstride, a_pitch, a_shift, rows, t_lo, t_hi, batch, out, (hipStream_t)stream);
}

int wn_chunk_softmax256_fwd(const float* x, float* y, int64_t nrows, wn_stream_t stream) {
    if (nrows > 0) WN_REQUIRE("wn_chunk_softmax256_fwd", x, y);
    return wn_launch_softmax_fwd(x, y, nrows, (hipStream_t)stream);
}
int wn_chunk_softmax256_bwd(const float* y, const float* dy, float* dx, int64_t nrows, wn_stream_t stream) {
    if (nrows > 0) WN_REQUIRE("wn_chunk_softmax256_bwd", y, dy, dx);
    return wn_launch_softmax_bwd(y, dy, dx, nrows, (hipStream_t)stream);
}
int wn_chunk_softmax256_ce(const float* x, const int64_t* target, float* probs, float* dx,
                           float* loss_part, int64_t nrows, float inv_n, wn_stream_t stream) {
    if (nrows > 0) WN_REQUIRE("wn_chunk_softmax256_ce", x, target);
    return wn_launch_softmax_ce(x, target, probs, dx, loss_part, nrows, inv_n, (hipStream_t)stream);
}
int wn_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                 float beta2, float eps, float bias_corr1, float bias_corr2, float gscale, wn_stream_t stream) {
    if (n > 0) WN_REQUIRE("wn_adam_flat", p, g, m, v);
    return wn_launch_adam(p, g, m, v, n, lr, beta1, beta2, eps, bias_corr1, bias_corr2, gscale, (hipStream_t)stream);
}
int wn_sgd_flat(float* p, const float* g, float* momentum_buf, int64_t n, float lr, float momentum, float gscale, int first_step,
                wn_stream_t stream) {
    if (momentum != 0.f && !momentum_buf) return wn_set_error_msg(-4, "wn_sgd_flat: momentum needs its buffer");
    if (n > 0) WN_REQUIRE("wn_sgd_flat", p, g);
    return wn_launch_sgd(p, g, momentum_buf, n, lr, momentum, gscale, first_step, (hipStream_t)stream);
}
int wn_rmsprop_flat(float* p, const float* g, float* square_avg, float* momentum_buf, int64_t n, float lr, float alpha, float eps,
                    float momentum, float gscale, wn_stream_t stream) {
    if (!square_avg || (momentum > 0.f && !momentum_buf)) return wn_set_error_msg(-4, "wn_rmsprop_flat: missing state buffer");
    if (n > 0) WN_REQUIRE("wn_rmsprop_flat", p, g);
    return wn_launch_rmsprop(p, g, square_avg, momentum_buf, n, lr, alpha, eps, momentum, gscale, (hipStream_t)stream);
}

// ---- guarded step (wn_guard.hip) ----
int wn_grad_guard(const float* g, int64_t n, float gscale, float max_norm, int skip_nonfinite, float beta1, float beta2, void* partials,
                  wn_guard_state* state, wn_stream_t stream) {
    WN_REQUIRE("wn_grad_guard", partials, state);
    if (n > 0) WN_REQUIRE("wn_grad_guard", g);
    if (n < 0) return wn_set_error_msg(-4, "wn_grad_guard: n is negative");
    if (((uintptr_t)g & 3) || ((uintptr_t)partials & 7) || ((uintptr_t)state & 7))
        return wn_set_error_msg(-4, "wn_grad_guard: g needs 4-byte, partials and state 8-byte alignment");
    return wn_launch_grad_guard(g, n, gscale, max_norm, skip_nonfinite, beta1, beta2, partials, state, (hipStream_t)stream);
}
int wn_adam_flat_guarded(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                         float gscale, const wn_guard_state* state, wn_stream_t stream) {
    if (n > 0) WN_REQUIRE("wn_adam_flat_guarded", p, g, m, v, state);
    return wn_launch_adam_guarded(p, g, m, v, n, lr, beta1, beta2, eps, gscale, state, (hipStream_t)stream);
}
int wn_sgd_flat_guarded(float* p, const float* g, float* momentum_buf, int64_t n, float lr, float momentum, float gscale,
                        const wn_guard_state* state, wn_stream_t stream) {
    if (momentum != 0.f && !momentum_buf) return wn_set_error_msg(-4, "wn_sgd_flat_guarded: momentum needs its buffer");
    if (n > 0) WN_REQUIRE("wn_sgd_flat_guarded", p, g, state);
    return wn_launch_sgd_guarded(p, g, momentum_buf, n, lr, momentum, gscale, state, (hipStream_t)stream);
}
int wn_rmsprop_flat_guarded(float* p, const float* g, float* square_avg, float* momentum_buf, int64_t n, float lr, float alpha, float eps,
                            float momentum, float gscale, const wn_guard_state* state, wn_stream_t stream) {
    if (!square_avg || (momentum > 0.f && !momentum_buf)) return wn_set_error_msg(-4, "wn_rmsprop_flat_guarded: missing state buffer");
    if (n > 0) WN_REQUIRE("wn_rmsprop_flat_guarded", p, g, state);
    return wn_launch_rmsprop_guarded(p, g, square_avg, momentum_buf, n, lr, alpha, eps, momentum, gscale, state, (hipStream_t)stream);
}
// ---- EMA shadow of the parameters (wn_guard.hip) ----
int wn_ema_flat(float* ema, const float* p, int64_t n, float decay, int warmup, int64_t t, const wn_guard_state* state,
                wn_stream_t stream) {
    if (n < 0) return wn_set_error_msg(-4, "wn_ema_flat: n is negative");
    if (n == 0) return 0;
    WN_REQUIRE("wn_ema_flat", ema, p);
    if ((uintptr_t)ema % 4 != 0) return wn_set_error_msg(-4, "wn_ema_flat: argument 'ema' needs 4-byte alignment");
    if ((uintptr_t)p % 4 != 0) return wn_set_error_msg(-4, "wn_ema_flat: argument 'p' needs 4-byte alignment");
    if ((uintptr_t)state % 8 != 0) return wn_set_error_msg(-4, "wn_ema_flat: argument 'state' needs 8-byte alignment");
    if (!(decay >= 0.f && decay < 1.f)) return wn_set_error_msg(-4, "wn_ema_flat: argument 'decay' must lie in [0, 1)");
    if (!state && t < 1) return wn_set_error_msg(-4, "wn_ema_flat: argument 't' counts the updates from 1 when state is NULL");
    return wn_launch_ema(ema, p, n, decay, warmup ? 1 : 0, t, state, (hipStream_t)stream);
}
// ---- per-timestep softmax and negative log-likelihood (wn_nll.hip) ----
// the refusals both entries share: shapes first (they need no pointer), then the pointers of a call that has work to do
static int step_checked(const char* fn, const void* x, int64_t x_bstride, int x_pitch, int w, int q, int batch) {
    char msg[160];
    const char* bad = nullptr;
    if (batch < 0) bad = "'batch' must be >= 0";
    else if (w < 0) bad = "'w' must be >= 0";
    else if (q < 1 || q > 1024) bad = "'q' must lie in [1, 1024]";
    else if (x_pitch < w) bad = "'x_pitch' must be >= w";
    else if (x_bstride < (int64_t)q * x_pitch) bad = "'x_bstride' must be >= q * x_pitch";
    if (bad) {
        snprintf(msg, sizeof(msg), "%s: argument %s", fn, bad);
        return wn_set_error_msg(-4, msg);
    }
    if (batch > 0 && w > 0) WN_REQUIRE(fn, x);
    return 0;
}
int wn_step_softmax(const float* x, int64_t x_bstride, int x_pitch, float* probs, int w, int q, int batch, wn_stream_t stream) {
    if (int rc = step_checked("wn_step_softmax", x, x_bstride, x_pitch, w, q, batch)) return rc;
    if (batch == 0 || w == 0) return 0;
    WN_REQUIRE("wn_step_softmax", probs);
    return wn_launch_step_nll(x, (long)x_bstride, x_pitch, nullptr, nullptr, 0, 0, probs, nullptr, nullptr, nullptr, w, q, batch, 0.f,
                              nullptr, nullptr, (hipStream_t)stream);
}
// wn_step_nll's refusals and launch under the entry's name `fn`; win NULL: no windows; wt NULL: no weights (else inv_n is unused)
static int step_nll_checked(const char* fn, const float* x, int64_t x_bstride, int x_pitch, const int64_t* target, float* dx,
                            int64_t dx_bstride, int dx_pitch, float* probs, float* row_nll, int32_t* row_hit, float* loss_part, int w,
                            int q, int batch, float inv_n, const WnNllWin* win, const WnNllWt* wt, wn_stream_t stream) {
    char msg[160];
    if (dx && dx_pitch < w) {
        snprintf(msg, sizeof(msg), "%s: argument 'dx_pitch' must be >= w", fn);
        return wn_set_error_msg(-4, msg);
    }
    if (dx && dx_bstride < (int64_t)q * dx_pitch) {
        snprintf(msg, sizeof(msg), "%s: argument 'dx_bstride' must be >= q * dx_pitch", fn);
        return wn_set_error_msg(-4, msg);
    }
    if (batch > 0 && w > 0) WN_REQUIRE(fn, target, loss_part);
    return wn_launch_step_nll(x, (long)x_bstride, x_pitch, target, dx, (long)dx_bstride, dx_pitch, probs, row_nll, row_hit, loss_part, w, q,
                              batch, inv_n, win, wt, (hipStream_t)stream);
}
int wn_step_nll(const float* x, int64_t x_bstride, int x_pitch, const int64_t* target, float* dx, int64_t dx_bstride, int dx_pitch,
                float* probs, float* row_nll, int32_t* row_hit, float* loss_part, int w, int q, int batch, float inv_n,
                wn_stream_t stream) {
    if (int rc = step_checked("wn_step_nll", x, x_bstride, x_pitch, w, q, batch)) return rc;
    return step_nll_checked("wn_step_nll", x, x_bstride, x_pitch, target, dx, dx_bstride, dx_pitch, probs, row_nll, row_hit, loss_part, w,
                            q, batch, inv_n, nullptr, nullptr, stream);
}
// the objective's window table (the samplers' checks, win_checked) in its kernel-argument form; q is in range here
static int nll_win_checked(const char* fn, const int32_t* win_host, int win_period, const int64_t* win_pos, int64_t win_pos0, int q,
                           WnNllWin& win) {
    memset(&win, 0, sizeof(win));
    int pos0 = 0;
    if (int rc = win_checked(fn, win_host, win_period, win_pos0, q, win.period, pos0, win.lo, win.hi)) return rc;
    win.pos0 = (unsigned)pos0;
    win.pow32 = win_period > 0 ? (unsigned)((1ull << 32) % (unsigned)win_period) : 0;
    win.pos = win_pos;
    return 0;
}
int wn_win_step_softmax(const float* x, int64_t x_bstride, int x_pitch, float* probs, int w, int q, int batch, const int32_t* win_host,
                        int win_period, const int64_t* win_pos, int64_t win_pos0, wn_stream_t stream) {
    const char* fn = "wn_win_step_softmax";
    if (int rc = step_checked(fn, x, x_bstride, x_pitch, w, q, batch)) return rc;
    WnNllWin win;
    if (int rc = nll_win_checked(fn, win_host, win_period, win_pos, win_pos0, q, win)) return rc;
    if (batch == 0 || w == 0) return 0;
    WN_REQUIRE(fn, probs);
    return wn_launch_step_nll(x, (long)x_bstride, x_pitch, nullptr, nullptr, 0, 0, probs, nullptr, nullptr, nullptr, w, q, batch, 0.f,
                              &win, nullptr, (hipStream_t)stream);
}
int wn_win_step_nll(const float* x, int64_t x_bstride, int x_pitch, const int64_t* target, float* dx, int64_t dx_bstride, int dx_pitch,
                    float* probs, float* row_nll, int32_t* row_hit, float* loss_part, int w, int q, int batch, float inv_n,
                    const int32_t* win_host, int win_period, const int64_t* win_pos, int64_t win_pos0, wn_stream_t stream) {
    const char* fn = "wn_win_step_nll";
    if (int rc = step_checked(fn, x, x_bstride, x_pitch, w, q, batch)) return rc;
    WnNllWin win;
    if (int rc = nll_win_checked(fn, win_host, win_period, win_pos, win_pos0, q, win)) return rc;
    return step_nll_checked(fn, x, x_bstride, x_pitch, target, dx, dx_bstride, dx_pitch, probs, row_nll, row_hit, loss_part, w, q, batch,
                            inv_n, &win, nullptr, stream);
}
int wn_wstep_nll(const float* x, int64_t x_bstride, int x_pitch, const int64_t* target, float* dx, int64_t dx_bstride, int dx_pitch,
                 float* probs, float* row_nll, int32_t* row_hit, float* loss_part, int w, int q, int batch, const int32_t* win_host,
                 int win_period, const int64_t* win_pos, int64_t win_pos0, const float* weight, int64_t ignore_index, float smoothing,
                 float* den, wn_stream_t stream) {
    const char* fn = "wn_wstep_nll";
    if (int rc = step_checked(fn, x, x_bstride, x_pitch, w, q, batch)) return rc;
    WnNllWin win;
    if (int rc = nll_win_checked(fn, win_host, win_period, win_pos, win_pos0, q, win)) return rc;
    if (!(smoothing >= 0.f && smoothing < 1.f)) return wn_set_error_msg(-4, "wn_wstep_nll: argument 'smoothing' must lie in [0, 1)");
    if (batch > 0 && w > 0) WN_REQUIRE(fn, den);
    const WnNllWt wt = {weight, ignore_index, smoothing, den};
    return step_nll_checked(fn, x, x_bstride, x_pitch, target, dx, dx_bstride, dx_pitch, probs, row_nll, row_hit, loss_part, w, q, batch,
                            0.f, &win, &wt, stream);
}
// ---- learned conditioning projections (wn_condproj.hip) ----
// the refusals both entries share: shapes, offsets and strides first (they need no pointer)
static int cond_proj_checked(const char* fn, int64_t w_off, int64_t b_off, int64_t stage_stride, int64_t wf_off, int64_t bf_off, int pair,
                             int n_stages, int dd, int ch, int sd, int bw, int le, int batch) {
    char msg[200];
    const char* bad = nullptr;
    if (batch < 0) bad = "'batch' must be >= 0";
    else if (n_stages < 1) bad = "'n_stages' must be >= 1";
    else if (dd < 1) bad = "'dd' must be >= 1";
    else if (sd < 1) bad = "'sd' must be >= 1";
    else if (bw < 1) bad = "'bw' must be >= 1";
    else if (le < 1) bad = "'le' must be >= 1";
    else if (ch < dd || ch % 32 != 0) bad = "'ch' must be a multiple of 32 and >= dd";
    else if (w_off < 0) bad = "'w_off' must be >= 0";
    else if (b_off < 0) bad = "'b_off' must be >= 0";
    else if (wf_off < 0) bad = "'wf_off' must be >= 0";
    else if (bf_off < 0) bad = "'bf_off' must be >= 0";
    else if (n_stages > 1 && stage_stride < (int64_t)2 * dd * bw) bad = "'stage_stride' must be >= 2 * dd * bw (the stages' weights overlap)";
    else if (pair && batch % 2 != 0) bad = "'batch' must be even for a table of clip pairs";
    if (bad) {
        snprintf(msg, sizeof(msg), "%s: argument %s", fn, bad);
        return wn_set_error_msg(-4, msg);
    }
    return 0;
}
int wn_cond_proj_fwd(const float* enc, const float* flat, int64_t w_off, int64_t b_off, int64_t stage_stride, int64_t wf_off,
                     int64_t bf_off, float* tab, float* tab_pair, float* enf, int n_stages, int dd, int ch, int sd, int bw, int le,
                     int batch, wn_stream_t stream) {
    if (int rc = cond_proj_checked("wn_cond_proj_fwd", w_off, b_off, stage_stride, wf_off, bf_off, tab_pair != nullptr, n_stages, dd, ch,
                                   sd, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_cond_proj_fwd", enc, flat, enf);
    if (!tab && !tab_pair) return wn_set_error_msg(-4, "wn_cond_proj_fwd: argument 'tab' or 'tab_pair' must not be NULL");
    WnCondProj p;
    memset(&p, 0, sizeof(p));
    p.enc = enc; p.flat = flat; p.w_off = (long)w_off; p.b_off = (long)b_off; p.stage_stride = (long)stage_stride;
    p.wf_off = (long)wf_off; p.bf_off = (long)bf_off; p.tab = tab; p.tab_pair = tab_pair; p.enf = enf;
    p.n_stages = n_stages; p.dd = dd; p.ch = ch; p.sd = sd; p.bw = bw; p.le = le; p.batch = batch;
    return wn_launch_cond_proj_fwd(p, (hipStream_t)stream);
}
int wn_cond_proj_bwd(const float* d_tab, int pair, const float* d_enf, const float* enc, const float* flat, int64_t w_off,
                     int64_t b_off, int64_t stage_stride, int64_t wf_off, int64_t bf_off, float* d_enc, float* flat_grad,
                     int n_stages, int dd, int ch, int sd, int bw, int le, int batch, wn_stream_t stream) {
    if (int rc = cond_proj_checked("wn_cond_proj_bwd", w_off, b_off, stage_stride, wf_off, bf_off, pair, n_stages, dd, ch, sd, bw, le,
                                   batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_cond_proj_bwd", d_tab, d_enf, enc, flat, d_enc, flat_grad);
    WnCondProj p;
    memset(&p, 0, sizeof(p));
    p.enc = enc; p.flat = flat; p.w_off = (long)w_off; p.b_off = (long)b_off; p.stage_stride = (long)stage_stride;
    p.wf_off = (long)wf_off; p.bf_off = (long)bf_off; p.d_tab = d_tab; p.d_pair = pair ? 1 : 0; p.d_enf = d_enf; p.d_enc = d_enc;
    p.flat_grad = flat_grad;
    p.n_stages = n_stages; p.dd = dd; p.ch = ch; p.sd = sd; p.bw = bw; p.le = le; p.batch = batch;
    return wn_launch_cond_proj_bwd(p, (hipStream_t)stream);
}
// ---- learned conditioning projections with a global class term (wn_gcond.hip) ----
static_assert(WN_GCOND_MAX_E == WN_GCOND_MAX_CHANNELS, "wn_kernels.h and wavenet_hip.h disagree");
// the refusals of cond_proj_checked, then the new arguments' (they need no pointer either)
static int gcond_checked(const char* fn, int64_t w_off, int64_t b_off, int64_t stage_stride, int64_t wf_off, int64_t bf_off, int pair,
                         int n_stages, int dd, int ch, int sd, int bw, int le, int batch, int64_t gw_off, int64_t gstage_stride,
                         int64_t gwf_off, int64_t emb_off, int ge, int n_cls) {
    if (int rc = cond_proj_checked(fn, w_off, b_off, stage_stride, wf_off, bf_off, pair, n_stages, dd, ch, sd, bw, le, batch)) return rc;
    char msg[200];
    const char* bad = nullptr;
    if (ge < 1 || ge > WN_GCOND_MAX_CHANNELS) bad = "'ge' must lie in [1, 512]";
    else if (n_cls < 1) bad = "'n_cls' must be >= 1";
    else if (gw_off < 0) bad = "'gw_off' must be >= 0";
    else if (gwf_off < 0) bad = "'gwf_off' must be >= 0";
    else if (emb_off < 0) bad = "'emb_off' must be >= 0";
    else if (n_stages > 1 && gstage_stride < (int64_t)2 * dd * ge) bad = "'gstage_stride' must be >= 2 * dd * ge (the stages' weights overlap)";
    if (bad) {
        snprintf(msg, sizeof(msg), "%s: argument %s", fn, bad);
        return wn_set_error_msg(-4, msg);
    }
    return 0;
}
static WnGcond gcond_args(const int32_t* cls, int64_t gw_off, int64_t gstage_stride, int64_t gwf_off, int64_t emb_off, int ge, int n_cls) {
    WnGcond g;
    g.cls = cls; g.gw_off = (long)gw_off; g.gstage_stride = (long)gstage_stride; g.gwf_off = (long)gwf_off; g.emb_off = (long)emb_off;
    g.ge = ge; g.n_cls = n_cls;
    return g;
}
int wn_gcond_proj_fwd(const float* enc, const float* flat, int64_t w_off, int64_t b_off, int64_t stage_stride, int64_t wf_off,
                      int64_t bf_off, float* tab, float* tab_pair, float* enf, int n_stages, int dd, int ch, int sd, int bw, int le,
                      int batch, const int32_t* cls, int64_t gw_off, int64_t gstage_stride, int64_t gwf_off, int64_t emb_off, int ge,
                      int n_cls, wn_stream_t stream) {
    if (int rc = gcond_checked("wn_gcond_proj_fwd", w_off, b_off, stage_stride, wf_off, bf_off, tab_pair != nullptr, n_stages, dd, ch, sd,
                               bw, le, batch, gw_off, gstage_stride, gwf_off, emb_off, ge, n_cls)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_gcond_proj_fwd", enc, flat, enf, cls);
    if (!tab && !tab_pair) return wn_set_error_msg(-4, "wn_gcond_proj_fwd: argument 'tab' or 'tab_pair' must not be NULL");
    WnCondProj p;
    memset(&p, 0, sizeof(p));
    p.enc = enc; p.flat = flat; p.w_off = (long)w_off; p.b_off = (long)b_off; p.stage_stride = (long)stage_stride;
    p.wf_off = (long)wf_off; p.bf_off = (long)bf_off; p.tab = tab; p.tab_pair = tab_pair; p.enf = enf;
    p.n_stages = n_stages; p.dd = dd; p.ch = ch; p.sd = sd; p.bw = bw; p.le = le; p.batch = batch;
    return wn_launch_gcond_proj_fwd(p, gcond_args(cls, gw_off, gstage_stride, gwf_off, emb_off, ge, n_cls), (hipStream_t)stream);
}
int wn_gcond_proj_bwd(const float* d_tab, int pair, const float* d_enf, const float* enc, const float* flat, int64_t w_off,
                      int64_t b_off, int64_t stage_stride, int64_t wf_off, int64_t bf_off, float* d_enc, float* flat_grad,
                      int n_stages, int dd, int ch, int sd, int bw, int le, int batch, const int32_t* cls, int64_t gw_off,
                      int64_t gstage_stride, int64_t gwf_off, int64_t emb_off, int ge, int n_cls, wn_stream_t stream) {
    if (int rc = gcond_checked("wn_gcond_proj_bwd", w_off, b_off, stage_stride, wf_off, bf_off, pair, n_stages, dd, ch, sd, bw, le, batch,
                               gw_off, gstage_stride, gwf_off, emb_off, ge, n_cls)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_gcond_proj_bwd", d_tab, d_enf, enc, flat, d_enc, flat_grad, cls);
    WnCondProj p;
    memset(&p, 0, sizeof(p));
    p.enc = enc; p.flat = flat; p.w_off = (long)w_off; p.b_off = (long)b_off; p.stage_stride = (long)stage_stride;
    p.wf_off = (long)wf_off; p.bf_off = (long)bf_off; p.d_tab = d_tab; p.d_pair = pair ? 1 : 0; p.d_enf = d_enf; p.d_enc = d_enc;
    p.flat_grad = flat_grad;
    p.n_stages = n_stages; p.dd = dd; p.ch = ch; p.sd = sd; p.bw = bw; p.le = le; p.batch = batch;
    return wn_launch_gcond_proj_bwd(p, gcond_args(cls, gw_off, gstage_stride, gwf_off, emb_off, ge, n_cls), (hipStream_t)stream);
}
// ---- the global class term alone (wn_gcond.hip): the tables of a class-conditional WaveNet ----
// wn_gcond_proj_*'s refusals that still apply (no bw, no le, no learned offsets); they need no pointer
static int gclass_checked(const char* fn, int pair, int n_stages, int dd, int ch, int sd, int batch, int64_t gw_off, int64_t gstage_stride,
                          int64_t gwf_off, int64_t emb_off, int ge, int n_cls) {
    char msg[200];
    const char* bad = nullptr;
    if (batch < 0) bad = "'batch' must be >= 0";
    else if (n_stages < 1) bad = "'n_stages' must be >= 1";
    else if (dd < 1) bad = "'dd' must be >= 1";
    else if (sd < 1) bad = "'sd' must be >= 1";
    else if (ch < dd || ch % 32 != 0) bad = "'ch' must be a multiple of 32 and >= dd";
    else if (pair && batch % 2 != 0) bad = "'batch' must be even for a table of clip pairs";
    else if (ge < 1 || ge > WN_GCOND_MAX_CHANNELS) bad = "'ge' must lie in [1, 512]";
    else if (n_cls < 1) bad = "'n_cls' must be >= 1";
    else if (gw_off < 0) bad = "'gw_off' must be >= 0";
    else if (gwf_off < 0) bad = "'gwf_off' must be >= 0";
    else if (emb_off < 0) bad = "'emb_off' must be >= 0";
    else if (n_stages > 1 && gstage_stride < (int64_t)2 * dd * ge) bad = "'gstage_stride' must be >= 2 * dd * ge (the stages' weights overlap)";
    if (bad) {
        snprintf(msg, sizeof(msg), "%s: argument %s", fn, bad);
        return wn_set_error_msg(-4, msg);
    }
    return 0;
}
int wn_gclass_fwd(const float* flat, float* tab, float* tab_pair, float* enf, int n_stages, int dd, int ch, int sd, int batch,
                  const int32_t* cls, int64_t gw_off, int64_t gstage_stride, int64_t gwf_off, int64_t emb_off, int ge, int n_cls,
                  wn_stream_t stream) {
    if (int rc = gclass_checked("wn_gclass_fwd", tab_pair != nullptr, n_stages, dd, ch, sd, batch, gw_off, gstage_stride, gwf_off, emb_off,
                                ge, n_cls)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_gclass_fwd", flat, enf, cls);
    if (!tab && !tab_pair) return wn_set_error_msg(-4, "wn_gclass_fwd: argument 'tab' or 'tab_pair' must not be NULL");
    WnCondProj p;
    memset(&p, 0, sizeof(p));
    p.flat = flat; p.tab = tab; p.tab_pair = tab_pair; p.enf = enf;
    p.n_stages = n_stages; p.dd = dd; p.ch = ch; p.sd = sd; p.bw = 1; p.le = 1; p.batch = batch;
    return wn_launch_gclass_fwd(p, gcond_args(cls, gw_off, gstage_stride, gwf_off, emb_off, ge, n_cls), (hipStream_t)stream);
}
int wn_gclass_bwd(const float* d_tab, int pair, const float* d_enf, const float* flat, float* flat_grad, int n_stages, int dd, int ch,
                  int sd, int batch, const int32_t* cls, int64_t gw_off, int64_t gstage_stride, int64_t gwf_off, int64_t emb_off, int ge,
                  int n_cls, wn_stream_t stream) {
    if (int rc = gclass_checked("wn_gclass_bwd", pair, n_stages, dd, ch, sd, batch, gw_off, gstage_stride, gwf_off, emb_off, ge, n_cls))
        return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_gclass_bwd", d_tab, d_enf, flat, flat_grad, cls);
    WnCondProj p;
    memset(&p, 0, sizeof(p));
    p.flat = flat; p.d_tab = d_tab; p.d_pair = pair ? 1 : 0; p.d_enf = d_enf; p.flat_grad = flat_grad;
    p.n_stages = n_stages; p.dd = dd; p.ch = ch; p.sd = sd; p.bw = 1; p.le = 1; p.batch = batch;
    return wn_launch_gclass_bwd(p, gcond_args(cls, gw_off, gstage_stride, gwf_off, emb_off, ge, n_cls), (hipStream_t)stream);
}
// ---- the tables of a phase-conditioned WaveNet (wn_phase.hip) ----
// the refusals both entries share: shapes, offsets and the stride (they need no pointer)
static int phase_checked(const char* fn, int pair, int n_stages, int dd, int ch, int sd, int period, int batch, int64_t pw_off,
                         int64_t pstage_stride, int64_t pwf_off) {
    char msg[200];
    const char* bad = nullptr;
    if (batch < 0) bad = "'batch' must be >= 0";
    else if (n_stages < 1) bad = "'n_stages' must be >= 1";
    else if (dd < 1) bad = "'dd' must be >= 1";
    else if (sd < 1) bad = "'sd' must be >= 1";
    else if (period < 1 || period > WN_PHASE_MAX_PERIOD) bad = "'period' must lie in [1, 16]";
    else if (ch < dd || ch % 32 != 0) bad = "'ch' must be a multiple of 32 and >= dd";
    else if (pair && batch % 2 != 0) bad = "'batch' must be even for a table of clip pairs";
    else if (pw_off < 0) bad = "'pw_off' must be >= 0";
    else if (pwf_off < 0) bad = "'pwf_off' must be >= 0";
    else if (n_stages > 1 && pstage_stride < (int64_t)2 * dd * period) bad = "'pstage_stride' must be >= 2 * dd * period (the stages' tables overlap)";
    if (bad) {
        snprintf(msg, sizeof(msg), "%s: argument %s", fn, bad);
        return wn_set_error_msg(-4, msg);
    }
    return 0;
}
static WnPhase phase_args(int64_t pw_off, int64_t pstage_stride, int64_t pwf_off, const int64_t* pos, const int32_t* rot, int n_stages,
                          int dd, int ch, int sd, int period, int batch) {
    WnPhase p;
    memset(&p, 0, sizeof(p));
    p.pw_off = (long)pw_off; p.pstage_stride = (long)pstage_stride; p.pwf_off = (long)pwf_off; p.pos = pos; p.rot = rot;
    p.n_stages = n_stages; p.dd = dd; p.ch = ch; p.sd = sd; p.period = period; p.batch = batch;
    return p;
}
int wn_phase_tab_fwd(const float* flat, int64_t pw_off, int64_t pstage_stride, int64_t pwf_off, const int64_t* pos, const int32_t* rot,
                     const float* add_tab, const float* add_pair, const float* add_enf, float* tab, float* tab_pair, float* enf,
                     int n_stages, int dd, int ch, int sd, int period, int batch, wn_stream_t stream) {
    const char* fn = "wn_phase_tab_fwd";
    if (int rc = phase_checked(fn, tab_pair != nullptr, n_stages, dd, ch, sd, period, batch, pw_off, pstage_stride, pwf_off)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_phase_tab_fwd", flat, pos, rot, enf);
    if (!tab && !tab_pair) return wn_set_error_msg(-4, "wn_phase_tab_fwd: argument 'tab' or 'tab_pair' must not be NULL");
    if (add_tab || add_pair || add_enf) {                    // the class term: an addend for every output
        if (!add_enf) return wn_set_error_msg(-4, "wn_phase_tab_fwd: argument 'add_enf' must not be NULL where an addend is given");
        if (tab && !add_tab) return wn_set_error_msg(-4, "wn_phase_tab_fwd: argument 'add_tab' must not be NULL where 'tab' and an addend are given");
        if (tab_pair && !add_pair)
            return wn_set_error_msg(-4, "wn_phase_tab_fwd: argument 'add_pair' must not be NULL where 'tab_pair' and an addend are given");
    }
    WnPhase p = phase_args(pw_off, pstage_stride, pwf_off, pos, rot, n_stages, dd, ch, sd, period, batch);
    p.flat = flat; p.add_tab = add_tab; p.add_pair = add_pair; p.add_enf = add_enf; p.tab = tab; p.tab_pair = tab_pair; p.enf = enf;
    return wn_launch_phase_tab_fwd(p, (hipStream_t)stream);
}
int wn_phase_tab_bwd(const float* d_tab, int pair, const float* d_enf, float* flat_grad, int64_t pw_off, int64_t pstage_stride,
                     int64_t pwf_off, const int64_t* pos, const int32_t* rot, float* sum_tab, float* sum_enf, int n_stages, int dd, int ch,
                     int sd, int period, int batch, wn_stream_t stream) {
    const char* fn = "wn_phase_tab_bwd";
    if (int rc = phase_checked(fn, pair, n_stages, dd, ch, sd, period, batch, pw_off, pstage_stride, pwf_off)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_phase_tab_bwd", d_tab, d_enf, flat_grad, pos, rot);
    if ((sum_tab != nullptr) != (sum_enf != nullptr))
        return wn_set_error_msg(-4, "wn_phase_tab_bwd: arguments 'sum_tab' and 'sum_enf' must both be NULL or both be given");
    WnPhase p = phase_args(pw_off, pstage_stride, pwf_off, pos, rot, n_stages, dd, ch, sd, period, batch);
    p.d_tab = d_tab; p.d_pair = pair ? 1 : 0; p.d_enf = d_enf; p.flat_grad = flat_grad; p.sum_tab = sum_tab; p.sum_enf = sum_enf;
    return wn_launch_phase_tab_bwd(p, (hipStream_t)stream);
}
// ---- vector-quantised bottleneck (wn_vq.hip) ----
static int vq_refused(const char* fn, const char* what) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: argument %s", fn, what);
    return wn_set_error_msg(-4, msg);
}
// the refusals the entries share: shapes and the offset first (they need no pointer)
static int vq_checked(const char* fn, int64_t cb_off, int K, int bw, int le, int batch) {
    const char* bad = nullptr;
    if (batch < 0) bad = "'batch' must be >= 0";
    else if (K < 2 || K > WN_VQ_MAX_CODES) bad = "'K' must lie in [2, 1024]";
    else if (bw < 1 || bw > WN_VQ_MAX_WIDTH) bad = "'bw' must lie in [1, 512]";
    else if (le < 1) bad = "'le' must be >= 1";
    else if (cb_off < 0) bad = "'cb_off' must be >= 0";
    else if ((int64_t)batch * le > 0x7fffffffLL - 64) bad = "'batch' * le frames do not fit 31 bits";
    return bad ? vq_refused(fn, bad) : 0;
}
// the residual chain over S codebooks (wn_rvq_*): the stage count, then the refusals above
static int rvq_checked(const char* fn, int S, int64_t cb_off, int K, int bw, int le, int batch) {
    if (S < 1 || S > WN_RVQ_MAX_STAGES) return vq_refused(fn, "'S' must lie in [1, 8]");
    return vq_checked(fn, cb_off, K, bw, le, batch);
}
// What every forward and backward entry hands its launcher.  res NULL: one stage (wn_vq_*; S is not read); else the chain over S stages,
// wn_rvq_* at S = 1 included.  nstage NULL: no stage counts
static WnVq rvq_args(const float* enc, const float* flat, int64_t cb_off, const int32_t* idx, const float* res, const int32_t* nstage, int S,
                     int K, int bw, int le, int batch) {
    WnVq p;
    memset(&p, 0, sizeof(p));
    p.enc = enc; p.flat = flat; p.cb_off = (long)cb_off; p.idx = const_cast<int32_t*>(idx); p.res = const_cast<float*>(res);
    p.nstage = nstage; p.S = S; p.K = K; p.bw = bw; p.le = le; p.batch = batch;
    return p;
}
static int vq_fwd_run(WnVq p, float* q_out, int32_t* counts, float* loss_part, wn_stream_t stream) {
    p.q_out = q_out; p.counts = counts; p.loss_part = loss_part;
    return wn_launch_vq_fwd(p, (hipStream_t)stream);
}
static int vq_bwd_run(WnVq p, const float* d_q, float beta, float g_scale, float* d_enc, float* flat_grad, float* stat, wn_stream_t stream) {
    p.d_q = d_q; p.d_enc = d_enc; p.flat_grad = flat_grad;
    return wn_launch_vq_bwd(p, beta, g_scale, stat, (hipStream_t)stream);
}
// wn_vq_ema_update (S = 1) and wn_rvq_ema_update
static int vq_ema_update_run(const char* fn, float* flat, int64_t cb_off, const float* stat, float* state, void* work, int32_t* info, int S,
                             int K, int bw, float decay, float eps, float restart, const wn_guard_state* guard_state, wn_stream_t stream) {
    if (int rc = rvq_checked(fn, S, cb_off, K, bw, 1, 1)) return rc;
    if (!(decay > 0.f && decay < 1.f)) return vq_refused(fn, "'decay' must lie in (0, 1)");
    if (!(eps >= 0.f)) return vq_refused(fn, "'eps' must be >= 0");
    if (!(restart >= 0.f)) return vq_refused(fn, "'restart' must be >= 0");
    WN_REQUIRE(fn, flat, stat, state, work);
    if ((uintptr_t)guard_state % 8 != 0) return vq_refused(fn, "'guard_state' needs 8-byte alignment");
    return wn_launch_vq_ema_update(flat, (long)cb_off, stat, state, work, info, S, K, bw, decay, eps, restart, guard_state,
                                   (hipStream_t)stream);
}

int wn_vq_fwd(const float* enc, const float* flat, int64_t cb_off, float* q_out, int32_t* idx, int32_t* counts, float* loss_part, int K,
              int bw, int le, int batch, wn_stream_t stream) {
    if (int rc = vq_checked("wn_vq_fwd", cb_off, K, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_vq_fwd", enc, flat, q_out, idx, loss_part);
    return vq_fwd_run(rvq_args(enc, flat, cb_off, idx, nullptr, nullptr, 1, K, bw, le, batch), q_out, counts, loss_part, stream);
}
int wn_vq_bwd(const float* enc, const int32_t* idx, const float* d_q, const float* flat, int64_t cb_off, float beta, float g_scale,
              float* d_enc, float* flat_grad, int K, int bw, int le, int batch, wn_stream_t stream) {
    if (int rc = vq_checked("wn_vq_bwd", cb_off, K, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_vq_bwd", enc, idx, d_q, flat, d_enc, flat_grad);
    return vq_bwd_run(rvq_args(enc, flat, cb_off, idx, nullptr, nullptr, 1, K, bw, le, batch), d_q, beta, g_scale, d_enc, flat_grad, nullptr,
                      stream);
}
int wn_vq_lookup(const int32_t* idx, const float* flat, int64_t cb_off, float* q_out, int32_t* bad, int K, int bw, int le, int batch,
                 wn_stream_t stream) {
    if (int rc = vq_checked("wn_vq_lookup", cb_off, K, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_vq_lookup", idx, flat, q_out);
    return wn_launch_vq_lookup(idx, nullptr, flat, (long)cb_off, q_out, bad, 1, K, bw, le, batch, (hipStream_t)stream);
}
int wn_vq_bwd_stats(const float* enc, const int32_t* idx, const float* d_q, const float* flat, int64_t cb_off, float beta, float g_scale,
                    float* d_enc, float* flat_grad, float* stat, int K, int bw, int le, int batch, wn_stream_t stream) {
    if (int rc = vq_checked("wn_vq_bwd_stats", cb_off, K, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_vq_bwd_stats", enc, idx, d_q, flat, d_enc, flat_grad, stat);
    return vq_bwd_run(rvq_args(enc, flat, cb_off, idx, nullptr, nullptr, 1, K, bw, le, batch), d_q, beta, g_scale, d_enc, flat_grad, stat,
                      stream);
}
int wn_vq_ema_update(float* flat, int64_t cb_off, const float* stat, float* state, void* work, int32_t* info, int K, int bw,
                     float decay, float eps, float restart, const wn_guard_state* guard_state, wn_stream_t stream) {
    return vq_ema_update_run("wn_vq_ema_update", flat, cb_off, stat, state, work, info, 1, K, bw, decay, eps, restart, guard_state, stream);
}
// ---- the residual chain over S codebooks
int wn_rvq_fwd(const float* enc, const float* flat, int64_t cb_off, float* q_out, int32_t* idx, int32_t* counts, float* res,
               float* loss_part, int S, int K, int bw, int le, int batch, wn_stream_t stream) {
    if (int rc = rvq_checked("wn_rvq_fwd", S, cb_off, K, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_rvq_fwd", enc, flat, q_out, idx, res, loss_part);
    return vq_fwd_run(rvq_args(enc, flat, cb_off, idx, res, nullptr, S, K, bw, le, batch), q_out, counts, loss_part, stream);
}
int wn_rvq_bwd(const float* enc, const int32_t* idx, const float* res, const float* d_q, const float* flat, int64_t cb_off, float beta,
               float g_scale, float* d_enc, float* flat_grad, int S, int K, int bw, int le, int batch, wn_stream_t stream) {
    if (int rc = rvq_checked("wn_rvq_bwd", S, cb_off, K, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_rvq_bwd", enc, idx, res, d_q, flat, d_enc, flat_grad);
    return vq_bwd_run(rvq_args(enc, flat, cb_off, idx, res, nullptr, S, K, bw, le, batch), d_q, beta, g_scale, d_enc, flat_grad, nullptr,
                      stream);
}
int wn_rvq_bwd_stats(const float* enc, const int32_t* idx, const float* res, const float* d_q, const float* flat, int64_t cb_off, float beta,
                     float g_scale, float* d_enc, float* flat_grad, float* stat, int S, int K, int bw, int le, int batch,
                     wn_stream_t stream) {
    if (int rc = rvq_checked("wn_rvq_bwd_stats", S, cb_off, K, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_rvq_bwd_stats", enc, idx, res, d_q, flat, d_enc, flat_grad, stat);
    return vq_bwd_run(rvq_args(enc, flat, cb_off, idx, res, nullptr, S, K, bw, le, batch), d_q, beta, g_scale, d_enc, flat_grad, stat, stream);
}
int wn_rvq_ema_update(float* flat, int64_t cb_off, const float* stat, float* state, void* work, int32_t* info, int S, int K, int bw,
                      float decay, float eps, float restart, const wn_guard_state* guard_state, wn_stream_t stream) {
    return vq_ema_update_run("wn_rvq_ema_update", flat, cb_off, stat, state, work, info, S, K, bw, decay, eps, restart, guard_state, stream);
}
int wn_rvq_lookup(const int32_t* idx, const float* flat, int64_t cb_off, float* q_out, int32_t* bad, int S, int stages, int K, int bw, int le,
                  int batch, wn_stream_t stream) {
    if (int rc = rvq_checked("wn_rvq_lookup", S, cb_off, K, bw, le, batch)) return rc;
    if (stages < 1 || stages > S) return wn_set_error_msg(-4, "wn_rvq_lookup: argument 'stages' must lie in [1, S]");
    if (batch == 0) return 0;
    WN_REQUIRE("wn_rvq_lookup", idx, flat, q_out);
    return wn_launch_vq_lookup(idx, nullptr, flat, (long)cb_off, q_out, bad, stages, K, bw, le, batch, (hipStream_t)stream);
}
// ---- quantiser dropout: the chain with a stage count per clip (nstage, batch int32 on the device; required)
int wn_rvq_fwd_n(const float* enc, const float* flat, int64_t cb_off, const int32_t* nstage, float* q_out, int32_t* idx, int32_t* counts,
                 float* res, float* loss_part, int S, int K, int bw, int le, int batch, wn_stream_t stream) {
    if (int rc = rvq_checked("wn_rvq_fwd_n", S, cb_off, K, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_rvq_fwd_n", enc, flat, nstage, q_out, idx, res, loss_part);
    return vq_fwd_run(rvq_args(enc, flat, cb_off, idx, res, nstage, S, K, bw, le, batch), q_out, counts, loss_part, stream);
}
int wn_rvq_bwd_n(const float* enc, const int32_t* idx, const float* res, const int32_t* nstage, const float* d_q, const float* flat,
                 int64_t cb_off, float beta, float g_scale, float* d_enc, float* flat_grad, int S, int K, int bw, int le, int batch,
                 wn_stream_t stream) {
    if (int rc = rvq_checked("wn_rvq_bwd_n", S, cb_off, K, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_rvq_bwd_n", enc, idx, res, nstage, d_q, flat, d_enc, flat_grad);
    return vq_bwd_run(rvq_args(enc, flat, cb_off, idx, res, nstage, S, K, bw, le, batch), d_q, beta, g_scale, d_enc, flat_grad, nullptr, stream);
}
int wn_rvq_bwd_stats_n(const float* enc, const int32_t* idx, const float* res, const int32_t* nstage, const float* d_q, const float* flat,
                       int64_t cb_off, float beta, float g_scale, float* d_enc, float* flat_grad, float* stat, int S, int K, int bw, int le,
                       int batch, wn_stream_t stream) {
    if (int rc = rvq_checked("wn_rvq_bwd_stats_n", S, cb_off, K, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_rvq_bwd_stats_n", enc, idx, res, nstage, d_q, flat, d_enc, flat_grad, stat);
    return vq_bwd_run(rvq_args(enc, flat, cb_off, idx, res, nstage, S, K, bw, le, batch), d_q, beta, g_scale, d_enc, flat_grad, stat, stream);
}
int wn_rvq_lookup_n(const int32_t* idx, const int32_t* nstage, const float* flat, int64_t cb_off, float* q_out, int32_t* bad, int S, int K,
                    int bw, int le, int batch, wn_stream_t stream) {
    if (int rc = rvq_checked("wn_rvq_lookup_n", S, cb_off, K, bw, le, batch)) return rc;
    if (batch == 0) return 0;
    WN_REQUIRE("wn_rvq_lookup_n", idx, nstage, flat, q_out);
    return wn_launch_vq_lookup(idx, nstage, flat, (long)cb_off, q_out, bad, S, K, bw, le, batch, (hipStream_t)stream);
}
int wn_coll_available(void) { return wn_coll_loaded(); }
int wn_comm_unique_id(char* id128) { return wn_coll_unique_id(id128); }
int wn_comm_create(int nranks, int rank, const char* id128, void** comm) { return wn_coll_create(nranks, rank, id128, comm); }
int wn_comm_destroy(void* comm) { return wn_coll_destroy(comm); }
int wn_allreduce_flat(void* comm, float* buf, int64_t n, wn_stream_t stream) {
    return wn_coll_allreduce_flat(comm, buf, n, (hipStream_t)stream);
}
int wn_gather_grads(const float* packed, const int32_t* idx, float* flat_grad, int n, wn_stream_t stream) {
    if (n > 0) WN_REQUIRE("wn_gather_grads", packed, idx, flat_grad);
    return wn_launch_gather_grads(packed, idx, flat_grad, n, (hipStream_t)stream);
}
int wn_gather_grads2(const float* packed, const int32_t* idx, const int32_t* idx2, float* flat_grad, int n, wn_stream_t stream) {
    if (!packed || !idx || !idx2 || !flat_grad) return wn_set_error_msg(-4, "wn_gather_grads2: null argument");
    return wn_launch_gather_grads2(packed, idx, idx2, flat_grad, n, (hipStream_t)stream);
}
int wn_onehot(const int32_t* codes, float* out, int batch, int q, int t, int scrambled, wn_stream_t stream) {
    if (batch <= 0 || q <= 0 || t <= 0) return 0;                // no work: nothing is written, no pointer is required
    WN_REQUIRE("wn_onehot", codes, out);
    return wn_launch_onehot(codes, out, batch, q, t, scrambled, (hipStream_t)stream);
}
int wn_mulaw_encode_tbl(const float* audio, const float* thresholds, uint8_t* codes, int64_t n, wn_stream_t stream) {
    if (n > 0) WN_REQUIRE("wn_mulaw_encode_tbl", audio, thresholds, codes);
    return wn_launch_mulaw_encode(audio, thresholds, codes, n, (hipStream_t)stream);
}
int wn_mulaw_decode_lut(const uint8_t* codes, const float* table, float* audio, int64_t n, wn_stream_t stream) {
    if (n > 0) WN_REQUIRE("wn_mulaw_decode_lut", codes, table, audio);
    return wn_launch_mulaw_decode(codes, table, audio, n, (hipStream_t)stream);
}
int wn_mulaw_encode_q(const float* audio, const float* thresholds, int q, int32_t* codes, int64_t n, wn_stream_t stream) {
    if (q < 2 || (n > 0 && (!audio || !thresholds || !codes))) return wn_set_error_msg(-4, "wn_mulaw_encode_q: bad argument");
    return wn_launch_mulaw_encode_q(audio, thresholds, q - 1, codes, n, (hipStream_t)stream);
}
int wn_mulaw_decode_q(const int32_t* codes, const float* table, int q, float* audio, int64_t n, wn_stream_t stream) {
    if (q < 2 || (n > 0 && (!audio || !table || !codes))) return wn_set_error_msg(-4, "wn_mulaw_decode_q: bad argument");
    return wn_launch_mulaw_decode_q(codes, table, q, audio, n, (hipStream_t)stream);
}

int wn_resblock_bwd_ms(const float* x_in, const float* dy, const float* dz, float* dfg, int64_t x_bstride,
                       int64_t dz_bstride, int64_t dfg_bstride, int pitch, const uint16_t* wfg, const uint16_t* wdT,
                       const float* bias_f, const float* bias_g, int n_f, int ch, int d, int t_lo, int t_hi, int z_lo,
                       float* slab_fg, float* slab_d, const float* cond, int64_t cond_bstride, int cond_pitch,
                       int cond_mode, int cond_le, int cond_q, int batch, int mode_fwd, int mode_bwd,
                       wn_stream_t stream) {
    if (pitch % 4 != 0) return wn_set_error_msg(-4, "wn_resblock_bwd_ms: pitch must be a multiple of 4");
    if (cond && (cond_le <= 0 || (cond_mode == 1 && cond_q <= 0) || (cond_mode != 1 && cond_mode != 2)))
        return wn_set_error_msg(-4, "wn_resblock_bwd_ms: bad conditioning arguments");
    if (!slab_fg) return wn_set_error_msg(-4, "wn_resblock_bwd_ms: slab_fg is required");
    if (batch > 0 && t_hi > t_lo) {
        WN_REQUIRE("wn_resblock_bwd_ms", x_in, dz, dfg, wfg);
        if (dy) WN_REQUIRE("wn_resblock_bwd_ms", wdT, slab_d);
    }
    WnResMsArgs a;
    memset(&a, 0, sizeof(a));
    a.x_in = x_in; a.dy = dy; a.dz = dz; a.dfg = dfg; a.x_bstride = x_bstride; a.dz_bstride = dz_bstride;
    a.dfg_bstride = dfg_bstride; a.pitch = pitch; a.wfg = wfg; a.wdT = wdT; a.bias_f = bias_f; a.bias_g = bias_g; a.n_f = n_f;
    a.slab_fg = slab_fg; a.slab_d = dy ? slab_d : nullptr; a.d = d; a.t_lo = t_lo; a.t_hi = t_hi; a.z_lo = z_lo;
    a.cond = cond; a.cond_bstride = cond_bstride; a.cond_pitch = cond_pitch; a.cond_mode = cond_mode;
    a.cond_le = cond_le; a.cond_q = cond_q;
    return wn_launch_resblock_bwd_ms(a, ch, batch, mode_fwd, mode_bwd, (hipStream_t)stream);
}
int wn_enc_resblock_bwd(const float* x_in, const float* dy, const float* h, float* dh, int64_t x_bstride,
                        int64_t h_bstride, int64_t dh_bstride, int pitch, const uint16_t* wdT, int ch, int d, int t_lo,
                        int t_hi, int y_lo, float* slab_dil, float* slab_d, int batch, int mode_bwd, wn_stream_t stream) {
    if (pitch % 4 != 0) return wn_set_error_msg(-4, "wn_enc_resblock_bwd: pitch must be a multiple of 4");
    if (!x_in || !dy || !h || !dh || !wdT || !slab_dil || !slab_d) return wn_set_error_msg(-4, "wn_enc_resblock_bwd: null argument");
    WnResMsArgs a;
    memset(&a, 0, sizeof(a));
    a.x_in = x_in; a.dy = dy; a.dz = h; a.dfg = dh; a.x_bstride = x_bstride; a.dz_bstride = h_bstride;
    a.dfg_bstride = dh_bstride; a.pitch = pitch; a.wdT = wdT; a.slab_fg = slab_dil; a.slab_d = slab_d;
    a.d = d; a.t_lo = t_lo; a.t_hi = t_hi; a.z_lo = y_lo < t_lo ? t_lo : y_lo;
    return wn_launch_enc_bwd_rw(a, ch, batch, mode_bwd, (hipStream_t)stream);
}
int wn_enc_resblock_bwd_slabs(int t_lo, int t_hi, int batch) { return wn_enc_bwd_slabs(t_lo, t_hi, batch); }
int wn_enc_resblock_bwd_pq(const float* x_in, const float* p_in, const float* q_in, int dn, int p_lo, const float* h,
                           float* p_out, float* q_out, int64_t x_bstride, int64_t h_bstride, int pitch, const uint16_t* wdT,
                           const uint16_t* wpq, int ch, int d, int t_lo, int t_hi, float* slab_dil, float* slab_d, int chain, int batch,
                           int mode_bwd, wn_stream_t stream) {
    if (pitch % 4 != 0) return wn_set_error_msg(-4, "wn_enc_resblock_bwd_pq: pitch must be a multiple of 4");
    if (!x_in || !p_in || !h || !p_out || (!q_out && !chain) || !wdT || !wpq || !slab_dil || !slab_d)
        return wn_set_error_msg(-4, "wn_enc_resblock_bwd_pq: null argument");
    WnEncPqArgs a;
    memset(&a, 0, sizeof(a));
    a.x_in = x_in; a.p_in = p_in; a.q_in = q_in; a.dn = q_in ? dn : 0; a.p_lo = p_lo; a.h = h; a.h_bstride = h_bstride;
    a.p_out = p_out; a.q_out = q_out; a.x_bstride = x_bstride; a.pitch = pitch; a.wdT = wdT; a.wpq = wpq;
    a.slab_dil = slab_dil; a.slab_d = slab_d; a.d = d; a.t_lo = t_lo; a.t_hi = t_hi; a.chain = chain == 2 ? 2 : chain ? 1 : 0;
    return wn_launch_enc_bwd_pq(a, ch, batch, mode_bwd, (hipStream_t)stream);
}
int wn_resblock_bwd_ms_slabs(int t_lo, int t_hi, int batch) { return wn_resms_slabs(t_lo, t_hi, batch); }

int wn_resblock_bwd_pq(const float* x_in, const float* p_in, const float* q_in, int dn, int p_lo, const float* dz,
                       float* p_out, float* q_out, int64_t x_bstride, int64_t dz_bstride, int pitch, const uint16_t* wfg,
                       const uint16_t* wdT, const uint16_t* wpq, int ch, int d, int t_lo, int t_hi, int z_lo,
                       float* slab_fg, float* slab_d, const float* cond, int64_t cond_bstride, int cond_pitch, int cond_le,
                       const uint8_t* cond_idx, float* cslab, int64_t dz_half_stride, int chain, int batch, int mode_fwd,
                       int mode_bwd, wn_stream_t stream) {
    if (pitch % 4 != 0) return wn_set_error_msg(-4, "wn_resblock_bwd_pq: pitch must be a multiple of 4");
    if (cond && (!cond_idx || cond_le < 1 || cond_le > 32))
        return wn_set_error_msg(-4, "wn_resblock_bwd_pq: a conditioned block needs cond_idx and 1..32 buckets");
    if (cslab && !cond) return wn_set_error_msg(-4, "wn_resblock_bwd_pq: cslab without cond");
    if (ch != 64) return wn_set_error_msg(-3, "wn_resblock_bwd_pq: 64 padded channels only");
    if (mode_fwd != WN_MODE_F16X3 || mode_bwd != WN_MODE_BF16X3) return wn_set_error_msg(-2, "wn_resblock_bwd_pq: (f16x3, bf16x3) only");
    if (!x_in || !dz || !p_out || (!q_out && !chain) || !wfg || !wpq || !slab_fg) return wn_set_error_msg(-4, "wn_resblock_bwd_pq: null argument");
    if ((p_in && !wdT) || (!p_in && q_in)) return wn_set_error_msg(-4, "wn_resblock_bwd_pq: p_in and wdT go together, q_in needs p_in");
    if (chain && (cond || dz_half_stride < 0)) return wn_set_error_msg(-4, "wn_resblock_bwd_pq: no chain form of a conditioned block");
    WnResPqArgs a;
    memset(&a, 0, sizeof(a));
    a.x_in = x_in; a.p_in = p_in; a.q_in = q_in; a.dn = dn; a.p_lo = p_lo; a.dz = dz; a.p_out = p_out; a.q_out = q_out;
    a.x_bstride = x_bstride; a.dz_bstride = dz_bstride; a.pitch = pitch; a.wfg = wfg; a.wdT = wdT; a.wpq = wpq;
    a.slab_fg = slab_fg; a.slab_d = p_in ? slab_d : nullptr; a.d = d; a.t_lo = t_lo; a.t_hi = t_hi; a.z_lo = z_lo;
    a.cond = cond; a.cond_bstride = cond_bstride; a.cond_pitch = cond_pitch; a.cond_le = cond_le;
    a.cond_idx = cond ? cond_idx : nullptr; a.cslab = cslab; a.dz_half = dz_half_stride; a.chain = chain ? 1 : 0;
    return wn_launch_resblock_bwd_pq(a, batch, (hipStream_t)stream);
}
int wn_resblock_bwd_pq_chain_ok(int t_lo, int t_hi, int batch, int d) { return wn_pq_chain_ok(t_lo, t_hi, batch, d); }
int wn_resblock_bwd_pq_slabs(int t_lo, int t_hi, int batch, int d, int chain) { return wn_pq_slabs(t_lo, t_hi, batch, d, chain); }
int wn_resblock_bwd_pq_chain_items(int t_lo, int t_hi, int batch, int d, int wg, int* out, int cap) {
    return wn_pq_chain_items(t_lo, t_hi, batch, d, wg, out, cap);
}
int wn_resblock_bwd_pq_cond_floats(int t_lo, int t_hi, int batch) { return wn_pq_cond_slab_floats(t_lo, t_hi, batch); }
int wn_resblock_bwd_pq_cond_reduce(const float* cslab, const int64_t* slab_off, const int* t_lo, int n_launches, int t_hi, int batch,
                                   int cond_le, float* out, int64_t out_lstride, int64_t out_bstride, int out_pitch,
                                   wn_stream_t stream) {
    if (!cslab || !out || !slab_off || !t_lo || n_launches < 1 || cond_le < 1 || cond_le > 32)
        return wn_set_error_msg(-4, "wn_resblock_bwd_pq_cond_reduce: bad argument");
    static_assert(sizeof(long) == sizeof(int64_t), "LP64");
    return wn_launch_pq_cond_reduce(cslab, reinterpret_cast<const long*>(slab_off), t_lo, n_launches, t_hi, batch, cond_le, out,
                                    (long)out_lstride, (long)out_bstride, out_pitch, (hipStream_t)stream);
}
int wn_gate_fwd(const float* fg, int64_t fg_bstride, int dp, int rows, float* z, int64_t z_bstride, int pitch, int t_lo, int t_hi,
                int batch, wn_stream_t stream) {
    if (!fg || !z || rows > dp) return wn_set_error_msg(-4, "wn_gate_fwd: bad argument");
    return wn_launch_gate_fwd(fg, (long)fg_bstride, dp, rows, z, (long)z_bstride, pitch, t_lo, t_hi, batch, (hipStream_t)stream);
}
int wn_gate_bwd(const float* fg, int64_t fg_bstride, int dp, int rows, const float* dz, int64_t dz_bstride, float* dfg,
                int64_t dfg_bstride, int pitch, int t_lo, int t_hi, int batch, wn_stream_t stream) {
    if (!fg || !dz || !dfg || rows > dp) return wn_set_error_msg(-4, "wn_gate_bwd: bad argument");
    return wn_launch_gate_bwd(fg, (long)fg_bstride, dp, rows, dz, (long)dz_bstride, dfg, (long)dfg_bstride, pitch, t_lo, t_hi, batch,
                              (hipStream_t)stream);
}
int wn_chunk_softmax_fwd(const float* x, float* y, int64_t nrows, int q, wn_stream_t stream) {
    if (q < 1 || (nrows > 0 && (!x || !y))) return wn_set_error_msg(-4, "wn_chunk_softmax_fwd: bad argument");
    return wn_launch_softmaxq_fwd(x, y, (long)nrows, q, (hipStream_t)stream);
}
int wn_chunk_softmax_bwd(const float* y, const float* dy, float* dx, int64_t nrows, int q, wn_stream_t stream) {
    if (q < 1 || (nrows > 0 && (!y || !dy || !dx))) return wn_set_error_msg(-4, "wn_chunk_softmax_bwd: bad argument");
    return wn_launch_softmaxq_bwd(y, dy, dx, (long)nrows, q, (hipStream_t)stream);
}
int wn_chunk_softmax_ce(const float* x, const int64_t* target, float* probs, float* dx, float* loss_part, int64_t nrows, int q,
                        float inv_n, wn_stream_t stream) {
    if (q < 1 || (nrows > 0 && (!x || !target))) return wn_set_error_msg(-4, "wn_chunk_softmax_ce: bad argument");
    return wn_launch_softmaxq_ce(x, target, probs, dx, loss_part, (long)nrows, q, inv_n, (hipStream_t)stream);
}
int wn_split16(const float* x, uint16_t* hi, uint16_t* lo, int64_t n, int is_bf16, wn_stream_t stream) {
    if (n > 0 && (!x || !hi || !lo)) return wn_set_error_msg(-4, "wn_split16: null argument");
    return wn_launch_split16(x, hi, lo, (long)n, is_bf16, (hipStream_t)stream);
}
int wn_shift_add(const float* p, const float* q, float* out, int64_t bstride, int pitch, int rows, int dn, int p_lo,
                 int t_lo, int t_hi, int batch, wn_stream_t stream) {
    if (batch > 0 && rows > 0 && t_hi > t_lo) WN_REQUIRE("wn_shift_add", p, q, out);
    return wn_launch_shift_add(p, q, out, bstride, pitch, rows, dn, p_lo, t_lo, t_hi, batch, (hipStream_t)stream);
}

int wn_causal_wgrad_codes(const int32_t* codes, int scrambled, const float* dx, const float* dx_q, int dn, int p_lo,
                          int64_t dx_bstride, int pitch, int ch, int q, int t, int batch, float* slab, wn_stream_t stream) {
    if (q != 256) return wn_set_error_msg(-4, "wn_causal_wgrad_codes: 256 quantisation channels only");
    if (!codes || !dx || !slab) return wn_set_error_msg(-4, "wn_causal_wgrad_codes: null argument");
    return wn_launch_causal_wgrad_codes(codes, scrambled, dx, dx_q, dn, p_lo, dx_bstride, pitch, ch, t, batch, slab, (hipStream_t)stream);
}
int wn_causal_wgrad_codes_slabs(int t, int batch) { return wn_causal_codes_slabs(t, batch); }
int wn_causal_fwd_codes(const int32_t* codes, int scrambled, const float* wt, const float* bias, int n_rows, float* x0,
                        int64_t x_bstride, int pitch, int ch, int q, int t, int batch, wn_stream_t stream) {
    if (q != 256) return wn_set_error_msg(-4, "wn_causal_fwd_codes: 256 quantisation channels only");
    if (!codes || !wt || !x0) return wn_set_error_msg(-4, "wn_causal_fwd_codes: null argument");
    return wn_launch_causal_fwd_codes(codes, scrambled, wt, bias, n_rows, x0, x_bstride, pitch, ch, t, batch, (hipStream_t)stream);
}

int wn_cond_grad(const float* in, int64_t in_bstride, int in_pitch, int rows, int t_lo, int t_hi, int mode, int le,
                 int q, float* out, int64_t out_bstride, int out_pitch, int batch, wn_stream_t stream) {
    if ((mode != 1 && mode != 2) || (mode == 1 && q <= 0))
        return wn_set_error_msg(-4, "wn_cond_grad: mode must be 1 (stretch, q > 0) or 2 (tile)");
    // the launcher launches whenever rows, batch, le > 0 - an empty window too, which stores le zeros per row through `out`
    if (batch > 0 && rows > 0 && le > 0) WN_REQUIRE("wn_cond_grad", in, out);
    return wn_launch_cond_grad(in, in_bstride, in_pitch, rows, t_lo, t_hi, mode, le, q, out, out_bstride, out_pitch, batch,
                               (hipStream_t)stream);
}
int wn_cond_expand(const float* tab, int64_t tab_bstride, int tab_pitch, int rows, int t_lo, int t_hi, int mode, int le, int q,
                   float* out, int64_t out_bstride, int out_pitch, int batch, wn_stream_t stream) {
    if (!tab || !out || le <= 0 || (mode == 1 && q <= 0) || (mode != 1 && mode != 2))
        return wn_set_error_msg(-4, "wn_cond_expand: bad argument");
    return wn_launch_cond_expand(tab, (long)tab_bstride, tab_pitch, rows, t_lo, t_hi, mode, le, q, out, (long)out_bstride, out_pitch,
                                 batch, (hipStream_t)stream);
}
int wn_avgpool_bwd(const float* denc, int64_t denc_bstride, int denc_pitch, int t0, int pool, int n_out, int rows,
                   float* out, int64_t out_bstride, int out_pitch, int t_hi, int batch, wn_stream_t stream) {
    if (batch > 0 && rows > 0) WN_REQUIRE("wn_avgpool_bwd", denc, out);
    return wn_launch_avgpool_bwd(denc, denc_bstride, denc_pitch, t0, pool, n_out, rows, out, out_bstride, out_pitch, t_hi,
                                 batch, (hipStream_t)stream);
}

int wn_avgpool(const float* in, int64_t in_bstride, int in_pitch, int t0, int pool, int n_out, int rows,
               float* out, int64_t out_bstride, int out_pitch, int batch, wn_stream_t stream) {
    if (batch > 0 && rows > 0 && n_out > 0) WN_REQUIRE("wn_avgpool", in, out);
    return wn_launch_avgpool(in, in_bstride, in_pitch, t0, pool, n_out, rows, out, out_bstride, out_pitch, batch,
                             (hipStream_t)stream);
}

int64_t wn_decode_sync_granules(int n_layers, int D, int S) {
    return (int64_t)wn_decode_granules(n_layers, D, S);      // z of every block, the split form's vectors, the tap-0 table, code, error flag
}

int wn_decode(int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host, const int64_t* q_off_host,
              float* queues, const float* w_causal, const float* b_causal, const float* w_layers,
              int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
              const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
              float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
              int n_steps, int push_input, uint64_t* sync, wn_stream_t stream) {
    return decode_checked("wn_decode", 0, (int64_t)n_layers * D + 2, 2, n_layers, R, D, S, Q, dilations_host, q_off_host, queues,
                          w_causal, b_causal, w_layers, layer_stride, b_layers, w_p1, b_p1, w_p2, b_p2, note0, prev0, note_out,
                          prev_out, forced, codes_out, probs_out, step0, n_steps, push_input, sync, 1, 0, 0.0f, 0,
                          nullptr, 0, 0, 0, -1, -1, -1, nullptr, 0, nullptr, 0, nullptr, nullptr, 1, 0, nullptr, 0, 1.0f, nullptr, 0, 0, nullptr, stream);
}

int wn_decode_batch(int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host, const int64_t* q_off_host,
                    float* queues, const float* w_causal, const float* b_causal, const float* w_layers,
                    int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                    const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                    float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                    int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                    uint64_t seed, wn_stream_t stream) {
    return decode_checked("wn_decode_batch", 0, (int64_t)n_layers * D + 2, 2, n_layers, R, D, S, Q, dilations_host, q_off_host,
                          queues, w_causal, b_causal, w_layers, layer_stride, b_layers, w_p1, b_p1, w_p2, b_p2, note0, prev0,
                          note_out, prev_out, forced, codes_out, probs_out, step0, n_steps, push_input, sync, n_utt, queues_ustride,
                          temperature, seed, nullptr, 0, 0, 0, -1, -1, -1, nullptr, 0, nullptr, 0, nullptr, nullptr, 1, 0,
                          nullptr, 0, 1.0f, nullptr, 0, 0, nullptr, stream);
}

int wn_decode_batch_pk(int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host, const int64_t* q_off_host,
                       float* queues, const float* w_causal, const float* b_causal, const float* w_layers,
                       int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                       const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                       float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                       int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                       uint64_t seed, const uint16_t* pk, int64_t pk_fg0, int64_t pk_d0, int64_t pk_lstride, int64_t pk_skip,
                       int64_t pk_p1, int64_t pk_p2, wn_stream_t stream) {
    return decode_checked("wn_decode_batch_pk", 0, wn_decode_sync_granules(n_layers, D, S), 2, n_layers, R, D, S, Q, dilations_host,
                          q_off_host, queues, w_causal, b_causal, w_layers, layer_stride, b_layers, w_p1, b_p1, w_p2, b_p2, note0,
                          prev0, note_out, prev_out, forced, codes_out, probs_out, step0, n_steps, push_input, sync, n_utt,
                          queues_ustride, temperature, seed, pk, pk_fg0, pk_d0, pk_lstride, pk_skip, pk_p1, pk_p2,
                          nullptr, 0, nullptr, 0, nullptr, nullptr, 1, 0, nullptr, 0, 1.0f, nullptr, 0, 0, nullptr, stream);
}

int wn_decode_batch_fw(int filter_width, int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host,
                       const int64_t* q_off_host, float* queues, const float* w_causal, const float* b_causal,
                       const float* w_layers, int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                       const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                       float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                       int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                       uint64_t seed, const uint16_t* pk, int64_t pk_fg0, int64_t pk_d0, int64_t pk_lstride, int64_t pk_skip,
                       int64_t pk_p1, int64_t pk_p2, wn_stream_t stream) {
    return decode_checked("wn_decode_batch_fw", DEC_FW, wn_decode_sync_granules(n_layers, D, S), filter_width, n_layers, R, D, S, Q,
                          dilations_host, q_off_host, queues, w_causal, b_causal, w_layers, layer_stride, b_layers, w_p1, b_p1, w_p2,
                          b_p2, note0, prev0, note_out, prev_out, forced, codes_out, probs_out, step0, n_steps, push_input, sync,
                          n_utt, queues_ustride, temperature, seed, pk, pk_fg0, pk_d0, pk_lstride, pk_skip, pk_p1, pk_p2,
                          nullptr, 0, nullptr, 0, nullptr, nullptr, 1, 0, nullptr, 0, 1.0f, nullptr, 0, 0, nullptr, stream);
}

int wn_decode_batch_cond(int filter_width, int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host,
                         const int64_t* q_off_host, float* queues, const float* w_causal, const float* b_causal,
                         const float* w_layers, int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                         const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                         float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                         int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                         uint64_t seed, const uint16_t* pk, int64_t pk_fg0, int64_t pk_d0, int64_t pk_lstride, int64_t pk_skip,
                         int64_t pk_p1, int64_t pk_p2, const float* cond_fg, int64_t cond_fg_ustride, const float* cond_p1,
                         int64_t cond_p1_ustride, const int32_t* c_shift_host, const int32_t* c_q_host, int le, int64_t pos0,
                         wn_stream_t stream) {
    return decode_checked("wn_decode_batch_cond", DEC_FW | DEC_COND, wn_decode_sync_granules(n_layers, D, S), filter_width, n_layers,
                          R, D, S, Q, dilations_host, q_off_host, queues, w_causal, b_causal, w_layers, layer_stride, b_layers, w_p1,
                          b_p1, w_p2, b_p2, note0, prev0, note_out, prev_out, forced, codes_out, probs_out, step0, n_steps,
                          push_input, sync, n_utt, queues_ustride, temperature, seed, pk, pk_fg0, pk_d0, pk_lstride, pk_skip, pk_p1,
                          pk_p2, cond_fg, cond_fg_ustride, cond_p1, cond_p1_ustride, c_shift_host, c_q_host, le, pos0,
                          nullptr, 0, 1.0f, nullptr, 0, 0, nullptr, stream);
}

int wn_decode_batch_samp(int filter_width, int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host,
                         const int64_t* q_off_host, float* queues, const float* w_causal, const float* b_causal,
                         const float* w_layers, int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                         const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                         float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                         int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                         uint64_t seed, const uint16_t* pk, int64_t pk_fg0, int64_t pk_d0, int64_t pk_lstride, int64_t pk_skip,
                         int64_t pk_p1, int64_t pk_p2, const float* cond_fg, int64_t cond_fg_ustride, const float* cond_p1,
                         int64_t cond_p1_ustride, const int32_t* c_shift_host, const int32_t* c_q_host, int le, int64_t pos0,
                         const wn_sampling* samp, int top_k, float top_p, wn_stream_t stream) {
    return decode_checked("wn_decode_batch_samp", DEC_FW | DEC_COND | DEC_SAMP, wn_decode_sync_granules(n_layers, D, S), filter_width,
                          n_layers, R, D, S, Q, dilations_host, q_off_host, queues, w_causal, b_causal, w_layers, layer_stride,
                          b_layers, w_p1, b_p1, w_p2, b_p2, note0, prev0, note_out, prev_out, forced, codes_out, probs_out, step0,
                          n_steps, push_input, sync, n_utt, queues_ustride, temperature, seed, pk, pk_fg0, pk_d0, pk_lstride, pk_skip,
                          pk_p1, pk_p2, cond_fg, cond_fg_ustride, cond_p1, cond_p1_ustride, c_shift_host, c_q_host, le, pos0, samp,
                          top_k, top_p, nullptr, 0, 0, nullptr, stream);
}

int wn_win_decode_batch(int filter_width, int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host,
                        const int64_t* q_off_host, float* queues, const float* w_causal, const float* b_causal,
                        const float* w_layers, int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                        const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                        float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                        int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                        uint64_t seed, const uint16_t* pk, int64_t pk_fg0, int64_t pk_d0, int64_t pk_lstride, int64_t pk_skip,
                        int64_t pk_p1, int64_t pk_p2, const float* cond_fg, int64_t cond_fg_ustride, const float* cond_p1,
                        int64_t cond_p1_ustride, const int32_t* c_shift_host, const int32_t* c_q_host, int le, int64_t pos0,
                        const wn_sampling* samp, int top_k, float top_p, const int32_t* win_host, int win_period,
                        int64_t win_pos0, wn_stream_t stream) {
    return decode_checked("wn_win_decode_batch", DEC_FW | DEC_COND | DEC_SAMP | DEC_WIN, wn_decode_sync_granules(n_layers, D, S),
                          filter_width, n_layers, R, D, S, Q, dilations_host, q_off_host, queues, w_causal, b_causal, w_layers,
                          layer_stride, b_layers, w_p1, b_p1, w_p2, b_p2, note0, prev0, note_out, prev_out, forced, codes_out,
                          probs_out, step0, n_steps, push_input, sync, n_utt, queues_ustride, temperature, seed, pk, pk_fg0, pk_d0,
                          pk_lstride, pk_skip, pk_p1, pk_p2, cond_fg, cond_fg_ustride, cond_p1, cond_p1_ustride, c_shift_host,
                          c_q_host, le, pos0, samp, top_k, top_p, win_host, win_period, win_pos0, nullptr, stream);
}

int wn_sample_logits(const float* logits, int64_t n, int Q, int64_t ld, const wn_sampling* samp, float temperature, uint64_t seed,
                     int top_k, float top_p, int64_t step0, const float* u, int32_t* codes, float* probs, wn_stream_t stream) {
    return sample_checked("wn_sample_logits", false, logits, n, Q, ld, samp, temperature, seed, top_k, top_p, step0, u, codes, probs,
                          nullptr, 0, 0, stream);
}

int wn_win_sample_logits(const float* logits, int64_t n, int Q, int64_t ld, const wn_sampling* samp, float temperature, uint64_t seed,
                         int top_k, float top_p, int64_t step0, const float* u, int32_t* codes, float* probs,
                         const int32_t* win_host, int win_period, int64_t win_pos0, wn_stream_t stream) {
    return sample_checked("wn_win_sample_logits", true, logits, n, Q, ld, samp, temperature, seed, top_k, top_p, step0, u, codes, probs,
                          win_host, win_period, win_pos0, stream);
}

int wn_cfg_decode_batch(int filter_width, int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host,
                        const int64_t* q_off_host, float* queues, const float* w_causal, const float* b_causal,
                        const float* w_layers, int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                        const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                        float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                        int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                        uint64_t seed, const uint16_t* pk, int64_t pk_fg0, int64_t pk_d0, int64_t pk_lstride, int64_t pk_skip,
                        int64_t pk_p1, int64_t pk_p2, const float* cond_fg, int64_t cond_fg_ustride, const float* cond_p1,
                        int64_t cond_p1_ustride, const int32_t* c_shift_host, const int32_t* c_q_host, int le, int64_t pos0,
                        const wn_sampling* samp, int top_k, float top_p, const int32_t* win_host, int win_period,
                        int64_t win_pos0, const float* guidance, wn_stream_t stream) {
    return decode_checked("wn_cfg_decode_batch", DEC_FW | DEC_COND | DEC_SAMP | DEC_WIN | DEC_CFG, wn_decode_sync_granules(n_layers, D, S),
                          filter_width, n_layers, R, D, S, Q, dilations_host, q_off_host, queues, w_causal, b_causal, w_layers,
                          layer_stride, b_layers, w_p1, b_p1, w_p2, b_p2, note0, prev0, note_out, prev_out, forced, codes_out,
                          probs_out, step0, n_steps, push_input, sync, n_utt, queues_ustride, temperature, seed, pk, pk_fg0, pk_d0,
                          pk_lstride, pk_skip, pk_p1, pk_p2, cond_fg, cond_fg_ustride, cond_p1, cond_p1_ustride, c_shift_host,
                          c_q_host, le, pos0, samp, top_k, top_p, win_host, win_period, win_pos0, guidance, stream);
}

int wn_cfg_sample_logits(const float* logits_c, int64_t n, int Q, int64_t ld, const wn_sampling* samp, float temperature, uint64_t seed,
                         int top_k, float top_p, int64_t step0, const float* u, int32_t* codes, float* probs,
                         const int32_t* win_host, int win_period, int64_t win_pos0, const float* logits_u, const float* guidance,
                         wn_stream_t stream) {
    return sample_checked("wn_cfg_sample_logits", true, logits_c, n, Q, ld, samp, temperature, seed, top_k, top_p, step0, u, codes, probs,
                          win_host, win_period, win_pos0, stream, logits_u, guidance);
}

}  // extern "C"
