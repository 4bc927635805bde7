/* libwavenet_hip.so — C ABI of the MI355X (gfx950) WaveNet hot path.
 *
 * The reference (deep-art-project/Music) is pure Python/PyTorch: it has no FFI, plugin table or
 * operator registry for this path.  The drop-in boundary is therefore the
 * torch.nn.Module surface of wavenet/model.py, which music_amd/model.py mirrors; that module calls
 * ONLY the entry points below (through ctypes, music_amd/_lib.py).  Each entry point names the
 * reference code it replaces.  INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Rules of the ABI
 *   - plain C types only: device pointers, sizes, a stream handle (hipStream_t passed as void*);
 *   - returns 0 on success, a negative code on error (wn_last_error() gives the text); no C++
 *     exceptions cross the boundary;
 *   - a call that has work to do checks its REQUIRED pointers first: a NULL one returns -4 and wn_last_error() names the
 *     function and the argument, nothing is launched (pointers documented as optional may be NULL; a call with no work -
 *     zero clips / rows / columns / elements - returns 0 whatever its pointers are);
 *   - no allocation, no synchronisation, no retained pointers: all workspace is the caller's,
 *     every call only enqueues work on `stream` (safe under hipGraph stream capture);
 *   - re-entrant across devices/streams and threads: no global mutable state; the last-error text is
 *     thread-local (wn_last_error() returns the calling thread's);
 *   - the one collective of the path (the data-parallel gradient sum) is `wn_allreduce_flat` on a communicator
 *     the CALLER owns; RCCL is resolved at first use from the process image (or librccl.so), not linked.  The Python host keeps
 *     `torch.distributed.all_reduce(flat_grad)` (music_amd/dist.py): ProcessGroupNCCL owns its communicator and does not hand
 *     the ncclComm_t out, and a second communicator behind its back would duplicate the xGMI rings and the bootstrap for one
 *     5 MB all-reduce per step; a host without torch uses the entry points below.
 *
 * Data layout: activations are float32 [clip][channel][time] with time
 * contiguous, in ABSOLUTE time (column t = index of the newest input sample the value depends
 * on), all with one row pitch (multiple of 4 floats) and 16-byte aligned bases, allocated with
 * >= 64 floats of slack in front of and >= 256 behind the addressed range.  Channel counts are
 * padded to a multiple of 32 with zero weights.  "mode" selects the arithmetic of the
 * channel-mixing products on the v_mfma_f32_16x16x32 matrix cores:
 *   WN_F16X3 / WN_BF16X3 : operands split x = hi + lo in f16 / bf16, 3 MFMAs per product,
 *                          fp32 accumulate (fp32-grade, the default: fwd F16X3, bwd BF16X3)
 *   WN_F16X1 / WN_BF16X1 : plain 16-bit operands, fp32 accumulate.
 */
#ifndef WAVENET_HIP_H
#define WAVENET_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* wn_stream_t;                 /* hipStream_t */
enum { WN_F16X3 = 0, WN_F16X1 = 1, WN_BF16X3 = 2, WN_BF16X1 = 3 };
#define WN_ABI_VERSION 9
#define WN_CE_NUM_PARTIALS 1024
#define WN_GUARD_NUM_PARTIALS 256           /* workgroups of wn_grad_guard's first launch = entries of its partials */
#define WN_GUARD_PARTIALS_BYTES (WN_GUARD_NUM_PARTIALS * 12)   /* bytes of `partials`: a double and a uint32 per workgroup */
#define WN_GUARD_STATE_BYTES 48             /* sizeof(wn_guard_state) */

int wn_version(void);
const char* wn_last_error(void);

/* Weight packing: flat fp32 parameter buffer -> MFMA A-fragment order, 16-bit hi(/lo) pieces.
 * idx[p] = offset of the source weight in `flat` (or -1 = structural zero) for logical position
 * p = (fragment, lane, j); n = number of logical positions (multiple of 512).
 * Replaces nothing in the reference (cuDNN consumes nn.Conv1d weights directly). */
int wn_pack_weights(const float* flat, const int32_t* idx, uint16_t* out, int n, int mode,
                    wn_stream_t stream);

/* Generic channel-mixing product over time:
 *   out[b][m][t+out_shift] = resid[b][m][t] (t >= resid_lo) + mask( bias[m]
 *        + sum_k W[m][k]      * pre(in0[b][k][t+shift0])            (k <  32*ks0)
 *        + sum_k W[m][K0 + k] * pre(in1[b][k][t+shift1]) )          (k <  32*ks1)
 * for t in [t_lo, t_hi); pre = relu if relu_in; mask keeps values where mask[b][m][t] > 0.
 * input columns (t+shift) outside [in_lo,in_hi) read as 0 and are never dereferenced.  Replaces: causal nn.Conv1d (wavenet/model.py:104),
 * the skip 1x1 convs + Python sum (model.py:127-134), post_process_1/2 (model.py:136-138) and
 * their autograd backward (data gradients). */
int wn_chan_gemm(const float* in0, const float* in1, int64_t in_bstride, int in_pitch, int in_lo, int in_hi,
                 int shift0, int shift1, int ks0, int ks1, const uint16_t* wpack, int mt, int m_valid,
                 float* out, int64_t out_bstride, int out_pitch, int out_shift, const float* bias,
                 const float* resid, int64_t resid_bstride, int resid_pitch, int resid_lo,
                 const float* mask, int64_t mask_bstride, int mask_pitch,
                 int t_lo, int t_hi, int relu_in, int batch, int mode, wn_stream_t stream);

/* Fused gated residual block, forward (wavenet/model.py:111-129 for one dilation d):
 *   [f;g] = Wfg [x(t-d); x(t)] ; z = tanh f * sigmoid g ; x_out = Wd z + x(t) on [t_lo,t_hi);
 *   z is stored on [z_lo, t_hi) (the crop the skip product needs).  ch = padded channels (32|64).  All ch rows of z and
 *   (write_x != 0) of x_out are written on their windows, the padded rows - zero weights, no bias (rows >= n_f / n_d), zero
 *   table rows - as exact zeros; nothing else is touched, and with write_x == 0 x_out is not touched at all.
 * Optional conditioning of the autoencoder's decoder (wavenet_autoencoder/model1.py:175-192,
 * 227-247): [f;g][row][t] += cond[b][row][idx(t)], cond = [B][2*ch][cond_pitch] (rows f then g),
 * idx = (t - t_lo) / cond_q when cond_mode == 1 ("stretch"), (t - t_lo) % cond_le when 2 ("tile");
 * cond == NULL disables it.  Optional, for ch = 64, mode f16x3 and cond_le <= 32: the same table once more as packed
 * A fragments, cond_pack[b] = wn_pack_weights order of the [2*ch rows][K = 32 buckets, zero beyond cond_le] matrix
 * (8 fragments = cond_pack_bstride 8192 halfs per clip), and the buckets as bytes, cond_idx (layout under
 * wn_resblock_bwd_pq) - the bias is then one more k-step of the fg product (table x 0/1 matrix on the matrix cores,
 * hi + lo: the table to ~2^-22) instead of 128 gathered loads per lane; NULL: the gather.
 * z_half_stride != 0 (ch = 64): TWO clips of a model with <= 32 channels side by side on the 64-channel block - x / x_out
 * are the two clips' 32-row tensors back to back (x_bstride = 64 rows), the packs block-diagonal ([W 0; 0 W] per product:
 * the zero blocks cost matrix time, no traffic), and the z rows of the second clip go z_half_stride floats behind the
 * first clip's (its own z slice) instead of 32 rows below them.  Same results as two launches of the 32-channel form. */
int wn_resblock_fwd(const float* x_in, float* x_out, float* z_out, int64_t x_bstride, int64_t z_bstride,
                    int pitch, const uint16_t* wfg, const uint16_t* wd, const float* bias_f,
                    const float* bias_g, const float* bias_d, int n_f, int n_d, int ch, int d,
                    int t_lo, int t_hi, int z_lo, int write_x, const float* cond, int64_t cond_bstride,
                    int cond_pitch, int cond_mode, int cond_le, int cond_q, const uint16_t* cond_pack,
                    int64_t cond_pack_bstride, const uint8_t* cond_idx, int64_t z_half_stride, int batch, int mode,
                    wn_stream_t stream);

/* Fused gated residual block, backward recompute half (autograd of model.py:118-124, SURVEY
 * Appendix B): recomputes f,g,z from x_in; dz = Wd^T dy (+ dz_crop on t >= z_lo);
 * writes dfg = [df; dg] (2*ch rows) and z (ch rows) on [t_lo,t_hi).  dy may be NULL; z may be NULL
 * (the caller kept the forward's z, stored with z_lo = t_lo): dfg then has the same bits and z is not touched.
 * cond*: the conditioning table of wn_resblock_fwd (the recompute adds it as well); NULL = none.
 * dy has x_in's layout: its clip stride is x_bstride as well.  All 2*ch rows of dfg and all ch rows of z are written on the
 * window, the padded rows (zero weights, no bias at rows >= n_f, zero table rows) as exact zeros; nothing else is touched.
 * Supported (mode_fwd, mode_bwd): (f16x3, bf16x3), (f16x1, bf16x1), (bf16x3, bf16x3), (bf16x1, bf16x1), else -2; ch other than
 * 32 | 64: -3; pitch no multiple of 4: -4; t_hi <= t_lo or batch <= 0: returns 0 and writes nothing.
 * The launch tiles the columns from t_lo & ~63 in steps of 512 and READS the rows of x_in (also d columns in front of each
 * tile, so up to 63 floats in front of the first row when t_lo - d < 64: the activation layout's front slack), dy and dz over
 * whole tiles, so the tiles must lie inside the row pitch.  Values that do not count are ignored, NaN included: x_in at columns
 * < t_lo - d and >= t_hi, dy outside [t_lo, t_hi), dz at columns < z_lo and >= t_hi (all of it when z_lo >= t_hi), bias
 * entries at rows >= n_f, table columns >= cond_le (stretch: buckets beyond cond_le - 1 clamp to the last one). */
int wn_resblock_bwd(const float* x_in, const float* dy, const float* dz, float* dfg, float* z,
                    int64_t x_bstride, int64_t dz_bstride, int64_t dfg_bstride, int64_t z_bstride,
                    int pitch, const uint16_t* wfg, const uint16_t* wdT, const float* bias_f,
                    const float* bias_g, int n_f, int ch, int d, int t_lo, int t_hi, int z_lo,
                    const float* cond, int64_t cond_bstride, int cond_pitch, int cond_mode, int cond_le, int cond_q,
                    int batch, int mode_fwd, int mode_bwd, wn_stream_t stream);

/* The forward epilogue in ONE launch (ABI v5; replaces the skip 1x1 convs + Python sum, F.relu, post_process_1, F.relu,
 * post_process_2 of wavenet/model.py:127-138 - three wn_chan_gemm launches):  per tile of 128 columns
 *   u = bias_skip + Ws z ;  h = bias_p1 + P1 relu(u) ;  o = bias_p2 + P2 relu(h)        on [t_lo, t_hi)
 * z: the z-crops of all blocks stacked on the channel axis, [B][32 ks_skip][pitch] (ks_skip even), valid on [t_lo, t_hi).  The launch
 * tiles the columns from t_lo & ~63 in steps of 128 and READS every row over whole tiles (values outside [t_lo, t_hi) are ignored, NaN
 * included): the tiles must lie inside the row pitch (-4 otherwise), i.e. the rows need the activation layout's slack.  u, h: [B][256][pitch] (s_bstride floats per clip; rows >= s_valid are not written) -
 * the backward masks with them.  o: compact [B][256][o_pitch], column t - t_lo (the reference's pre-softmax memory order).
 * w_skip: packed [16][ks_skip], natural k.  w_p1c / w_p2c: packed [16][8] in the CHAINED k order (the u / h tile is handed from
 * product to product out of the accumulators, like wn_resblock_fwd's dense weights).  At most 256 skip and 256 quantisation
 * channels; x3 modes.  Biases may be NULL. */
int wn_skip_epilogue_fwd(const float* z, int64_t z_bstride, int pitch, int ks_skip, const uint16_t* w_skip, const float* bias_skip,
                         float* u, float* h, int64_t s_bstride, const uint16_t* w_p1c, const float* bias_p1,
                         const uint16_t* w_p2c, const float* bias_p2, float* o, int64_t o_bstride, int o_pitch,
                         int s_valid, int q_valid, int t_lo, int t_hi, int batch, int mode, wn_stream_t stream);

/* The backward of that epilogue, data gradients, in ONE launch (ABI v5; autograd of wavenet/model.py:127-138 - three
 * wn_chan_gemm launches):  per tile of 128 columns
 *   dh = (P2^T d_o) * [h > 0] ;  du = (P1^T dh) * [u > 0] ;  dz = Ws^T du        on [t_lo, t_hi)
 * d_o: compact [B][256][o_pitch], column t - t_lo (d loss / d pre-softmax).  h, u: the forward's tensors (masks); dh, du: same
 * layout, stored for the weight gradients (wn_wgrad).  dz: [B][16 mt_z][pitch], all blocks' z-crop gradients stacked on the channel
 * axis, mt_z a multiple of 3.  w_p2T: packed P2^T [16][8], natural k; w_p1Tc, w_skipTc: P1^T [16][8] and Ws^T [mt_z][8] in the
 * CHAINED k order.  The mask rows are read unguarded over the tile's 128 columns (workspace rows of the activation layout). */
int wn_skip_epilogue_bwd(const float* d_o, int64_t o_bstride, int o_pitch, const float* h, const float* u, int64_t s_bstride, int pitch,
                         float* d_h, float* d_u, float* d_z, int64_t z_bstride, const uint16_t* w_p2T, const uint16_t* w_p1Tc,
                         const uint16_t* w_skipTc, int mt_z, int z_valid, int s_valid, int t_lo, int t_hi, int batch, int mode,
                         wn_stream_t stream);

/* Encoder block of the autoencoder, forward (wavenet_autoencoder/model1.py:137-152 for one dilation d), one launch:
 *   h = Wdil [relu x(t-d); relu x(t)] (+ bias_dil) ; x_out = Wd relu(h) (+ bias_d) + x(t)   on [t_lo, t_hi);
 *   h (the pre-activation the backward masks with) is stored on the same range.  wdil: packed [ch/16][2ch/32] (natural
 *   k: tap 0 channels then tap 1 channels), wd: packed [ch/16][ch/32] in the chained k order (as wn_resblock_fwd's
 *   dense weights).  ch = padded channels (32|64); n_h / n_d = real dilation / residual channel counts. */
int wn_enc_resblock_fwd(const float* x_in, float* x_out, float* h_out, int64_t x_bstride, int64_t h_bstride, int pitch,
                        const uint16_t* wdil, const uint16_t* wd, const float* bias_dil, const float* bias_d, int n_h,
                        int n_d, int ch, int d, int t_lo, int t_hi, int batch, int mode, wn_stream_t stream);

/* Encoder block of the autoencoder, backward except the data gradient (64 padded channels, bf16x3), one launch:
 *   dh = (Wd^T dy) * [h > 0]  written on [t_lo, t_hi) (dy counts as 0 below y_lo: the top block's gradient only exists on
 *   the pooled crop);  one slab per workgroup: slab_dil[w] = partial dWdil (ch x 2ch, columns = tap0 ch | tap1 ch, the
 *   x operand is relu x), slab_d[w] = partial dWd (ch x ch, rows = dy rows, the other operand is relu h);
 *   wn_enc_resblock_bwd_slabs gives the number of slabs (sum them with wn_reduce_slabs).  The data gradient
 *   dx = [x > 0] (Wdil1^T dh[t] + Wdil0^T dh[t+d]) + dy is a wn_chan_gemm launch on dh.  wdT: packed Wd^T. */
int wn_enc_resblock_bwd(const float* x_in, const float* dy, const float* h, float* dh, int64_t x_bstride,
                        int64_t h_bstride, int64_t dh_bstride, int pitch, const uint16_t* wdT, int ch, int d, int t_lo,
                        int t_hi, int y_lo, float* slab_dil, float* slab_d, int batch, int mode_bwd, wn_stream_t stream);
int wn_enc_resblock_bwd_slabs(int t_lo, int t_hi, int batch);
/* The same backward with the data gradient INSIDE the launch (no biases), handed on as the unshifted pair of
 * wn_resblock_bwd_pq:  in : dy[t] = p_in[t] (t >= p_lo) + q_in[t + dn]  (the pair the block above wrote, dn = ITS dilation,
 * p_lo = ITS t_lo; q_in = NULL: p_in is a plain tensor valid from p_lo - the top block);
 * out: p_out[t] = dy[t] + [x(t) > 0] W1^T dh[t],  q_out[t] = [x(t-d) > 0] W0^T dh[t]  on [t_lo, t_hi), so that
 * dx[s] = p_out[s] + q_out[s + d] (wn_shift_add makes it whole); dh never reaches HBM.  x / P / Q share x_bstride and pitch,
 * q buffers must read as zero beyond t_hi.  wpq: packed [W1^T; W0^T] ([2ch rows][K = ch dh channels], bf16x3); slabs as
 * wn_enc_resblock_bwd.  Autograd of wavenet_autoencoder/model1.py:143-152 for one layer.
 * chain != 0 (d a multiple of 32, wn_resblock_bwd_pq_chain_ok; slabs = wn_resblock_bwd_pq_slabs(.., chain)): the CHAIN form of
 * wn_resblock_bwd_pq - a workgroup walks the items of one residue class downwards in time and carries the Q rows in registers, dx
 * leaves the launch WHOLE in p_out (valid on [t_lo - d, t_hi)), q_out is not touched (may be NULL); the block below takes it as a
 * plain tensor (q_in = NULL, p_lo = this launch's t_lo - d).  4 activation tensors per block instead of 6: the launch is bound by
 * its bytes (profiles/r05_ab_enc_noq.json).
 * chain == 2 (1 <= d < 32; slabs = wn_resblock_bwd_pq_slabs(t_lo, t_hi, batch, 32, 1)): the same hand-over for the small dilations - the
 * workgroups walk ADJACENT items downwards (the chain plan of d = 32) and an item's Q rows reach the dx rows of the same and of the next
 * item through LDS; dx whole in p_out on [t_lo - d, t_hi) as above. */
int wn_enc_resblock_bwd_pq(const float* x_in, const float* p_in, const float* q_in, int dn, int p_lo, const float* h,
                           float* p_out, float* q_out, int64_t x_bstride, int64_t h_bstride, int pitch, const uint16_t* wdT,
                           const uint16_t* wpq, int ch, int d, int t_lo, int t_hi, float* slab_dil, float* slab_d, int chain,
                           int batch, int mode_bwd, wn_stream_t stream);

/* Backward of one residual block with BOTH weight gradients in the launch (channel-split form,
 * 64 padded channels, modes (f16x3, bf16x3)): what wn_resblock_bwd + the two per-layer wn_wgrad calls
 * compute (autograd of wavenet/model.py:111-129 for one layer except the data gradient of the
 * dilated convs, which wn_chan_gemm forms from dfg).  Writes dfg = [df; dg] on [t_lo,t_hi) and one
 * slab per workgroup: slab_fg[w] = partial dWfg (2ch x 2ch, columns = tap0 ch | tap1 ch), slab_d[w] =
 * partial dWd (ch x ch); wn_resblock_bwd_ms_slabs gives the number of slabs (sum them with
 * wn_reduce_slabs).  dy NULL (last block): no dz product, no dWd.  z is not written at all.
 * cond*: the conditioning table of wn_resblock_fwd (the recompute adds it as well); NULL = none.
 * Kernel: the two-role persistent block of wn_resrw.hip (8 waves).  The buffers need the usual slack: rows are
 * read up to 63 columns outside [t_lo - d, t_hi). */
int wn_resblock_bwd_ms(const float* x_in, const float* dy, const float* dz, float* dfg, int64_t x_bstride,
                       int64_t dz_bstride, int64_t dfg_bstride, int pitch, const uint16_t* wfg, const uint16_t* wdT,
                       const float* bias_f, const float* bias_g, int n_f, int ch, int d, int t_lo, int t_hi, int z_lo,
                       float* slab_fg, float* slab_d, const float* cond, int64_t cond_bstride, int cond_pitch,
                       int cond_mode, int cond_le, int cond_q, int batch, int mode_fwd, int mode_bwd,
                       wn_stream_t stream);
int wn_resblock_bwd_ms_slabs(int t_lo, int t_hi, int batch);

/* The whole backward of one residual block in ONE launch, data gradient of the dilated convs included (64 padded
 * channels, modes (f16x3, bf16x3), no biases): what wn_resblock_bwd_ms + the wn_chan_gemm launch on its dfg compute,
 * without [df;dg] ever reaching HBM.  The data gradient travels between blocks as an UNSHIFTED pair:
 *   in : dx_{i+1}[t] = p_in[t] (t >= p_lo) + q_in[t + dn]   (the pair the block above wrote; dn = ITS dilation, p_lo =
 *        ITS t_lo; both NULL for the last block: no dz product, no dWd);
 *   out: p_out[t] = W1^T [df;dg][t] + dx_{i+1}[t],  q_out[t] = W0^T [df;dg][t]  on [t_lo, t_hi), so that
 *        dx_i[t] = p_out[t] + q_out[t + d] (wn_shift_add makes it whole where a plain tensor is needed).
 * x / P / Q share x_bstride and pitch; q buffers must read as zero beyond t_hi (never written there).  wpq: packed
 * [W1^T; W0^T] ([2ch rows][K = df | dg], bf16x3).  Slabs as wn_resblock_bwd_ms (same count: wn_resblock_bwd_ms_slabs).
 * Autograd of wavenet/model.py:111-129 for one layer.
 * The autoencoder's conditioned decoder blocks (wavenet_autoencoder/model1.py:183,227-247): cond != NULL is the table
 * cond[b][2ch rows][cond_le <= 32] whose column bucket(t) is added to [f;g][.][t]; the buckets come as bytes,
 * cond_idx[WN_COND_IDX_PAD + (t - t_lo)] for t in [t_lo, t_hi) with WN_COND_IDX_PAD zero bytes in front and 64 behind
 * (stretch or tile rule: whatever the caller wrote there), and the bias is formed on the matrix cores as one more k-step
 * of the recompute (table x 0/1 matrix).  cslab != NULL (wn_resblock_bwd_pq_cond_floats() floats): the conditioning
 * GRADIENT d cond[b][row][j] = sum of [df;dg][b][row][t] over bucket j is formed inside the launch as well (a 0/1
 * selection product, exact): every workgroup leaves its sums per clip in cslab and wn_resblock_bwd_pq_cond_reduce adds
 * them in a fixed order (no float atomics; the same sums as wn_cond_grad on the [df;dg] wn_resblock_bwd_ms writes, up to
 * summation order; dz_half_stride != 0: two 32-channel clips side by side as under wn_resblock_fwd - the dz-crop rows of the
 * second clip sit that many floats behind the first clip's, the slabs hold the block-diagonal gradients, wn_gather_grads2
 * adds the two copies) - for n_launches block launches in ONE reduce: launch l ran with t_lo[l] (HOST array, as slab_off) and
 * the same t_hi / batch and wrote its slabs at cslab + slab_off[l] floats; out[l][b][2ch rows][cond_le] with the strides
 * given.  More than 32 buckets: wn_resblock_bwd_ms + wn_cond_grad.
 * WHOLE forms (ABI 2).  q_in == NULL with p_in != NULL: the block above handed dx_{i+1} on as ONE tensor, p_in, valid on
 * [p_lo, t_hi).  chain != 0 (unconditioned blocks with d % 32 == 0 and at least d / 32 items of 32 columns per clip:
 * wn_resblock_bwd_pq_chain_ok): the launch walks its 32-column items in chains of stride d downwards in time, so that the Q
 * rows of an item are added to the P rows of the next one in registers - dx_i is written WHOLE to p_out on
 * [t_lo - d, t_hi), q_out is not touched, nothing else changes (same sums per item; the weight-gradient slabs follow the
 * chain plan: wn_resblock_bwd_pq_slabs(…, d, chain) slabs). */
#define WN_COND_IDX_PAD 64
int wn_resblock_bwd_pq(const float* x_in, const float* p_in, const float* q_in, int dn, int p_lo, const float* dz,
                       float* p_out, float* q_out, int64_t x_bstride, int64_t dz_bstride, int pitch, const uint16_t* wfg,
                       const uint16_t* wdT, const uint16_t* wpq, int ch, int d, int t_lo, int t_hi, int z_lo,
                       float* slab_fg, float* slab_d, const float* cond, int64_t cond_bstride, int cond_pitch, int cond_le,
                       const uint8_t* cond_idx, float* cslab, int64_t dz_half_stride, int chain, int batch, int mode_fwd,
                       int mode_bwd, wn_stream_t stream);
int wn_resblock_bwd_pq_chain_ok(int t_lo, int t_hi, int batch, int d);
int wn_resblock_bwd_pq_slabs(int t_lo, int t_hi, int batch, int d, int chain);
/* Host-only view of the chain plan (what tests check it with; nothing is launched): the items workgroup wg of a chain-form launch
 * walks, in order, as triples (clip, first column t0, flags: 1 = halo item - recomputed for its Q rows only, 2 = top of its chain,
 * 4 = bottom) written to out[3 * k ..]; returns the number of items (at most cap are written), -1 when there is no chain form. */
int wn_resblock_bwd_pq_chain_items(int t_lo, int t_hi, int batch, int d, int wg, int* out, int cap);
int wn_resblock_bwd_pq_cond_floats(int t_lo, int t_hi, int batch);
int wn_resblock_bwd_pq_cond_reduce(const float* cslab, const int64_t* slab_off, const int* t_lo, int n_launches, int t_hi, int batch,
                                   int cond_le, float* out, int64_t out_lstride, int64_t out_bstride, int out_pitch,
                                   wn_stream_t stream);
/* ---- the GENERAL path: shapes the specialised kernels do not cover (filter_width != 2, quantization_channels != 256, more
 * than 64 residual / dilation channels; wavenet/model.py:8-15 takes any).  Its channel-mixing products are wn_chan_gemm /
 * wn_wgrad launches (any row count and K, two taps per launch, more taps accumulate through `resid`); these are the
 * elementwise pieces (music_amd/engine_generic.py sequences them).
 * Gate (model.py:120): z[b][r][t] = tanh(fg[b][r][t]) * sigmoid(fg[b][dp + r][t]) for r < rows, t in [t_lo, t_hi);
 * its derivative: dfg[b][r] = dz sigma(g)(1 - tanh^2 f), dfg[b][dp + r] = dz tanh(f) sigma(g)(1 - sigma(g)). */
int wn_gate_fwd(const float* fg, int64_t fg_bstride, int dp, int rows, float* z, int64_t z_bstride, int pitch, int t_lo, int t_hi,
                int batch, wn_stream_t stream);
int wn_gate_bwd(const float* fg, int64_t fg_bstride, int dp, int rows, const float* dz, int64_t dz_bstride, float* dfg,
                int64_t dfg_bstride, int pitch, int t_lo, int t_hi, int batch, wn_stream_t stream);
/* CHUNK softmax for any row length q (model.py:142-144: the contiguous (B, Q, W) buffer viewed (-1, Q)), its
 * backward dx = y (dy - <dy, y>), and the fused softmax + nn.CrossEntropyLoss-on-the-probabilities step of
 * wn_chunk_softmax256_ce (train.py:146,179) for any q; loss_part has WN_CE_NUM_PARTIALS entries, probs / dx may be NULL. */
int wn_chunk_softmax_fwd(const float* x, float* y, int64_t nrows, int q, wn_stream_t stream);
int wn_chunk_softmax_bwd(const float* y, const float* dy, float* dx, int64_t nrows, int q, wn_stream_t stream);
int wn_chunk_softmax_ce(const float* x, const int64_t* target, float* probs, float* dx, float* loss_part, int64_t nrows, int q,
                        float inv_n, wn_stream_t stream);
/* The operand format of the "x3" products: hi[i] = round16(x[i]), lo[i] = round16(x[i] - hi[i]),
 * 16-bit = IEEE half (is_bf16 = 0) or bfloat16 (1), round to nearest even.  The same device function every MFMA operand
 * of the library is split with; no counterpart in the reference (its products are fp32). */
int wn_split16(const float* x, uint16_t* hi, uint16_t* lo, int64_t n, int is_bf16, wn_stream_t stream);
/* out[b][r][t] = p[b][r][t] (t >= p_lo) + q[b][r][t+dn] (t+dn < t_hi), t in [t_lo,t_hi) */
int wn_shift_add(const float* p, const float* q, float* out, int64_t bstride, int pitch, int rows, int dn, int p_lo,
                 int t_lo, int t_hi, int batch, wn_stream_t stream);

/* Weight gradient: C[m][n] = sum_{b, t in [t_lo,t_hi)} A[b][m][t+a_shift] * B_tap[b][n][t+b_shift_tap]
 * C columns [0, 16*nt_per_tap) come from b0, the next 16*nt_per_tap from b1 (if not NULL).
 * The time axis is cut into chunks; workgroup (clip b, chunk j) writes its partial C (leading
 * dimension ldc) with plain stores into slab number b*nchunks + j at c + slab*c_slab_stride.
 * wn_wgrad_slabs() returns the number of slabs a call writes; wn_reduce_slabs() sums them in slab
 * order (bit-reproducible, no float atomics).  Replaces the weight half of autograd's conv
 * backward (wavenet/train.py:181).
 * Operand values outside the window - columns other than [t_lo + shift, t_hi + shift) of a row - do not enter the result,
 * NaN included (the engines' workspaces hold stale data there); operand columns below 0 read as zero. */
int wn_wgrad(const float* a, int64_t a_bstride, int a_pitch, int a_shift, int a_cols,
             const float* b0, const float* b1, int64_t b_bstride, int b_pitch, int b_shift0,
             int b_shift1, int b_cols, int nt_per_tap, int mt, int relu_b, float* c, int ldc,
             int64_t c_slab_stride, int t_lo, int t_hi, int chunk, int batch, int mode, wn_stream_t stream);
int wn_wgrad_slabs(int t_lo, int t_hi, int chunk, int batch);
/* Weight gradient of the causal layer (autograd of wavenet/model.py:104) when the layer's input is the ONE-HOT tensor
 * wn_onehot built from `codes` (int32 [batch][t]; scrambled as there): dW[r][q][tap] = sum_{b,s} dx[b][r][s] *
 * in[b][q][s-1+tap] becomes a scatter of dx columns - dx (ch rows) is read once, the 4*q*t bytes per clip of dense
 * one-hot are not read at all.  Writes wn_causal_wgrad_codes_slabs(t, batch) slabs [ch][2q] (columns = tap 0 rows |
 * tap 1 rows, the layout wn_wgrad gives the same product); sum them with wn_reduce_slabs.  Bit-reproducible.
 * dx_q != NULL: the data gradient comes as the unshifted pair wn_resblock_bwd_pq writes, dx[s] (s >= p_lo) + dx_q[s + dn]
 * (s + dn < t); the same bits as the plain form on the float32 sum of the pair.
 * s runs over [1, t): dx at column 0 and at columns >= t does not count (NaN included), nor do dx below p_lo and dx_q at
 * columns < 1 + dn or >= t in the pair form.  A code outside [0, q) sets no one (wn_onehot's rule) and contributes nothing.
 * Every element of every slab is written, zeros included (t == 1: the slabs are all zeros); q other than 256: -4, ch other
 * than 32 | 64: -3; t <= 0 or batch <= 0: returns 0 and writes nothing.
 * Arbitrary float inputs (faster_audio_data.py hands the model a dense tensor) keep using wn_wgrad. */
int wn_causal_wgrad_codes(const int32_t* codes, int scrambled, const float* dx, const float* dx_q, int dn, int p_lo,
                          int64_t dx_bstride, int pitch, int ch, int q, int t, int batch, float* slab, wn_stream_t stream);
int wn_causal_wgrad_codes_slabs(int t, int batch);
/* Forward of the causal layer (wavenet/model.py:104) from the same codes, without the one-hot tensor:
 * x0[b][r][s] = bias[r] + sum over the ones (q, s-1) of W[r][q][0] + sum over the ones (q, s) of W[r][q][1], s in [1, t).
 * wt = the layer's weight re-laid as [tap][q][ch] floats (ch contiguous, zero-padded to ch); n_rows = real channel count;
 * bias may be NULL.  Sums of exact fp32 weights in a fixed order (bit-reproducible).
 * Only rows < n_rows x columns [1, t) of every clip are written (the padded rows are NOT touched).  A code outside [0, q)
 * sets no one and contributes nothing; in the scrambled layout a column holds as many ones as the reshape puts there.
 * q other than 256: -4, ch other than 32 | 64: -3; t <= 1 or batch <= 0: returns 0 and writes nothing. */
int wn_causal_fwd_codes(const int32_t* codes, int scrambled, const float* wt, const float* bias, int n_rows, float* x0,
                        int64_t x_bstride, int pitch, int ch, int q, int t, int batch, wn_stream_t stream);
/* desc[op] = {vec_start, slab_off, n_slabs, stride, out_off, n} (int64, device memory):
 * out[out_off+e] = sum_s slab[slab_off + s*stride + e] for e < n; work item v covers 4 floats and
 * belongs to the op with vec_start <= v. */
int wn_reduce_slabs(const int64_t* desc, int n_ops, int64_t total_vec, const float* slab, float* out,
                    wn_stream_t stream);

/* out[row] = sum_{b, t in [t_lo,t_hi)} a[b][row][t+a_shift]  (bias gradients, use_bias=true).
 * Values of a outside the window [t_lo + a_shift, t_hi + a_shift) of a row do not enter the result, NaN included.
 * No clips, rows or columns: returns 0 and writes nothing. */
int wn_bias_grad(const float* a, int64_t a_bstride, int a_pitch, int a_shift, int rows, int t_lo,
                 int t_hi, int batch, float* out, wn_stream_t stream);

/* The reference's chunk softmax: rows of 256 CONSECUTIVE floats of the (B,256,W) buffer
 * (wavenet/model.py:142-144). */
int wn_chunk_softmax256_fwd(const float* x, float* y, int64_t nrows, wn_stream_t stream);
int wn_chunk_softmax256_bwd(const float* y, const float* dy, float* dx, int64_t nrows, wn_stream_t stream);
/* Fused chunk softmax + nn.CrossEntropyLoss applied to the PROBABILITIES (wavenet/train.py:146,179;
 * SURVEY Q1) + both backward steps.  probs/dx may be NULL.  loss_part: WN_CE_NUM_PARTIALS floats,
 * their sum is the mean loss.  A target outside [0, 256) - nn.CrossEntropyLoss raises for it - turns the loss and
 * that row's dx into NaN (no silent wrong value, no host round trip). */
int wn_chunk_softmax256_ce(const float* x, const int64_t* target, float* probs, float* dx,
                           float* loss_part, int64_t nrows, float inv_n, wn_stream_t stream);

/* torch.optim.Adam step on a flat buffer (wavenet/train.py:39-42,182); g is multiplied by gscale. */
int wn_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                 float beta2, float eps, float bias_corr1, float bias_corr2, float gscale,
                 wn_stream_t stream);
/* torch.optim.SGD(params, lr, momentum) / torch.optim.RMSprop(params, lr, momentum) steps on a flat buffer - the other two
 * optimizers wavenet/train.py:28-38 constructs (every further argument at torch's default: no dampening / Nesterov / weight
 * decay; RMSprop not centered, alpha and eps passed in).  g is multiplied by gscale.  SGD: first_step != 0 sets the momentum
 * buffer to the gradient (torch's first step); momentum == 0 needs no buffer (NULL).  RMSprop: momentum_buf may be NULL when
 * momentum == 0. */
int wn_sgd_flat(float* p, const float* g, float* momentum_buf, int64_t n, float lr, float momentum, float gscale,
                int first_step, wn_stream_t stream);
int wn_rmsprop_flat(float* p, const float* g, float* square_avg, float* momentum_buf, int64_t n, float lr, float alpha,
                    float eps, float momentum, float gscale, wn_stream_t stream);
/* ---- Guarded optimizer step (ABI 9): global-norm clipping and the skipping of a non-finite step, decided ON THE DEVICE.
 * Replaces torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) followed by the optimizer's step (wavenet/train.py:28-42,
 * 182 - the reference has neither the clip nor a guard; a NaN gradient there ends the run), with no host read-back between the
 * backward and the update, so a host that runs ahead of the device keeps doing so and every call is legal under stream capture.
 *
 * wn_guard_state: the device-resident block one optimizer owns (WN_GUARD_STATE_BYTES bytes, 8-byte aligned, zeroed by the caller
 * before the first step; wn_grad_guard rewrites the first four fields at every call and advances the rest). */
typedef struct wn_guard_state {
    float norm;          /* L2 norm of gscale * g over the whole buffer at the last call (summed in float64) */
    float coef;          /* factor the guarded update applies to gscale * g: 1, or max_norm / (norm + 1e-6) when that is below 1
                          * (clip_grad_norm_'s rule); NaN when the gradient held a non-finite element or its norm is not finite */
    uint32_t nonfinite;  /* elements of the last gradient for which the float32 value gscale * g is NaN or +-inf */
    uint32_t skip;       /* 1: the guarded update that follows returns without touching anything; else 0 */
    uint64_t n_taken;    /* steps applied so far - Adam's t, and SGD's "first step" is n_taken == 1.  The caller may seed it
                          * (a restored run) while no step is in flight */
    uint64_t n_clipped;  /* of those, steps with coef < 1 */
    uint64_t n_skipped;  /* steps skipped so far */
    float bc1;           /* 1 - beta1^n_taken, in float64 from the device's counter, written at every step taken */
    float bc2;           /* 1 - beta2^n_taken */
} wn_guard_state;
/* One pass over g (n floats, ANY 4-byte aligned address) and the decision, two launches on `stream`, no allocation, no
 * synchronisation, no atomics (the result is a pure function of g, n, gscale, the arguments and the state before):
 *   nonfinite, norm as above; broken = nonfinite > 0 or norm not finite;
 *   skip = skip_nonfinite != 0 and broken;
 *   coef = NaN when broken (an unskipped non-finite step turns the parameters into NaN at once, as the unguarded step does);
 *          else 1 when max_norm <= 0 (no clipping); else min(1, max_norm / (norm + 1e-6));
 *   a skipped step adds 1 to n_skipped and leaves n_taken, n_clipped, bc1, bc2 as they are - Adam's bias correction does not
 *   advance; any other step adds 1 to n_taken, 1 to n_clipped when coef < 1, and rewrites bc1 / bc2 from beta1 / beta2 (pass 0
 *   for an optimizer that has none).
 * partials: WN_GUARD_PARTIALS_BYTES bytes of device scratch, 8-byte aligned.  n == 0 is legal (g may be NULL): norm 0, coef 1, a
 * step taken.  NULL partials / state, or NULL g with n > 0: -4, the argument named in wn_last_error. */
int wn_grad_guard(const float* g, int64_t n, float gscale, float max_norm, int skip_nonfinite, float beta1, float beta2,
                  void* partials, wn_guard_state* state, wn_stream_t stream);
/* wn_adam_flat / wn_sgd_flat / wn_rmsprop_flat after a wn_grad_guard of the same g, n, gscale on the same stream: the same
 * arithmetic with gscale * coef * g as the gradient; with state->skip set they write nothing (parameters, moments and momentum
 * buffers stay bit for bit).  Adam takes its bias corrections from the state block (no bias_corr arguments); SGD's first step -
 * the momentum buffer is SET to the gradient - is the first step TAKEN (state->n_taken == 1; no first_step argument).
 * NULL rules as for the unguarded entries, plus `state`; n == 0 returns 0. */
int wn_adam_flat_guarded(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                         float gscale, const wn_guard_state* state, wn_stream_t stream);
int wn_sgd_flat_guarded(float* p, const float* g, float* momentum_buf, int64_t n, float lr, float momentum, float gscale,
                        const wn_guard_state* state, wn_stream_t stream);
int wn_rmsprop_flat_guarded(float* p, const float* g, float* square_avg, float* momentum_buf, int64_t n, float lr, float alpha,
                            float eps, float momentum, float gscale, const wn_guard_state* state, wn_stream_t stream);
/* EMA shadow of the parameters - the weights every WaveNet recipe samples from (tf.train.ExponentialMovingAverage(decay,
 * num_updates) in the NSynth code; torch.optim.swa_utils.get_ema_avg_fn's lerp rule).  The reference keeps none.  One launch on
 * `stream` behind the optimizer's update: no allocation, no synchronisation, no atomics, legal under stream capture.  Per element,
 * in float32 (an fma may form the sum):
 *   d_eff = warmup ? min(decay, (1 + T) / (10 + T)) : decay     (in double from the float `decay`, rounded once to float)
 *   w = 1.0f - d_eff;   ema[i] = ema[i] + w * (p[i] - ema[i])
 * state == NULL: T = t, the caller's count of updates including this one (t >= 1).
 * state != NULL: the block a wn_grad_guard on the same stream wrote for this step.  With state->skip set nothing is written (the
 *   shadow stays bit for bit); else T = state->n_taken + t, where t is an OFFSET: 0 in a fresh run, set by a host that restored a
 *   run whose device counter was seeded differently (a T below 1 counts as 1).
 * ema and p: n floats each at ANY 4-byte aligned addresses (not necessarily alike); p is never written, nothing outside [0, n) is
 * touched.  n == 0 returns 0 (NULLs allowed).  -4, the argument named in wn_last_error: n < 0; NULL ema or p with n > 0; a
 * misaligned pointer (state: 8 bytes); decay outside [0, 1) or NaN; t < 1 with state == NULL. */
int wn_ema_flat(float* ema, const float* p, int64_t n, float decay, int warmup, int64_t t, const wn_guard_state* state,
                wn_stream_t stream);
/* ---- The PER-TIMESTEP softmax and the true negative log-likelihood: the distribution the decoder samples from (the softmax over the
 * q channels of ONE output column), as an objective.  Nothing of the reference's loss is reproduced here: no second log-softmax
 * (SURVEY Q1), no softmax over time.  x holds logits as [batch][q][x_pitch] with clip stride x_bstride (floats): the
 * channel axis has stride x_pitch, time is contiguous - the layout the epilogue leaves and the backward consumes.  For clip b and
 * column c < w, over the q values x[b * x_bstride + k * x_pitch + c], with y = target[b * w + c]:
 *   m = max_k x_k;  S = sum_k exp(x_k - m);  p_k = exp(x_k - m) / S;  nll = log S + m - x_y
 *   probs[(b * w + c) * q + k] = p_k                    row-major per time step, the shape of the module's output
 *   dx[b * dx_bstride + k * dx_pitch + c] = (p_k - [k == y]) * inv_n
 *   row_nll[b * w + c] = nll;   row_hit[b * w + c] = (the FIRST index of max_k x_k == y)
 *   loss_part: WN_CE_NUM_PARTIALS floats, ALL rewritten at every call; their sum is inv_n * sum of nll over all columns
 * dx, probs, row_nll and row_hit may each be NULL (not wanted).  A target outside [0, q) turns the loss, that column's dx and its
 * row_nll into NaN and its row_hit into 0; other columns are untouched (the rule of wn_chunk_softmax256_ce).  Columns c >= w of a
 * row are never read or written, in x and in dx; any w and any 4-byte aligned bases are valid.  One launch on `stream`: no
 * allocation, no synchronisation, no float atomics (the result is a pure function of the inputs: the same bits at every launch),
 * legal under stream capture.  q == 256 has a kernel of its own; 1 <= q <= 1024.
 * batch == 0 or w == 0: returns 0 and writes nothing, except that wn_step_nll zeroes loss_part when it is given (NULLs allowed).
 * -4, the argument named in wn_last_error: batch < 0 or w < 0; q < 1 or q > 1024; x_pitch < w; x_bstride < q * x_pitch; with dx
 * given, dx_pitch < w or dx_bstride < q * dx_pitch; with work to do, NULL x, target or loss_part (wn_step_softmax: x or probs). */
int wn_step_softmax(const float* x, int64_t x_bstride, int x_pitch, float* probs, int w, int q, int batch, wn_stream_t stream);
int wn_step_nll(const float* x, int64_t x_bstride, int x_pitch, const int64_t* target, float* dx, int64_t dx_bstride, int dx_pitch,
                float* probs, float* row_nll, int32_t* row_hit, float* loss_part, int w, int q, int batch, float inv_n,
                wn_stream_t stream);
/* The WINDOWED objective (ABI 9 still: new entries only): the two entries above under the samplers' position windows ("POSITION-WINDOWED
 * sampling" below states the table and the rule once; this is that rule applied to the softmax, the NLL and its gradient), so that a
 * prior over an interleaved code stream is trained and scored on the distribution wn_win_decode_batch draws from.  Layout, the
 * NULL-able outputs, loss_part, empty calls and refusals are wn_step_nll's / wn_step_softmax's.  win_host: a HOST array of
 * 2 * win_period int32 lo0, hi0, lo1, hi1, .., read during the call (at most 16 pairs, 0 <= lo < hi <= q; it travels in the kernel
 * arguments).  win_pos: a DEVICE array of `batch` int64 (one stream position per clip: a loader's clips start anywhere in a piece), or
 * NULL for zeros.  Column c of clip b sits at stream position p = win_pos0 + win_pos[b] + c and uses pair j = p mod win_period:
 *   - m, S, p_k and nll = log S + m - x_y are taken over k in [lo_j, hi_j) only; row_hit compares the FIRST index of the maximum
 *     inside the window with y.
 *   - Outside the window probs is an exact 0 and dx an exact +0.0; both are written (the backward consumes the whole dx).  What x
 *     holds outside influences nothing - not a NaN, not +inf, not a value far above every logit inside.
 *   - A target inside [0, q) but outside its column's window poisons that column as a target outside [0, q) does (loss, the column's
 *     dx and row_nll NaN, row_hit 0, other columns untouched): a misaligned position is loud, not silently wrong.  A negative
 *     win_pos[b] cannot be refused before the launch: it poisons every column of clip b the same way and is never used as an index.
 *   - win_period == 0 (win_host and win_pos may be NULL): wn_step_nll / wn_step_softmax bit for bit - the same kernel is launched.
 *     A table whose every pair is (0, q) gives those bits too, on every output.
 * -4 before any launch, the entry and the argument named in wn_last_error: win_period < 0 or > 16; win_period > 0 with NULL win_host;
 * a pair with lo < 0, hi > q or lo >= hi; win_pos0 < 0; and everything the entries above refuse. */
int wn_win_step_softmax(const float* x, int64_t x_bstride, int x_pitch, float* probs, int w, int q, int batch, const int32_t* win_host,
                        int win_period, const int64_t* win_pos, int64_t win_pos0, wn_stream_t stream);
int wn_win_step_nll(const float* x, int64_t x_bstride, int x_pitch, const int64_t* target, float* dx, int64_t dx_bstride, int dx_pitch,
                    float* probs, float* row_nll, int32_t* row_hit, float* loss_part, int w, int q, int batch, float inv_n,
                    const int32_t* win_host, int win_period, const int64_t* win_pos, int64_t win_pos0, wn_stream_t stream);
/* The MASKED, WEIGHTED and SMOOTHED objective (ABI 9 still: a new entry only): wn_win_step_nll without inv_n, as a weighted mean over
 * the columns that carry a target - the objective's side of "an absent token contributes nothing" (wn_onehot, the partially forced
 * decode).  Layout, the NULL-able outputs, loss_part and the windows (win_period == 0: none, rows [0, q)) are wn_win_step_nll's.
 *   weight: DEVICE, [batch * w] floats, or NULL for ones.  ignore_index: a target value that marks an absent column.  smoothing: the
 *   label smoothing e in [0, 1).  den: DEVICE, 2 floats, written by the call.
 * Column col = b * w + c, its window [lo, hi) of n = hi - lo rows, y = target[col]:
 *   W = 0 if y == ignore_index, else weight ? weight[col] : 1.
 *   den[0] = sum of W over all columns, accumulated in double in a fixed order by a launch of its own in front of the main kernel on
 *     `stream` (no host read-back); den[1] = (float)(1.0 / that sum), or 0 for a sum of 0.  A counted weight that is negative or not
 *     finite makes both NaN, and with them the loss and the dx of every counted column; it cannot be refused before the launch.
 *   W == 0 exactly: the column is SKIPPED by a predicate, not by a multiply.  Its target is compared with ignore_index and otherwise
 *     has no effect (garbage is fine); its logits reach no arithmetic that leaves the column - NaN, +-inf or 1e30 there change no
 *     output bit elsewhere; its dx is an exact +0.0 in all q rows, its row_nll 0.0, its row_hit 0.  probs is still its softmax.
 *   W != 0, with m, S, p_k as in wn_win_step_nll:
 *     l = log S + m - (1 - e) x_y - (e / n) sum_{k in [lo, hi)} x_k
 *     dx = (W den[1]) (p_k - (1 - e) [k == y] - e / n) inside the window, +0.0 outside
 *     loss_part sums to den[1] * sum of W l;  row_nll is the UNSMOOTHED log S + m - x_y, row_hit as before.
 *     A target outside [0, q) or outside its window poisons the column, a negative win_pos[b] its clip, as in wn_win_step_nll.
 *   smoothing == 0 is a bypass: the sum of x_k is not formed (a -inf logit inside a window gives no 0 * inf).
 *   Every column skipped: the loss is 0, every dx +0.0, den = {0, 0}.
 *   weight == NULL, no target equal to ignore_index, smoothing == 0: every output equals wn_win_step_nll with
 *     inv_n = (float)(1.0 / (double)(batch * w)) bit for bit (with win_period == 0: wn_step_nll).
 * No float atomics, the same bits at every launch; legal under stream capture, allocates and retains nothing.  batch == 0 or w == 0:
 * returns 0 and zeroes loss_part and den where given.  -4, entry and argument named in wn_last_error: everything wn_win_step_nll
 * refuses; smoothing NaN, < 0 or >= 1; with work to do, a NULL den. */
int wn_wstep_nll(const float* x, int64_t x_bstride, int x_pitch, const int64_t* target, float* dx, int64_t dx_bstride, int dx_pitch,
                 float* probs, float* row_nll, int32_t* row_hit, float* loss_part, int w, int q, int batch, const int32_t* win_host,
                 int win_period, const int64_t* win_pos, int64_t win_pos0, const float* weight, int64_t ignore_index, float smoothing,
                 float* den, wn_stream_t stream);
/* ---- LEARNED conditioning projections of the autoencoder: the N + 1 1x1 convs of the pooled encoding enc [batch][bw][le]
 * (wavenet_autoencoder/model1.py:178-179, 216-217 draws them afresh per forward; here they are parameters), read from and
 * differentiated into the flat buffers.  Offsets count floats from `flat` (and from `flat_grad`): stage i < n_stages has its weight
 * [2 dd][bw] at w_off + i * stage_stride and its bias [2 dd] at b_off + i * stage_stride, rows in the reference's order (gate rows
 * [0, dd), filter rows [dd, 2 dd)); the final stage has [sd][bw] at wf_off and [sd] at bf_off.
 *   en_i[b][c][l] = bias_i[c] + sum_k W_i[c][k] enc[b][k][l]        enf[b][c][l] likewise with the final stage, [batch][sd][le]
 * Block tables hold en_i in the layouts the block kernels read, [n_stages][tensors][rows][le], ch = dd padded to 32:
 *   per clip (tab, d_tab with pair = 0):   tensor b,      filter row c -> c - dd,               gate row c -> ch + c,       rows 2 ch
 *   clip pairs (tab_pair, pair = 1):       tensor b >> 1, filter row c -> (b & 1) ch + c - dd,  gate row c -> 2 ch + (b & 1) ch + c,  rows 4 ch
 * wn_cond_proj_fwd writes every table it is given (tab, tab_pair: at least one) WHOLE, padding rows as zeros, and enf, in one launch.
 * wn_cond_proj_bwd takes d_tab in the layout `pair` names and d_enf [batch][sd][le] and writes, in two launches,
 *   d_enc[b][k][l] = sum_i sum_c W_i[c][k] d_en_i[b][c][l] + sum_c W_f[c][k] d_enf[b][c][l]         [batch][bw][le]
 *   flat_grad:  dW_i[c][k] = sum_b sum_l d_en_i[b][c][l] enc[b][k][l],  db_i[c] = sum_b sum_l d_en_i[b][c][l]  (final stage alike)
 * at the parameters' offsets, overwriting; nothing else of flat_grad is touched.  fp32 FMA arithmetic in a fixed order, no atomics:
 * the same bits at every launch.  On `stream`, no allocation, nothing retained.  Any bw, le, dd, sd, n_stages >= 1.
 * batch == 0 returns 0 (NULLs allowed).  -4, function and argument named in wn_last_error: batch < 0; n_stages, dd, sd, bw or le < 1;
 * ch < dd or ch not a multiple of 32; a pair table with an odd batch; a negative offset; stage_stride < 2 dd bw with more than one
 * stage; with work to do, a NULL required pointer. */
int wn_cond_proj_fwd(const float* enc, const float* flat, int64_t w_off, int64_t b_off, int64_t stage_stride, int64_t wf_off,
                     int64_t bf_off, float* tab, float* tab_pair, float* enf, int n_stages, int dd, int ch, int sd, int bw, int le,
                     int batch, wn_stream_t stream);
int wn_cond_proj_bwd(const float* d_tab, int pair, const float* d_enf, const float* enc, const float* flat, int64_t w_off,
                     int64_t b_off, int64_t stage_stride, int64_t wf_off, int64_t bf_off, float* d_enc, float* flat_grad,
                     int n_stages, int dd, int ch, int sd, int bw, int le, int batch, wn_stream_t stream);
/* ---- the same projections with a GLOBAL CLASS term (VQ-VAE's speaker id, NSynth's instrument): clip b has a class cls[b] (int32
 * [batch], on the device) whose embedding row emb[cls[b]] [ge] is projected into every stage, constant over the clip's frames:
 *   en_i[b][c][l] = (bias_i[c] + sum_k W_i[c][k] enc[b][k][l]) + sum_e G_i[c][e] emb[cls[b]][e]           (the final stage alike)
 * - the bracket is wn_cond_proj_fwd's value to the bit, the global product a second reduction added to it.  In flat (flat_grad),
 * counted in floats: stage i's G_i [2 dd][ge] at gw_off + i * gstage_stride, rows in the reference's order like W_i; the final
 * stage's G_f [sd][ge] at gwf_off; the embedding [n_cls][ge] at emb_off.  All other arguments are wn_cond_proj_fwd / _bwd's.
 * wn_gcond_proj_fwd writes every table it is given WHOLE, padding rows as zeros, and enf, in ONE launch.
 * wn_gcond_proj_bwd writes, in THREE launches (wn_cond_proj_bwd's two, the first with dG's tiles behind dW's, and d_emb's),
 *   d_enc, dW_i, db_i:  what wn_cond_proj_bwd writes from the same inputs, the same bits
 *   dG_i[c][e]  = sum_b sum_l d_en_i[b][c][l] emb[cls[b]][e]                                               (the final stage alike)
 *   d_emb[m][e] = sum_{b: cls[b] == m, in ascending b} sum_r G[r][e] (sum_l d[r][b][l])    over all n_stages * 2 dd + sd rows r
 * at the parameters' offsets, OVERWRITING all n_cls rows of d_emb - a class no clip has gets exactly 0; nothing else of flat_grad is
 * touched.  A cls[b] outside [0, n_cls) is never used as an index: the forward turns that clip's columns of every table and of enf
 * into NaN, the backward its share of dG (d_emb has no row for it).  fp32 FMA arithmetic in a fixed order, no float atomics: the
 * same bits at every launch.  On `stream`, no allocation, nothing retained, legal under stream capture.
 * batch == 0 returns 0 (NULLs allowed).  -4, function and argument named in wn_last_error: every case of wn_cond_proj_fwd / _bwd;
 * ge < 1 or ge > WN_GCOND_MAX_CHANNELS; n_cls < 1; a negative gw_off, gwf_off or emb_off; gstage_stride < 2 dd ge with more than one
 * stage; with work to do, a NULL cls. */
#define WN_GCOND_MAX_CHANNELS 512
int wn_gcond_proj_fwd(const float* enc, const float* flat, int64_t w_off, int64_t b_off, int64_t stage_stride, int64_t wf_off,
                      int64_t bf_off, float* tab, float* tab_pair, float* enf, int n_stages, int dd, int ch, int sd, int bw, int le,
                      int batch, const int32_t* cls, int64_t gw_off, int64_t gstage_stride, int64_t gwf_off, int64_t emb_off, int ge,
                      int n_cls, wn_stream_t stream);
int wn_gcond_proj_bwd(const float* d_tab, int pair, const float* d_enf, const float* enc, const float* flat, int64_t w_off,
                      int64_t b_off, int64_t stage_stride, int64_t wf_off, int64_t bf_off, float* d_enc, float* flat_grad,
                      int n_stages, int dd, int ch, int sd, int bw, int le, int batch, const int32_t* cls, int64_t gw_off,
                      int64_t gstage_stride, int64_t gwf_off, int64_t emb_off, int ge, int n_cls, wn_stream_t stream);
/* ---- the GLOBAL CLASS term ALONE: the tables of a class-conditional WaveNet (WaveNet paper section 2.5), which has no encoding.
 * wn_gcond_proj_fwd / _bwd without the bracket and with le = 1: one column per clip, constant over the clip's time.
 *   en_i[b][c] = sum_e G_i[c][e] emb[cls[b]][e]          enf[b][c] likewise with G_f, [batch][sd]
 * G_i, G_f, the embedding, cls, the table layouts (per clip / clip pairs, ch = dd padded to 32, le = 1) and the offsets are
 * wn_gcond_proj_fwd's.  The sums run over e ascending from +0 in fp32 FMA: the bits of wn_gcond_proj_fwd with bw = 1, le = 1 and
 * zero W_i, b_i.
 * wn_gclass_fwd writes every table it is given (tab, tab_pair: at least one) WHOLE, padding rows as exact zeros, and enf, in ONE launch.
 * wn_gclass_bwd takes d_tab in the layout `pair` names and d_enf [batch][sd] and writes, in TWO launches,
 *   dG_i[c][e]  = sum_b d_en_i[b][c] emb[cls[b]][e]        in ascending b                                  (the final stage alike)
 *   d_emb[m][e] = sum_{b: cls[b] == m, in ascending b} sum_r G[r][e] d[r][b]               over all n_stages * 2 dd + sd rows r
 * at the parameters' offsets in flat_grad, OVERWRITING them and all n_cls rows of d_emb - a class no clip has gets exactly 0; nothing
 * else of flat_grad is touched.  A cls[b] outside [0, n_cls) is never used as an index: the forward turns that clip's column of every
 * table and its row of enf into NaN, the backward its share of dG (d_emb has no row for it).  No float atomics, a fixed order: the
 * same bits at every launch.  On `stream`, no allocation, nothing retained, legal under stream capture.
 * batch == 0 returns 0 (NULLs allowed).  -4, function and argument named in wn_last_error: batch < 0; n_stages, dd or sd < 1; ch < dd
 * or ch not a multiple of 32; a pair table with an odd batch; ge < 1 or ge > WN_GCOND_MAX_CHANNELS; n_cls < 1; a negative gw_off,
 * gwf_off or emb_off; gstage_stride < 2 dd ge with more than one stage; with work to do, a NULL required pointer. */
int wn_gclass_fwd(const float* flat, float* tab, float* tab_pair, float* enf, int n_stages, int dd, int ch, int sd, int batch,
                  const int32_t* cls, int64_t gw_off, int64_t gstage_stride, int64_t gwf_off, int64_t emb_off, int ge, int n_cls,
                  wn_stream_t stream);
int wn_gclass_bwd(const float* d_tab, int pair, const float* d_enf, const float* flat, float* flat_grad, int n_stages, int dd, int ch,
                  int sd, int batch, const int32_t* cls, int64_t gw_off, int64_t gstage_stride, int64_t gwf_off, int64_t emb_off, int ge,
                  int n_cls, wn_stream_t stream);
/* ---- the tables of a PHASE-conditioned WaveNet: a prior over a residual-VQ code stream (S stages, frame-major) is told the stage it
 * is at, p mod P of the stream position p, by a learned column per phase instead of a token alphabet of S K.  The model owns
 * T_i [2 dd][period] per block (rows as G_i: gate rows first) at flat + pw_off + i * pstage_stride and T_f [sd][period] at flat + pwf_off
 * (their gradients at the same offsets of flat_grad; offsets count floats).  Clip b's first target sits at stream position pos[b]
 * (device, int64, >= 0).  The block kernels read a table of `period` frames in their tile mode, frame (t - t_lo) mod period of stage i's
 * own t_lo; rot [n_stages + 1] (device, int32, any integer; the last entry is the final stage's) carries each stage's t_lo:
 *   en_i[b][c][l] = T_i[c][(l + pos[b] + rot[i]) mod period]      enf[b][c][l] likewise with T_f and rot[n_stages], [batch][sd][period]
 * the mathematical mod on int64, never negative.  The table layouts are wn_cond_proj_fwd's with le = period: per clip
 * [n_stages][batch][2 ch][period] and / or clip pairs [n_stages][batch/2][4 ch][period], ch = dd padded to 32, rows mapped as documented
 * there.  add_tab / add_pair / add_enf: all NULL, or the class term in the le = 1 layouts of wn_gclass_fwd (its tab, tab_pair, enf; an
 * addend for every output given) - every frame is then the correctly rounded fp32 sum (class column + phase column).
 * wn_phase_tab_fwd writes every table it is given (tab, tab_pair: at least one) WHOLE, padding rows as exact zeros, and enf, in ONE launch.
 * wn_phase_tab_bwd takes d_tab in the layout `pair` names and d_enf [batch][sd][period] and writes, in ONE launch,
 *   dT_i[c][s] = sum_b d_en_i[b][c][(s - pos[b] - rot[i]) mod period]       in ascending b from +0              (the final stage alike)
 * at the tables' offsets in flat_grad, OVERWRITING them; nothing else of flat_grad is touched.  sum_tab / sum_enf: both NULL, or the
 * outputs of the frame sums sum_l d_en_i[b][c][l] (ascending l from +0; every row of the layout, padding included) in the le = 1
 * layouts: sum_tab in the layout `pair` names, sum_enf [batch][sd] - what wn_gclass_bwd takes as its d_tab and d_enf.
 * A negative pos[b] is never used as an index: the forward turns that clip's rows of every table (not the padding) and of enf into NaN,
 * the backward its share of every dT.  fp32 in a fixed order, no float atomics: the same bits at every launch.  On `stream`, no
 * allocation, nothing retained, legal under stream capture.
 * batch == 0 returns 0 (NULLs allowed).  -4, function and argument named in wn_last_error, before any launch: batch < 0; n_stages, dd
 * or sd < 1; period < 1 or > WN_PHASE_MAX_PERIOD; ch < dd or ch not a multiple of 32; a pair table with an odd batch; a negative pw_off
 * or pwf_off; pstage_stride < 2 dd period with more than one stage; with work to do, a NULL required pointer (an addend missing for an
 * output, one of sum_tab / sum_enf without the other). */
#define WN_PHASE_MAX_PERIOD 16
int wn_phase_tab_fwd(const float* flat, int64_t pw_off, int64_t pstage_stride, int64_t pwf_off, const int64_t* pos, const int32_t* rot,
                     const float* add_tab, const float* add_pair, const float* add_enf, float* tab, float* tab_pair, float* enf,
                     int n_stages, int dd, int ch, int sd, int period, int batch, wn_stream_t stream);
int wn_phase_tab_bwd(const float* d_tab, int pair, const float* d_enf, float* flat_grad, int64_t pw_off, int64_t pstage_stride,
                     int64_t pwf_off, const int64_t* pos, const int32_t* rot, float* sum_tab, float* sum_enf, int n_stages, int dd, int ch,
                     int sd, int period, int batch, wn_stream_t stream);
/* ---- VECTOR-QUANTISED bottleneck of the autoencoder (VQ-VAE, van den Oord et al. 2017; the reference has none): every pooled frame
 * e = enc[b][:][l] of enc [batch][bw][le] is replaced by its nearest row of the codebook c [K][bw], which sits at flat + cb_off
 * (its gradient at flat_grad + cb_off; offsets count floats).  C = batch * le frames.  Everything in float32:
 *   dist(b, l, k) = sum_j (e_j - c_kj)^2          the difference form (exact on multiples of 1/8), not |c|^2 - 2 e.c
 *   idx[b][l]     = argmin_k dist, ties to the SMALLEST k;          q[b][:][l] = c[idx[b][l]], the layout of enc
 *   mse           = sum (q - e)^2 / (C bw);       the model's vq_loss = (1 + beta) mse (codebook term + beta x commitment term)
 * wn_vq_fwd writes q_out, idx (int32 [batch][le]), counts (int32 [K], frames per code; may be NULL) and loss_part:
 * WN_VQ_NUM_PARTIALS floats, ALL rewritten at every call, their sum is mse.  One kernel launch (and a memset node for counts).
 * wn_vq_bwd, with s = 2 / (C bw) and g_scale the upstream scalar on vq_loss, writes in one launch
 *   d_enc[b][j][l] = d_q[b][j][l] + g_scale beta s (e - q)          straight-through + commitment; d_enc may alias d_q
 *   flat_grad + cb_off: d_c[k] = g_scale s sum_{frames with idx = k, in ascending frame order} (c_k - e)
 * OVERWRITING all K rows - a code no frame chose gets exactly 0 - and touching nothing else of flat_grad; an idx outside [0, K)
 * turns that frame's d_enc into NaN and is not dereferenced.
 * wn_vq_lookup writes q_out = c[idx] from given codes (decoding): an idx outside [0, K) is never dereferenced - that frame of
 * q_out becomes NaN and *bad (int32 on the device, cleared by the call; may be NULL) becomes 1.
 * On `stream`, no allocation, nothing retained, legal under stream capture; no float atomics and a fixed summation order: the same
 * bits at every launch.  2 <= K <= WN_VQ_MAX_CODES, 1 <= bw <= WN_VQ_MAX_WIDTH, any le >= 1.  batch == 0 returns 0 and writes
 * nothing (NULLs allowed).  -4, function and argument named in wn_last_error, before anything is launched: batch < 0; K < 2 or
 * K > 1024; bw < 1 or bw > 512; le < 1; cb_off < 0; with work to do, a NULL required pointer (all but counts and bad). */
#define WN_VQ_NUM_PARTIALS 256
#define WN_VQ_MAX_CODES 1024                /* = WN_DEC_MAX_Q: what a prior over the codes, wn_step_nll and the samplers accept */
#define WN_VQ_MAX_WIDTH 512
int wn_vq_fwd(const float* enc, const float* flat, int64_t cb_off, float* q_out, int32_t* idx, int32_t* counts, float* loss_part, int K,
              int bw, int le, int batch, wn_stream_t stream);
int wn_vq_bwd(const float* enc, const int32_t* idx, const float* d_q, const float* flat, int64_t cb_off, float beta, float g_scale,
              float* d_enc, float* flat_grad, int K, int bw, int le, int batch, wn_stream_t stream);
int wn_vq_lookup(const int32_t* idx, const float* flat, int64_t cb_off, float* q_out, int32_t* bad, int K, int bw, int le, int batch,
                 wn_stream_t stream);
/* ---- EMA codebook updates for the bottleneck above (van den Oord et al. 2017, appendix A.1) and the restart of dead codes: the codebook
 * follows the running mean of the frames assigned to its rows instead of a gradient.  stat and state share ONE layout, K (bw + 1)
 * floats: K counts, then K rows of bw sums.  stat = [n | s]: n_k the frames with idx = k (as a float), s_k their sum in ascending
 * frame order.  state = [N | m]: running usage and running sums; m / N is the codebook, [1 | c] the initial state.
 * wn_vq_bwd_stats takes the place of wn_vq_bwd, in ONE launch: d_enc exactly as there (the same formula and bits; d_enc may alias
 * d_q; an idx outside [0, K) is compared, never dereferenced, and turns that frame's d_enc into NaN), ALL K (bw + 1) entries of
 * stat, and exactly 0 into all K codebook rows of flat_grad (nothing else of flat_grad is touched): vq_loss = beta mse here.
 * wn_vq_ema_update, with g = decay, updates state and the codebook rows of flat IN PLACE, in two launches:
 *   N'_k = g N_k + (1 - g) n_k      m'_k = g m_k + (1 - g) s_k      tot = sum_k N'_k      Nhat_k = (N'_k + eps) / (tot + K eps) tot
 *   c'_k = m'_k / Nhat_k
 *   restart > 0: the dead codes (N'_k < restart), in ascending index, are paired with the donors (not dead, n_k >= 2 in THIS stat)
 *   in the order of n_k descending, ties to the smaller index; the d-th dead code j takes the d-th donor k: c'_j = m'_j = s_k / n_k
 *   (the donor's batch mean), N'_j = 1; the donor is unchanged; a dead code without a donor stays as the plain update left it.
 * A pure function of stat, state and the scalars: replicas holding the same stat stay bit-identical.  The first launch (one
 * workgroup) reads the old N and stat and writes only `work`, WN_VQ_EMA_WORK_BYTES of device scratch; in the second every
 * workgroup reads and writes only its own codes' rows of state and flat (and reads work and stat).  info (int32[2] on the device,
 * may be NULL): info[0] += the codes restarted by this call, info[1] = the dead codes left without a donor.  guard_state (may be
 * NULL): the wn_guard_state of the wn_grad_guard before it on the stream; with its skip set NOTHING is written - codebook, state
 * and info stay bit for bit.
 * On `stream`, no allocation, no synchronisation, no float atomics, fp32 in a fixed order: the same bits at every launch.  Limits and
 * refusals (-4, function and argument named, before any launch) as for wn_vq_bwd; wn_vq_bwd_stats with batch == 0 returns 0 and
 * writes nothing (NULLs allowed).  wn_vq_ema_update refuses: K < 2 or K > 1024; bw < 1 or bw > 512; cb_off < 0; decay outside
 * (0, 1); eps < 0; restart < 0 (or a NaN for any of the three); NULL flat, stat, state or work; a guard_state off 8-byte alignment. */
#define WN_VQ_EMA_WORK_BYTES 4112
int wn_vq_bwd_stats(const float* enc, const int32_t* idx, const float* d_q, const float* flat, int64_t cb_off, float beta, float g_scale,
                    float* d_enc, float* flat_grad, float* stat, int K, int bw, int le, int batch, wn_stream_t stream);
int wn_vq_ema_update(float* flat, int64_t cb_off, const float* stat, float* state, void* work, int32_t* info, int K, int bw,
                     float decay, float eps, float restart, const wn_guard_state* guard_state, wn_stream_t stream);
/* ---- RESIDUAL vector quantisation of the same bottleneck (SoundStream, EnCodec): S codebooks of K rows, stage s owns rows
 * [s K, (s + 1) K) of the (S K, bw) block at flat + cb_off.  With r_0 = e, for s = 0 .. S-1, everything in float32:
 *   idx_s = argmin_k sum_j (r_s,j - c_s,kj)^2 (wn_vq_fwd's rule: the difference form, ties to the smallest k);   q_s = c_s[idx_s]
 *   r_s+1 = r_s - q_s;          q = (..(q_0 + q_1) + ..) + q_S-1 (ascending, NOT e - r_S: a lookup from the codes gives the same bits)
 *   mse_s = sum (r_s - q_s)^2 / (C bw);          the model's vq_loss = coef sum_s mse_s
 * The frames are independent, so the chain is one launch per direction.  wn_rvq_fwd (one launch and the memset node for counts)
 * writes q_out, idx (int32 [S][batch][le]), counts (int32 [S][K]; may be NULL), res ([S][batch][bw][le], res[s] = r_s+1: the
 * backward reads it) and loss_part ([S][WN_VQ_NUM_PARTIALS], ALL rewritten at every call, row s sums to mse_s).
 * wn_rvq_bwd, one launch, the residual passing between the stages detached (s = 2 / (C bw), g_scale the scalar on vq_loss):
 *   d_enc = d_q + g_scale beta s (r_1 + r_2 + .. + r_S)      the sum in ascending order, then ONE fma onto d_q; d_enc may alias d_q
 *   d_c_s[k] = g_scale s sum_{frames with idx_s = k, ascending} (c_s,k - r_s)      all S K rows overwritten, 0 for an unused row
 * wn_rvq_bwd_stats in its place (EMA mode): the same d_enc, stat = S blocks of [n | sums of r_s] (K (bw + 1) floats each, all
 * written) and exact zeros into all S K codebook rows of flat_grad.  An idx outside [0, K), in any stage, is compared and never
 * dereferenced: that frame's d_enc becomes NaN.
 * wn_rvq_ema_update: wn_vq_ema_update's rule and its two launches for all stages at once (the stage is a second grid dimension), each
 * stage on its own block of stat and state - dead codes and donors are ranked within the stage.  work: S x WN_VQ_EMA_WORK_BYTES,
 * info: int32 [S][2] (may be NULL), guard_state as there.
 * wn_rvq_lookup: q_out = the sum of the first `stages` (1 .. S) stages' rows, in stage order, from idx [stages][batch][le] - a prefix of
 * the stages is the coarser code; an idx outside [0, K) gives a NaN frame and sets *bad (cleared by the call; may be NULL).
 * On `stream`, no allocation, no float atomics, a fixed order: the same bits at every launch, and at S = 1 the bits of the wn_vq_*
 * entry.  Limits and refusals (-4, function and argument named, before any launch) as for wn_vq_*, and: S outside
 * [1, WN_RVQ_MAX_STAGES]; stages outside [1, S]; a NULL res.  batch == 0 returns 0 and writes nothing. */
#define WN_RVQ_MAX_STAGES 8
int wn_rvq_fwd(const float* enc, const float* flat, int64_t cb_off, float* q_out, int32_t* idx, int32_t* counts, float* res,
               float* loss_part, int S, int K, int bw, int le, int batch, wn_stream_t stream);
int wn_rvq_bwd(const float* enc, const int32_t* idx, const float* res, const float* d_q, const float* flat, int64_t cb_off, float beta,
               float g_scale, float* d_enc, float* flat_grad, int S, int K, int bw, int le, int batch, wn_stream_t stream);
int wn_rvq_bwd_stats(const float* enc, const int32_t* idx, const float* res, const float* d_q, const float* flat, int64_t cb_off, float beta,
                     float g_scale, float* d_enc, float* flat_grad, float* stat, int S, int K, int bw, int le, int batch,
                     wn_stream_t stream);
int wn_rvq_ema_update(float* flat, int64_t cb_off, const float* stat, float* state, void* work, int32_t* info, int S, int K, int bw,
                      float decay, float eps, float restart, const wn_guard_state* guard_state, wn_stream_t stream);
int wn_rvq_lookup(const int32_t* idx, const float* flat, int64_t cb_off, float* q_out, int32_t* bad, int S, int stages, int K, int bw,
                  int le, int batch, wn_stream_t stream);
/* ---- QUANTISER DROPOUT for the residual chain (SoundStream, EnCodec, DAC): every clip b has its own stage count n_b, frame fr of
 * clip b is ACTIVE in stage s iff s < n_b.  nstage: `batch` int32 on the device, required; wn_rvq_fwd_n / _bwd_n / _bwd_stats_n clamp
 * a value outside [1, S] to [1, S] before any use (the host validates before it uploads), it is never a bound unchecked.
 * wn_rvq_fwd_n (one launch and the memset node for counts, as wn_rvq_fwd): per frame and stage an active frame gets exactly what
 * wn_rvq_fwd computes; for an inactive one idx_s = -1, the residual and the running q stay as they are (no arithmetic on them),
 * res[s] = the carried r_n_b (no uninitialised floats), and nothing goes into counts[s] or stage s's loss partial.  q_out = the sum of
 * the first n_b winning rows in stage order.  loss_part[s] keeps the FIXED denominator: sum over the ACTIVE frames of the best
 * distance / (C bw), so the model's vq_loss is the batch expectation.  A tile's stage loop ends at the largest n of its frames.
 * wn_rvq_bwd_n / wn_rvq_bwd_stats_n: wn_rvq_bwd / wn_rvq_bwd_stats with
 *   d_enc = d_q + g_scale beta s (r_1 + .. + r_n_b)     the ACTIVE stages, ascending; NaN iff an active stage's idx lies outside [0, K)
 * and d_c_s[k] / stat's [n | sums] over the active frames of stage s alone (idx = -1 matches no code): a stage nobody used gets exact
 * zeros.  Inactive indices are not looked at.  wn_rvq_ema_update takes the stats as they are.
 * wn_rvq_lookup_n: q_out = the sum of the first n_b stages' rows from idx [S][batch][le]; an ACTIVE idx outside [0, K), or an n_b
 * outside [1, S] (NOT clamped here), gives a NaN frame and sets *bad (cleared by the call; may be NULL) - never dereferenced.
 * With every n_b = S every output of the four has the bits of the entry without _n.  On `stream`, no allocation, no float atomics, a
 * fixed order.  Limits and refusals as for wn_rvq_*, and a NULL nstage; batch == 0 returns 0 and writes nothing (NULLs allowed). */
int wn_rvq_fwd_n(const float* enc, const float* flat, int64_t cb_off, const int32_t* nstage, float* q_out, int32_t* idx, int32_t* counts,
                 float* res, float* loss_part, int S, int K, int bw, int le, int batch, wn_stream_t stream);
int wn_rvq_bwd_n(const float* enc, const int32_t* idx, const float* res, const int32_t* nstage, const float* d_q, const float* flat,
                 int64_t cb_off, float beta, float g_scale, float* d_enc, float* flat_grad, int S, int K, int bw, int le, int batch,
                 wn_stream_t stream);
int wn_rvq_bwd_stats_n(const float* enc, const int32_t* idx, const float* res, const int32_t* nstage, const float* d_q, const float* flat,
                       int64_t cb_off, float beta, float g_scale, float* d_enc, float* flat_grad, float* stat, int S, int K, int bw, int le,
                       int batch, wn_stream_t stream);
int wn_rvq_lookup_n(const int32_t* idx, const int32_t* nstage, const float* flat, int64_t cb_off, float* q_out, int32_t* bad, int S, int K,
                    int bw, int le, int batch, wn_stream_t stream);
/* The reference's nn.DataParallel gradient reduction (wavenet/train.py:116-122) as ONE in-place sum over the ranks of the flat
 * fp32 gradient buffer: ncclAllReduce(buf, buf, n, ncclFloat32, ncclSum, comm, stream) on the caller's RCCL communicator
 * (`comm` = an ncclComm_t).  The 1 / world_size of the mean goes into wn_adam_flat's gscale.  Returns -5 when RCCL is neither
 * loaded in the process nor on the loader path (wn_coll_available() == 0), -6 with RCCL's error text when RCCL fails.
 * wn_comm_unique_id / wn_comm_create / wn_comm_destroy are ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy for a host that
 * does not link RCCL itself: rank 0 makes the 128-byte id, every rank gets it by the host's own means and creates its
 * communicator on its current device (collective: returns when all ranks have called). */
int wn_coll_available(void);
int wn_comm_unique_id(char* id128);
int wn_comm_create(int nranks, int rank, const char* id128, void** comm);
int wn_comm_destroy(void* comm);
int wn_allreduce_flat(void* comm, float* buf, int64_t n, wn_stream_t stream);
/* flat_grad[i] = packed[idx[i]] (idx<0 -> 0): dense wgrad results -> state_dict (out,in,k) layout. */
int wn_gather_grads(const float* packed, const int32_t* idx, float* flat_grad, int n, wn_stream_t stream);
/* ... with two sources per element, flat_grad[i] = packed[idx[i]] + packed[idx2[i]] (< 0: nothing): the gradient of a weight
 * that occupies two places of a block-diagonal effective matrix (see z_half_stride of wn_resblock_fwd). */
int wn_gather_grads2(const float* packed, const int32_t* idx, const int32_t* idx2, float* flat_grad, int n, wn_stream_t stream);

/* The conditioning term expanded over time (model1.py:227-247 `_conditon`, both branches): out[b][row][t] =
 * tab[b][row][idx(t)] for t in [t_lo, t_hi), idx as in wn_resblock_fwd (mode 1: (t - t_lo) / q clamped to le - 1, "stretch";
 * mode 2: (t - t_lo) % le, "tile").  What the reference's repeat / index expressions build as a tensor. */
int wn_cond_expand(const float* tab, int64_t tab_bstride, int tab_pitch, int rows, int t_lo, int t_hi, int mode, int le, int q,
                   float* out, int64_t out_bstride, int out_pitch, int batch, wn_stream_t stream);
/* Gradient of the conditioning table: out[b][row][j] = sum over t in [t_lo,t_hi) with idx(t) == j of
 * in[b][row][t]; idx as in wn_resblock_fwd (mode 1 stretch by q, mode 2 tile modulo le)
 * (autograd of wavenet_autoencoder/model1.py:227-247).  Only out[b][row][0 .. le) is written (out_pitch may be larger; what lies
 * behind column le stays).  Values of `in` outside [t_lo, t_hi) do not count and are not read, NaN included.  An empty window
 * (t_hi <= t_lo) with valid pointers writes le zeros per row - the sum over nothing; callers hand in a window, not a promise that
 * it is non-empty.  `in` and `out` are required exactly when something is launched, that is whenever rows, batch and le are all
 * > 0 (NULL: -4, nothing launched); rows, batch or le <= 0 returns 0 and writes nothing.  Refused with -4 and a message, as by
 * wn_cond_expand: a mode outside {1, 2}, q <= 0 under mode 1 (a negative q would start the last bucket in front of the row), and
 * le > 1024.  Under mode 2 q is ignored, whatever its value.  Fixed summation order: the same inputs give the same bits. */
int wn_cond_grad(const float* in, int64_t in_bstride, int in_pitch, int rows, int t_lo, int t_hi, int mode, int le,
                 int q, float* out, int64_t out_bstride, int out_pitch, int batch, wn_stream_t stream);
/* Backward of AvgPool1d: out[b][c][t0 + j*pool + k] = denc[b][c][j] / pool (j < n_out), 0 up to t_hi. */
int wn_avgpool_bwd(const float* denc, int64_t denc_bstride, int denc_pitch, int t0, int pool, int n_out, int rows,
                   float* out, int64_t out_bstride, int out_pitch, int t_hi, int batch, wn_stream_t stream);

/* out[b][c][j] = mean_{k < pool} in[b][c][t0 + j*pool + k], j < n_out  (nn.AvgPool1d,
 * wavenet_autoencoder/model1.py:154-155). */
int wn_avgpool(const float* in, int64_t in_bstride, int in_pitch, int t0, int pool, int n_out, int rows,
               float* out, int64_t out_bstride, int out_pitch, int batch, wn_stream_t stream);

/* One-hot input on device from int32 codes (B,T) -> float32 (B,Q,T).  scrambled=1 reproduces
 * faster_audio_data.one_hot_encode's reshape (wavenet/faster_audio_data.py:77-81);
 * scrambled=0 is the textbook layout fast_generate.py:159-160 builds.  Scrambled: sample s of a clip puts its one at flat offset
 * s*q + code of that clip's q*t floats; textbook: out[b][code][s] = 1.  Every other element of the batch*q*t floats is set to 0,
 * nothing behind them is touched.  A code outside [0, q) sets no one (its sample stays all zero).  batch, q or t <= 0 returns 0 and
 * writes nothing (NULL pointers accepted). */
int wn_onehot(const int32_t* codes, float* out, int batch, int q, int t, int scrambled, wn_stream_t stream);

/* mu-law (wavenet/audio_func.py:5-39): encode through the 255-entry float32 threshold table of the
 * canonical encoder (bit-exact); decode through the 256-entry table. */
int wn_mulaw_encode_tbl(const float* audio, const float* thresholds, uint8_t* codes, int64_t n, wn_stream_t stream);
int wn_mulaw_decode_lut(const uint8_t* codes, const float* table, float* audio, int64_t n, wn_stream_t stream);
/* The same for any number q >= 2 of quantisation channels (the argument of audio_func.py:5,24): q - 1 ascending float32
 * thresholds (code = number of thresholds <= the sample), a q-entry decode table (codes clamped to [0, q)), int32 codes. */
int wn_mulaw_encode_q(const float* audio, const float* thresholds, int q, int32_t* codes, int64_t n, wn_stream_t stream);
int wn_mulaw_decode_q(const int32_t* codes, const float* table, int q, float* audio, int64_t n, wn_stream_t stream);

/* Cached-queue greedy decode, n_steps samples in one persistent launch
 * (wavenet/fast_generate.py:66-141 per sample; :166-172 loop).  All weights fp32 in "decode
 * layout" (music_amd/fast_generate.py builds it): w_causal [R][2Q] (k = tap0 q | tap1 q);
 * per block at w_layers + i*layer_stride: Wfg [2D][2R] (rows f then g; k = tap1 r | tap0 r),
 * Wd [R][D], Ws [S][D]; b_layers per block [bf D | bg D | bd R | bs S] or NULL; w_p1 [S][S],
 * w_p2 [Q][S].  queues: block i's FIFO as a ring [d_i][R] (time-major) at float offset q_off[i];
 * at global step g the column at slot g % d_i is the oldest, is consumed, then overwritten with
 * the block OUTPUT (as written in the reference) or its INPUT (push_input != 0).
 * note0 / prev0: dense [Q] current and previous input columns; forced: teacher-forced next codes
 * (NULL = feed back the argmax).  codes_out[n_steps] = argmax of the probabilities (first index on
 * ties); probs_out optional.  dilations_host / q_off_host are HOST arrays.
 * PARTIALLY FORCED DECODE - the rule of `forced`, here and in every decode entry below that takes it, per utterance u and
 * step s: forced[u][s] >= 0: the input column after step s is the one-hot of that code (teacher forcing; the entry must be
 * < Q).  forced[u][s] < 0: the step is FREE - the input column is the code the launch chose at step s, exactly as with
 * forced == NULL.  Nothing else depends on the entry: codes_out[u][s] and probs_out[u][s] are the model's own pick and
 * distribution at every step, forced or free (the likelihood of kept tokens is read from probs_out); the uniform number of
 * step s is that of global step step0 + s whether s is forced or free, so a stream's draws do not move with the mask; the
 * window, top-k, top-p and guidance rules are untouched (under guidance the two members of a pair carry EQUAL forced rows -
 * the fp32 kernel reads row 2j's - and a free step feeds the pair's one code to both).  A launch with forced == NULL, or
 * without a negative entry, computes what it computed before this rule was written down, bit for bit.
 * sync: optional device scratch of (n_layers*D + 2) uint64, used by the two-workgroup matrix-core form
 * (wn_decode_batch_pk; hand-offs through tagged 8-byte granules, the last word is an error flag: non-zero = a
 * bounded spin timed out).  wn_decode / wn_decode_batch run one workgroup of fp32 FMAs per utterance
 * (any channel counts, with or without biases) and ignore it. */
int wn_decode(int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host, const int64_t* q_off_host,
              float* queues, const float* w_causal, const float* b_causal, const float* w_layers,
              int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
              const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
              float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
              int n_steps, int push_input, uint64_t* sync, wn_stream_t stream);

/* The same loop for n_utt (<= 128) INDEPENDENT utterances side by side in one launch (batched
 * utterances; the reference generates one at a time): weights shared, everything else per utterance with
 * utterance u at queues + u*queues_ustride, note0/prev0/note_out/prev_out + u*Q, forced/codes_out +
 * u*n_steps, probs_out + u*n_steps*Q, sync + u*(n_layers*D + 2).  All utterances share step0 / n_steps.
 * forced: wn_decode's rule, per utterance and step (a negative entry frees that step of that utterance only); it holds for
 * every batched entry below (_pk, _fw, _cond, _samp, wn_win_decode_batch, wn_cfg_decode_batch).
 * temperature > 0: SAMPLE each code from softmax(logits / temperature) (inverse CDF, uniform numbers from
 * a counter-based generator keyed by (seed, step0 + step, u): reproducible); <= 0: greedy argmax. */
int wn_decode_batch(int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host, const int64_t* q_off_host,
                    float* queues, const float* w_causal, const float* b_causal, const float* w_layers,
                    int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                    const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                    float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                    int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                    uint64_t seed, wn_stream_t stream);
/* wn_decode_batch with the chain's products on the matrix cores: pk = the packed f16 hi/lo weight fragments of the
 * forward blocks (wn_pack_weights, mode WN_F16X3: per block l "fg" at pk + pk_fg0 + l*pk_lstride halfs in natural k
 * order, "d" at pk + pk_d0 + l*pk_lstride in chained k order, as wn_resblock_fwd takes them; pk_skip / pk_p1 / pk_p2 >= 0:
 * the skip product and the two post-processing products as well (S = 256 or 512, Q = 256), else -1).  Used when R = D = 64,
 * S = 256 or 512 and Q = 256 with all of pk given (biases allowed); NULL or other shapes = wn_decode_batch.  A model with
 * FEWER residual / dilation channels (the reference's shipped 32 / 32 / 512) runs here as the 64 / 64 model it is with zero
 * rows and columns: the decoder is bound by latency, not by traffic, so the padding is free (music_amd/fast_generate.py
 * hands over padded weights, packs and 64-wide queue columns).
 * sync here holds wn_decode_sync_granules(n_layers, D, S) uint64 PER UTTERANCE (error flag = the last word of an
 * utterance's region).  Eight utterances share a workgroup pair, one pair of MFMA result columns each (n_utt <= 1024
 * on this path; when fewer than eight are left for a pair the spare columns mirror the last utterance; same arithmetic
 * per utterance, so rows are bit-identical whatever the batch).
 * With 512 skip channels (and room: at most 24 pairs per launch, else the form above) the skip sum and the post-processing of a
 * pair are split over S / 64 workgroups, one 16-row tile per wave, their post-processing tiles register-resident, the
 * S-vectors exchanged as tagged granules through the hand-off area (decode): same sums per row, same codes.
 * Models deeper than 31 blocks keep the tap-0 partial sums of a sample in the pair's hand-off area instead of LDS. */
int64_t wn_decode_sync_granules(int n_layers, int D, int S);
int wn_decode_batch_pk(int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host, const int64_t* q_off_host,
                       float* queues, const float* w_causal, const float* b_causal, const float* w_layers,
                       int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                       const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                       float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                       int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                       uint64_t seed, const uint16_t* pk, int64_t pk_fg0, int64_t pk_d0, int64_t pk_lstride, int64_t pk_skip,
                       int64_t pk_p1, int64_t pk_p2, wn_stream_t stream);
/* wn_decode_batch_pk for any filter width k = filter_width >= 1 (ABI 6).  Block i reads its input at t, t - d_i, ..,
 * t - (k-1) d_i: its queue is a ring of L_i = (k-1) d_i columns [L_i][R] (time-major) at float offset q_off[i]; at global
 * step g tap j (0 <= j <= k-2) reads slot (g + j d_i) mod L_i, and slot g mod L_i - the oldest, tap 0 - is then overwritten
 * with the block's INPUT (k = 1: no rings).  The causal layer keeps k - 1 previous input columns: prev0 / prev_out hold
 * (k-1) * Q floats per utterance, oldest column first (utterance u at + u*(k-1)*Q; may be NULL when k = 1).  fp32 weights:
 * w_causal [R][kQ] (k = tap 0 q | tap 1 q | .. | tap k-1 q); per block Wfg [2D][kR] with k = tap k-1 r (current input) |
 * tap k-2 r | .. | tap 0 r, then Wd [R][D], Ws [S][D] at layer_stride floats per block.  Any Q from 1 to 1024 (probs_out
 * rows hold Q floats).  k = 2 is wn_decode_batch_pk, same results.  The matrix-core kernels serve k = 2, 3 and 4 (pk with
 * fg fragments [2 x 64][64 k] per block in natural k order; k = 3 / 4 need the tap-0-ahead form); other widths run the
 * fp32 kernel and ignore pk.  Returns -4 (wn_last_error says why) for filter_width < 1, push_input = 0 with
 * k != 2 (the as-written recurrence is only defined for k = 2), NULL required pointers, and a layout that does not fit
 * the kernel's LDS. */
int wn_decode_batch_fw(int filter_width, int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host,
                       const int64_t* q_off_host, float* queues, const float* w_causal, const float* b_causal,
                       const float* w_layers, int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                       const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                       float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                       int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                       uint64_t seed, const uint16_t* pk, int64_t pk_fg0, int64_t pk_d0, int64_t pk_lstride, int64_t pk_skip,
                       int64_t pk_p1, int64_t pk_p2, wn_stream_t stream);

/* wn_decode_batch_fw with a PER-UTTERANCE, TIME-VARYING conditioning table under every block's [f; g] and under
 * post_process_1's output (ABI 7): the autoencoder's decoder (wavenet_autoencoder/model1.py:158-247) as a cached-queue
 * recurrence, so an encoding of any number of pooled frames can be decoded, and the utterances of a launch decode
 * different encodings.  cond_fg: float [n_utt][n_layers][le][2D] (utterance u at + u*cond_fg_ustride), rows f then g - the
 * decode layout, the reference's "gate = first half" order is swapped by the caller; cond_p1: float [n_utt][le][S]
 * (+ u*cond_p1_ustride).  The tables stay in global memory, le is not capped.
 * The SCHEDULE (host arrays of n_layers + 1 ints, blocks first, post-processing last; shared by the launch) says which
 * column a stage reads: step s of the launch is output position j = pos0 + s, stage i's column is c = j + c_shift[i]
 * (c_shift[i] = L_{i+1} - W: length of the stage's output in the forward over the whole clip minus the forward's output
 * width) and its table column is  c / c_q[i]  when c_q[i] > 0 (the stretch branch of _conditon),  c mod le  when c_q[i] == 0
 * (the tile branch).  c < 0 reads column 0 (pos0 may be negative: priming steps before the first output position); a
 * stretch column past the end reads the last one, le - 1; the tile branch is periodic and has no end.
 * Either table may be NULL (that stage is then unconditioned); with both NULL the call is wn_decode_batch_fw bit for bit.
 * The fp32 kernel serves every shape it serves unconditioned; the matrix-core kernels serve the tap-0-ahead forms (filter
 * widths 2, 3, 4; 256 or 512 skip channels, one-workgroup and split skip stage): the f / g term of sample t + 1 is added
 * to the tap-0 partial sums in the sample-ahead pass, the cond_p1 column is staged per sample by the skip workgroups while
 * they wait for the chain.  A launch the matrix-core kernels do not serve conditioned (tap-0-ahead switched off) runs the
 * fp32 kernel; nothing is ever decoded silently unconditioned.
 * Returns -4 (wn_last_error says why) for le < 1, a NULL schedule array with a non-NULL table, c_q[i] < 0, push_input == 0
 * (conditioned decode exists for the corrected recurrence only) and everything wn_decode_batch_fw refuses. */
int wn_decode_batch_cond(int filter_width, int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host,
                         const int64_t* q_off_host, float* queues, const float* w_causal, const float* b_causal,
                         const float* w_layers, int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                         const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                         float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                         int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                         uint64_t seed, const uint16_t* pk, int64_t pk_fg0, int64_t pk_d0, int64_t pk_lstride, int64_t pk_skip,
                         int64_t pk_p1, int64_t pk_p2, const float* cond_fg, int64_t cond_fg_ustride, const float* cond_p1,
                         int64_t cond_p1_ustride, const int32_t* c_shift_host, const int32_t* c_q_host, int le, int64_t pos0,
                         wn_stream_t stream);

/* Sampling settings of one utterance of a decode launch, or of one row of wn_sample_logits (ABI 8), 24 bytes.
 * temperature <= 0: greedy first-index argmax (the filters are ignored).  top_k <= 0 or >= Q: no top-k filter; top_p <= 0 or
 * >= 1: no nucleus filter.  The uniform number of step s is dec_uniform(seed, s, stream) (splitmix64 finaliser, 24 bits). */
typedef struct { float temperature; float top_p; int32_t top_k; uint32_t stream; uint64_t seed; } wn_sampling;

/* wn_decode_batch_cond with TRUNCATED sampling and PER-UTTERANCE settings (ABI 8).  The rule, per row of Q logits l with
 * temperature T > 0 and a uniform number u in [0, 1), is decided on the LOGITS, so the kept set is exact:
 *   1. top-k (0 < top_k < Q): K = { i : l_i >= the top_k-th largest logit } - ties at the boundary are kept; else K = all.
 *   2. p_i = exp((l_i - max l) / T) / sum over K on K, 0 elsewhere.
 *   3. top-p (0 < top_p < 1): tau = the largest logit value v in K with sum_{K, l_i >= v} p_i >= top_p, N = { i in K :
 *      l_i >= tau } (ties kept); else N = K.
 *   4. r = p / sum over N on N, 0 elsewhere: probs_out receives r (exact zeros outside N); the code is the first index whose
 *      inclusive cumulative r exceeds u, and the LARGEST INDEX IN N when none does (u above the rounded total).
 *   5. T <= 0: greedy first-index argmax, probs_out is the plain softmax.
 * samp == NULL: the scalar temperature / seed / top_k / top_p apply to every utterance and utterance u draws from stream u;
 * with top_k = 0 and top_p = 1 that is wn_decode_batch_cond bit for bit.  samp != NULL: a DEVICE array [n_utt]; utterance
 * u takes everything from samp[u] (read once, before the first sample) and the scalars are ignored.  Row u of a launch with
 * a table equals the single-utterance launch with samp[u] - bit for bit when both run the same kernel form (at 256 skip
 * channels one pair's skip stage is split over four workgroups by default, several pairs' are not, and the two forms round
 * the logits differently: WN_DEC_KS holds the form fixed).
 * Returns -4 (wn_last_error names the argument) for a scalar top_p that is NaN or negative, a scalar top_k < 0, and
 * everything wn_decode_batch_cond refuses. */
int wn_decode_batch_samp(int filter_width, int n_layers, int R, int D, int S, int Q, const int32_t* dilations_host,
                         const int64_t* q_off_host, float* queues, const float* w_causal, const float* b_causal,
                         const float* w_layers, int64_t layer_stride, const float* b_layers, const float* w_p1, const float* b_p1,
                         const float* w_p2, const float* b_p2, const float* note0, const float* prev0, float* note_out,
                         float* prev_out, const int32_t* forced, int32_t* codes_out, float* probs_out, int64_t step0,
                         int n_steps, int push_input, uint64_t* sync, int n_utt, int64_t queues_ustride, float temperature,
                         uint64_t seed, const uint16_t* pk, int64_t pk_fg0, int64_t pk_d0, int64_t pk_lstride, int64_t pk_skip,
                         int64_t pk_p1, int64_t pk_p2, const float* cond_fg, int64_t cond_fg_ustride, const float* cond_p1,
                         int64_t cond_p1_ustride, const int32_t* c_shift_host, const int32_t* c_q_host, int le, int64_t pos0,
                         const wn_sampling* samp, int top_k, float top_p, wn_stream_t stream);

/* The decoder's sampler (the same device function) on a logits matrix: row i of logits [n][Q] (row stride ld >= Q floats)
 * is "step" step0 + i.  samp: optional DEVICE table [n], one entry per row; NULL: the scalars apply to every row and the
 * stream id is 0.  u: optional DEVICE array [n] of explicit uniform numbers in [0, 1) that replace the generated ones.
 * codes [n] receives the codes, probs [n][Q] (optional) the distribution drawn from.  1 <= Q <= 1024; n == 0 launches
 * nothing.  Returns -4 for Q out of range, n < 0, ld < Q, NULL logits / codes, and a scalar top_p / top_k as above. */
int wn_sample_logits(const float* logits, int64_t n, int Q, int64_t ld, const wn_sampling* samp, float temperature, uint64_t seed,
                     int top_k, float top_p, int64_t step0, const float* u, int32_t* codes, float* probs, wn_stream_t stream);

/* POSITION-WINDOWED sampling (ABI 9 still: new entries only).  A code stream that interleaves several alphabets - the residual
 * quantiser's frame-major stream l0s0, l0s1, .., l1s0, .. with token = s K + code - allows at stream position p only the tokens
 * of stage p mod S.  A launch carries a WINDOW TABLE of `period` pairs (lo_j, hi_j), 0 <= lo_j < hi_j <= Q, and a position
 * win_pos0 >= 0; step s of the launch (row s of a logits matrix) uses pair j = (win_pos0 + s) mod period.  The rule:
 *   - The window is applied FIRST: the row is the hi - lo logits l[lo .. hi), and steps 1-5 of wn_decode_batch_samp's rule apply
 *     to it as if Q were hi - lo.  The maximum, every sum, the top-k count, the nucleus search and the smallest real key are taken
 *     over the window only; top_k >= hi - lo means no top-k filter AT THAT POSITION (widths may differ between positions).
 *   - Entries outside the window are never part of the result: their probability in probs_out is an exact 0 and their values
 *     influence nothing - not a NaN, not a value far above every logit inside.
 *   - Codes are reported in the full alphabet, lo + index.  Greedy (temperature <= 0) is the first-index argmax inside the window,
 *     its probs_out the plain softmax over the window.
 *   - The code lies in [lo, hi) whatever the logits hold: with u above the rounded total it is the largest index of the kept set
 *     inside the window (hi - 1 without filters); on a row whose logits inside the window are all -inf or NaN the probabilities
 *     are unspecified and the code is still inside the window (greedy: lo).
 *   - period == 0 (win_host may be NULL): no table, the launch is wn_decode_batch_samp / wn_sample_logits bit for bit; so is a
 *     table whose every pair is (0, Q) - the window is the validity predicate lo <= i < hi where those test i < Q.
 * The table travels in the kernel arguments (at most 16 pairs), shared by the utterances of a launch.
 *
 * wn_win_decode_batch: wn_decode_batch_samp's arguments up to top_p, then win_host - a HOST array of 2 * win_period int32
 * lo0, hi0, lo1, hi1, .., read during the call - win_period and win_pos0.  A teacher-forced step still reports the windowed
 * code and probabilities.  Returns -4 (wn_last_error names the entry and the argument) before any launch for win_period < 0 or
 * > 16, win_period > 0 with NULL win_host, a pair with lo < 0, hi > Q or lo >= hi, win_pos0 < 0, and everything
 * wn_decode_batch_samp refuses (so: the corrected recurrence only).  n_steps == 0 or n_utt == 0 launch nothing and return 0. */
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
                        int64_t win_pos0, wn_stream_t stream);
/* wn_sample_logits under a window table: row i uses pair (win_pos0 + i) mod win_period (independent of step0, which still
 * numbers the generated uniforms).  Same refusals for the three new arguments, plus everything wn_sample_logits refuses; n == 0
 * launches nothing. */
int wn_win_sample_logits(const float* logits, int64_t n, int Q, int64_t ld, const wn_sampling* samp, float temperature, uint64_t seed,
                         int top_k, float top_p, int64_t step0, const float* u, int32_t* codes, float* probs,
                         const int32_t* win_host, int win_period, int64_t win_pos0, wn_stream_t stream);

/* CLASSIFIER-FREE GUIDANCE (ABI 9 still: new entries only).  A model trained with its class dropped for a share of the clips is
 * sampled from an extrapolation of its unconditional logits l_u towards its conditional ones l_c (Ho & Salimans 2021).  A launch
 * carries a GUIDANCE TABLE, a DEVICE array of n_utt / 2 floats, and its rows are PAIRS: row 2j is the conditional member, row
 * 2j + 1 the unconditional one, guidance[j] the pair's scale s.  Each member runs the recurrence on its own rings and its own
 * conditioning tables exactly as in wn_win_decode_batch; only the choice changes.  The rule:
 *   - Combination: g_i = l_c,i + (s - 1) (l_c,i - l_u,i), element by element in fp32 (the difference rounded, then one fused
 *     multiply-add).  s = 1 is the conditional model, s > 1 more of the class, s = 0 the unconditional model.
 *   - s == 1 is a bypass: g IS l_c, bit for bit, whatever l_u holds - NaN and inf included.
 *   - The pick runs ONCE, on g, by the rule above: window first, then top-k, temperature, top-p, draw.  It uses row 2j's sampling
 *     settings, stream id and uniform number; row 2j + 1's wn_sampling entry is ignored.  An entry outside the step's window
 *     influences nothing, in either matrix.
 *   - Feedback: the ONE code is the next input of both members and goes to both codes_out rows; both members therefore see the
 *     same input history and their note_out / prev_out rows are equal.  probs_out row 2j receives the distribution drawn from
 *     (of g) and row 2j + 1 the same values: no row is left unwritten.
 *   - forced, note0 and prev0 stay per row and the caller passes EQUAL rows for the two members of a pair (the fp32 kernel, which
 *     runs both members of a pair in one workgroup, reads row 2j's).  A negative forced entry (wn_decode's rule) frees the step for
 *     the pair: its one code is fed to both members.
 *   - guidance == NULL: no table, the launch is wn_win_decode_batch / wn_win_sample_logits bit for bit.
 * The per-launch limits stay per row: 1024 rows on the matrix-core path (512 guided streams), 128 on the fp32 kernel (64).
 *
 * wn_cfg_decode_batch: wn_win_decode_batch's arguments up to win_pos0, then guidance.  Returns -4 (wn_last_error names the entry
 * and the argument) before any launch for a non-NULL guidance with odd n_utt, a non-NULL guidance without conditioning tables
 * (cond_fg and cond_p1 both NULL), and everything wn_win_decode_batch refuses. */
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
                        int64_t win_pos0, const float* guidance, wn_stream_t stream);
/* The guided sampler alone (the decode kernels' device function): wn_win_sample_logits' arguments up to win_pos0 with logits_c in
 * the place of logits, then logits_u [n][Q] (row stride ld too) and guidance [n], DEVICE arrays - row i is picked from the
 * combination of the two matrices' rows i under guidance[i], with row i's settings.  guidance == NULL is wn_win_sample_logits on
 * logits_c (logits_u is not read); a non-NULL guidance with NULL logits_u is refused like every missing pointer (-4, by name).  Everything
 * wn_win_sample_logits refuses is refused under this entry's name. */
int wn_cfg_sample_logits(const float* logits_c, int64_t n, int Q, int64_t ld, const wn_sampling* samp, float temperature, uint64_t seed,
                         int top_k, float top_p, int64_t step0, const float* u, int32_t* codes, float* probs,
                         const int32_t* win_host, int win_period, int64_t win_pos0, const float* logits_u, const float* guidance,
                         wn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
