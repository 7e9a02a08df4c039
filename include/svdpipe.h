/* svdpipe.h – C ABI of libsvdpipe_hip.so, the MI355X (gfx950) kernel library under the
 * per-step SVD UNet hot path.
 *
 * The reference (inai17ibar/video-diffusion-pipeline-parallel) defines NO FFI: its hot path is the
 * Python call `latent = self.model(latent, step)` (/root/reference/src/pipeline/pipeline.py:95)
 * -> `StableVideoUNet.forward` (/root/reference/src/models/svd_unet.py:351-439)
 * -> `self.unet(sample=..., timestep=..., encoder_hidden_states=..., added_time_ids=...)`
 *    (svd_unet.py:389,400,416), where `unet` is diffusers' UNetSpatioTemporalConditionModel running
 *    on cuDNN/cuBLAS/xformers.  The entry points below are what a binding for that path binds
 *    instead of those vendor libraries; each comment names the diffusers/torch op it replaces and
 *    the reference line that reaches it.  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes; `stream` is a hipStream_t passed as void* (NULL = default stream)
 *   - device pointers are owned by the caller (PyTorch allocator); the library never allocates,
 *     frees or synchronises; every call only enqueues kernels on `stream`
 *   - return 0 on success, negative SP_E* on a rejected argument (nothing is launched);
 *     sp_last_error() returns a thread-local message
 *   - activations are fp16, channels-last: a "token matrix" [rows][C] where rows enumerate
 *     (frame, y, x) in that order (NHWC per frame); weights are fp16 [N][K] (K contiguous);
 *     biases / norm affine parameters are fp32
 *   - gfx950 code objects only
 */
#ifndef SVDPIPE_H
#define SVDPIPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_OK 0
#define SP_EINVAL (-1)   /* bad argument / unsupported shape */
#define SP_ELAUNCH (-2)  /* hipLaunchKernel reported an error */

const char *sp_last_error(void);
int sp_version(void);
/* bytes of zero-filled device memory every gather kernel needs behind `zero_page` */
#define SP_ZERO_PAGE_BYTES 4096

/* ---------------------------------------------------------------------------------------------
 * Implicit-GEMM family:  D[M][Nout] = epilogue( sum_{tap,k} A_tap[m][k] * W[n][tap*Cin + k] )
 * Replaces torch.nn.functional.conv2d (ResnetBlock2D conv1/conv2, Downsample2D, Upsample2D conv,
 * conv_in/conv_out), conv3d with kernel (3,1,1) (TemporalResnetBlock), 1x1 shortcut convs and every
 * nn.Linear of the transformer blocks – i.e. cuDNN/cuBLAS under svd_unet.py:416.
 * MFMA fp16 -> fp32 accumulate; A tiles are gathered straight from the NHWC tensor into LDS
 * (no im2col buffer).
 * ------------------------------------------------------------------------------------------- */
enum { SP_A_LINEAR = 0, SP_A_CONV3X3 = 1, SP_A_TEMPORAL3 = 2 };

typedef struct sp_gemm_desc {
  /* A operand */
  const void *a;        /* fp16 [rows_in][lda] */
  int64_t lda;          /* elements between consecutive A rows (>= cin, a multiple of 8) */
  int mode;             /* SP_A_* */
  int cin;              /* channels per tap (multiple of 64); K = taps*cin */
  /* geometry for SP_A_CONV3X3: input images [n_img][hin][win], output [n_img][hout][wout];
     pad 1; stride 1 or 2; upsample2x!=0 reads the input through a nearest-neighbour x2 upsample */
  int n_img, hin, win, hout, wout, stride, upsample2x;
  /* geometry for SP_A_TEMPORAL3: rows = [batch][frames][hw]; taps are frames f-1, f, f+1 */
  int frames; int64_t hw;
  /* B operand */
  const void *w;        /* fp16 [n][taps*cin]; for geglu the rows are pre-interleaved in blocks of 16 */
  int m, n;             /* GEMM M (output rows) and N (weight rows; multiple of 64) */
  /* epilogue: v = oscale*(acc + bias[n] + bias2[(m/bias2_rows)][n]) + r1scale*res1 + r2scale*res2
     geglu!=0: out[m][j] = h*gelu(gate) over the interleaved column pairs, Nout = n/2
     (bias applies before gelu; oscale/res are applied to the product) */
  const float *bias;    /* [n] or NULL */
  const float *bias2;   /* [nb][ldb2] or NULL */
  int64_t bias2_rows;   /* rows of D sharing one bias2 row (e.g. frames*H*W of a batch item); 0 = one row for all m */
  int64_t ldb2;         /* floats between bias2 rows: 0 (= n), or >= n and a multiple of 4 */
  const void *res1; int64_t ldr1; float r1scale;   /* fp16 [m][ldr1] or NULL; ldr1 >= stored columns, a multiple of 8 */
  const void *res2; int64_t ldr2; float r2scale;   /* the same */
  float oscale;
  int geglu;            /* needs n a multiple of 128 */
  int n_store;          /* number of leading output columns actually stored (0 <= n_store <= Nout); 0 = all */
  void *d; int64_t ldd; /* fp16 [m][ldd]; ldd >= stored columns (n_store, or Nout), a multiple of 8 -- with 0 < n_store < 8
                           any such pitch (conv_out stores rows of 4) */
  const void *zero_page;
  /* Every rule of this descriptor is checked before anything is launched (SP_EINVAL, sp_last_error() names the field):
     a, w, d, zero_page non-NULL; m, n > 0; the multiples and minimum row pitches above; SP_A_CONV3X3: stride 1 or 2,
     positive geometry, hout / wout = ((hin / win, doubled with upsample2x) + 2 - 3) / stride + 1, m == n_img*hout*wout;
     SP_A_TEMPORAL3: frames, hw > 0, m a multiple of frames*hw.  Buffers are not known to the library: a, w, d, res1, res2 and
     a2 must be 16-byte aligned (d with 0 < n_store < 8: 2-byte), bias / bias2 / ln_colsum 16-byte aligned. */
  /* LayerNorm folded into this contraction (SP_A_LINEAR only, bias2 must be NULL): with W pre-multiplied by the norm's
     gamma, LN(x).W^T + b = rstd[m]*(x.W'^T - mean[m]*ln_colsum[n]) + bias[n], so the normalised tensor is never
     written: ln_stats = fp32 [m][2] (mean, rstd) from sp_ln_stats_f16, ln_colsum[n] = sum_k W'[n][k] (of the fp16
     values), bias[n] = W.beta + b.  NULL = no fold; ln_stats and ln_colsum come together (one without the other is
     refused). */
  const float *ln_stats;
  const float *ln_colsum;
  /* Guidance mix + Euler update folded into the epilogue of the UNet's last convolution (conv_out: n = 64 padded
     weight rows of which 4 are real; /root/reference/src/models/svd_unet.py:410-439).  euler_out != NULL: instead of
     storing eps rows in d, row m = (b, f, pixel) updates the four latent channels
       eps = euler_eps_uncond ? u + g[f]*(eps - u) (evaluated in fp16 like the reference) : eps
       x0 = eps*(-sigma/sqrt(sigma^2+1)) + x/(sigma^2+1);  x' = x + (x - x0)/sigma*(sigma_next - sigma)   (fp32)
     with x read from euler_latent and x' written to euler_out, both fp16 (B,4,F,H,W); d is not written.
     Needs euler_latent, n == 64, n_store == 4, no geglu, no residuals, oscale == 1, euler_frames, euler_hw > 0, m a multiple
     of euler_frames*euler_hw, euler_sigma > 0; with euler_eps_uncond also euler_guidance and euler_ld_eps >= 4, a multiple
     of 4. */
  const void *euler_latent; void *euler_out;
  const void *euler_eps_uncond; int64_t euler_ld_eps;   /* fp16 [m][euler_ld_eps] eps rows of the unconditional pass, or NULL */
  const float *euler_guidance;                         /* fp32 [frames] per-frame guidance scale (with euler_eps_uncond) */
  float euler_sigma, euler_sigma_next;
  int euler_frames; int64_t euler_hw;                  /* m = b*frames*hw + f*hw + pixel */
  /* Optional scratch (the library never allocates): with at least sp_gemm_workspace_bytes(desc) bytes, contractions with
     few rows and a long K (m <= 6144, K >= 8192: the 3x3 convolutions of the UNet's 2,016-row level, 4,032 rows for a micro-batch of two) are split over K on 256 x 256 tiles,
     fp32 partial sums go here and a second kernel reduces them and applies the epilogue.  NULL = never split. */
  void *workspace; size_t workspace_bytes;
  /* LayerNorm statistics of the OUTPUT rows, for the next contraction's ln_stats (what a following sp_ln_stats_f16 pass
     over d would compute, without that pass): ln_out = fp32 [m][2] (mean, rstd = 1/sqrt(var + ln_out_eps)) of the n
     stored fp16 values of every row.  A row must be one to four 256- or 320-column tiles (n = 256 ... 1280; with more
     than one tile the per-tile sums pass through `workspace`, >= m * tiles * 8 bytes, 8-byte aligned, and a second small
     kernel folds them); no geglu, no
     n_store, no Euler tail; the call runs on the ping-pong kernels (no split-K).  Sums are folded in a fixed order:
     bit-reproducible.  NULL = off. */
  float *ln_out; float ln_out_eps;
  /* Per-row-group weights (SP_A_LINEAR only): with w_group_rows > 0, output rows [g*w_group_rows, (g+1)*w_group_rows)
     are multiplied with the weight matrix at w + g*w_group_stride halves instead of w (what a GroupNorm folded into the
     linear layer behind it needs: one scaled copy of the weights per frame, sp_groupnorm_fold_linear_f16; combine with a
     bias2 row per group).  w_group_rows must be a multiple of 128 AND of the height of the tiles the call runs on (no
     tile may straddle two groups): a multiple of 256 with gn_part (256-row tiles), of 256 or 192 with ln_out, and where it
     is a multiple of neither 256 nor 192 (128-row tiles) n must be a multiple of 256.  w_group_stride > 0, a multiple of 8;
     n a multiple of 256 or 320; no geglu / folded LayerNorm / Euler tail; the call runs on the ping-pong kernels (no
     split-K).  0 = one weight matrix for every row. */
  int64_t w_group_rows; int64_t w_group_stride;
  /* GroupNorm statistics of the NEXT norm out of this contraction's epilogue (round 5): gn_part = fp32
     [m/256][2][n][2] -- for every 256-row tile, each of its two 128-row halves and every output column, (sum, sum of
     squares) of the fp32 output values of the half's rows (bias / bias2 included, before the rounding to fp16).
     With residuals the sums are of the FINAL stored fp16 values instead (the tile is rebuilt in LDS behind the stores).
     sp_groupnorm_tile_sums_f16 folds them into the (mean, rstd) of any instance that is a whole number of tiles and
     normalises d without a statistics pass over it.  Needs m a multiple of 256, n a multiple of 256 or 320, no geglu /
     folded LayerNorm / ln_out / n_store / Euler tail; the call runs on the 256-row ping-pong tiles.  Sums
     are folded in a fixed order (bit-reproducible).  16-byte aligned.  NULL = off. */
  float *gn_part;
  /* Extra LINEAR tap (round 5): behind the taps of `mode` the contraction runs on over cin2 channels of a SECOND tensor a2
     (fp16 [m][lda2], row i for output row i), multiplied with weight columns [taps*cin, taps*cin + cin2): w is then
     [n][taps*cin + cin2].  A resnet's 1x1 shortcut convolution folded into its second 3x3 convolution
     (conv2(h) + conv_shortcut(x) = one contraction with bias = b2 + b_sc): the skip tensor is neither written nor read.
     cin2 a multiple of 64; runs on the 256-row ping-pong tiles (n a multiple of 256 or 320; no geglu / folded LayerNorm /
     ln_out / n_store / Euler tail / per-group weights / split-K; together with gn_part only without residuals).  lda2 >=
     cin2, a multiple of 8.  NULL = off. */
  const void *a2; int64_t lda2; int cin2;
  /* Guidance rows of the Euler tail: with euler_eps_uncond, video b of the batch mixes with
     euler_guidance[b * euler_guidance_ld + f] (fp32 [B][euler_guidance_ld], one row of per-frame scales per video;
     euler_guidance_ld >= euler_frames).  0 = the one row euler_guidance[f] is shared by every video. */
  int64_t euler_guidance_ld;
} sp_gemm_desc;

int sp_gemm_f16(const sp_gemm_desc *desc, void *stream);
/* sizeof(sp_gemm_desc) as the library was built: a binding in another language checks its mirror of the struct against
 * it once at load time (the Python one does: hip/__init__.py::load). */
size_t sp_gemm_desc_size(void);
/* bytes of sp_gemm_desc.workspace this contraction can use (0: it is not a split-K candidate) */
size_t sp_gemm_workspace_bytes(const sp_gemm_desc *desc);

/* Name of the kernel instantiation the calling thread's last sp_gemm_f16 launched (e.g. "gemm_pp_kernel<256, 320, 0>";
 * thread-local, valid until that thread's next call): lets a profile attribute FLOPs to kernel templates. */
const char *sp_gemm_last_kernel(void);

/* Nearest-neighbour x2 upsample followed by a 3x3 convolution (pad 1, stride 1; Upsample2D + conv of the UNet's up blocks)
 * as FOUR 2x2 convolutions.  After the upsample the nine taps of output pixel (oy, ox) touch a 2x2 window of source pixels
 * only, and which window, and how the nine weights add up onto it, depends on the parity (py, px) = (oy & 1, ox & 1) alone.
 * With phase p = 2*py + px, window tap t = 2*ty + tx and source pixel (sy, sx) = (oy >> 1, ox >> 1):
 *   d[img][2*sy + py][2*sx + px][:] = bias + sum_t a[img][sy + py - 1 + ty][sx + px - 1 + tx][:] . w[p][:][t*cin : (t+1)*cin]^T
 * (pixels outside the source image are zero), where the row weights of the fold are (w0, w1 + w2) for py = 0 and
 * (w0 + w1, w2) for py = 1, the same for columns with px (models/weights.py::pack_conv3x3_up2x folds in fp32 and rounds to
 * fp16 once).  K = 4*cin instead of the 9*cin of sp_gemm_f16 with upsample2x; same result up to that one rounding.
 *   a: fp16 [n_img*hin*win][lda] (NHWC rows), w: fp16 [4][n][4*cin], bias: fp32 [n] or NULL, d: fp16 [n_img*2hin*2win][ldd];
 *   gn_part: NULL, or fp32 [n_img*4*hin*win/256][2][n][2] column sums for the next GroupNorm as sp_gemm_desc.gn_part leaves
 *   them -- the 256-row tiles of one phase of one image cover the same 256 source pixels, so their sums stand at tile index
 *   img*4t + p*t + j (t = hin*win/256): the 4t tiles of an image are contiguous, which is all the folding kernels rely on.
 * Checked before anything is launched (SP_EINVAL, the message names the argument): a, w, d, zero_page non-NULL, all
 * pointers 16-byte aligned; cin a multiple of 64; n a multiple of 256 or 320; lda >= cin, ldd >= n, both multiples of 8;
 * positive geometry, 4*n_img*hin*win below 2^31; with gn_part hin*win a multiple of 256.
 * Runs as "gemm_pp_kernel<256, 256 | 320, 8192>" (the name sp_gemm_last_kernel reports afterwards). */
int sp_conv_up2x_f16(const void *a, int64_t lda, int cin, int n_img, int hin, int win, const void *w, int n,
                     const float *bias, void *d, int64_t ldd, float *gn_part, const void *zero_page, void *stream);

/* Test / micro-benchmark hook (no counterpart in the reference): pins the kernel family sp_gemm_f16 picks for the
 * shapes that family supports; everything else keeps the automatic choice.  Process-wide, not thread-safe: set it
 * before the calls it should affect.  route 0 = automatic (default), 1 = small tiles only, 2 = ping-pong large tiles
 * (bm in {0,128,192,256}, bn in {0,256,320}; 0 = automatic), 3 = persistent-stream tiles (bm in {0,192,256},
 * bn in {0,256}), 4 = split-K whenever a workspace is given (also for short K).
 * gn_part, a2, ln_out and w_group_rows override a forced route: those calls run on the ping-pong tiles their comments name,
 * whatever route is set. */
int sp_gemm_set_route(int route, int bm, int bn);

/* y[n] = act_out( W[n][:] . act_in(x) + b[n] ), M = 1.  Replaces the nn.Linear GEMVs of the
 * timestep / added-time / frame-position embeddings and every `time_emb_proj` (diffusers
 * TimestepEmbedding, ResnetBlock2D.time_emb_proj).  x, W fp16; b, y fp32 (y_f16 optional copy).
 * silu_in / silu_out apply SiLU to the input vector / output. `rows` independent input vectors. */
int sp_gemv_f16(const void *x, int64_t ldx, const void *w, const float *b, float *y, void *y_f16,
                int64_t ldy, int rows, int n, int k, int silu_in, int silu_out, void *stream);
/* `batch` independent GEMVs of one shape in a single launch (the 32 single-token cross-attention modules and the 16
 * frame-position MLPs of a forward are grouped by width).  Strides are in elements between consecutive problems;
 * x_stride = 0 shares the input, b may be NULL.  Otherwise as sp_gemv_f16. */
int sp_gemv_batched_f16(const void *x, int64_t ldx, int64_t x_stride, const void *w, int64_t w_stride,
                        const float *b, int64_t b_stride, float *y, void *y_f16, int64_t ldy, int64_t y_stride,
                        int batch, int rows, int n, int k, int silu_in, int silu_out, void *stream);

/* Sinusoidal embedding [cos | sin] (diffusers Timesteps(dim, flip_sin_to_cos=True, shift=0)) of
 * `count` fp32 values read from device memory; writes fp16 [count][dim]. */
int sp_sinusoid_f16(const float *values, void *out, int count, int dim, void *stream);

/* ---------------------------------------------------------------------------------------------
 * GroupNorm (+ optional SiLU), channels-last.  Replaces torch.nn.GroupNorm + F.silu in
 * ResnetBlock2D / TemporalResnetBlock / TransformerSpatioTemporalModel.norm / conv_norm_out.
 * x,y: fp16 [instances][rows][C]; statistics are taken per (instance, group) over rows x C/groups.
 * Spatial norm: instance = frame; temporal norm: instance = batch (rows = frames*H*W).
 * ws: >= sp_groupnorm_ws_bytes() bytes of scratch.
 * ------------------------------------------------------------------------------------------- */
size_t sp_groupnorm_ws_bytes(int instances, int64_t rows, int c, int groups);
int sp_groupnorm_f16(const void *x, const float *gamma, const float *beta, void *y, int instances,
                     int64_t rows, int c, int groups, float eps, int fuse_silu, void *ws,
                     size_t ws_bytes, void *stream);
/* The same with x a column slice of a wider row-major tensor: rows of ldx halves (ldx >= C, a multiple of 8), the C
 * channels at the head of each; y stays dense.  (The skip tensors of the down path live inside the buffers the up path
 * would otherwise build with torch.cat -- unet_spatio_temporal_condition.py up blocks -- so the norms that read them
 * in the down path see strided rows.) */
int sp_groupnorm_ld_f16(const void *x, int64_t ldx, const float *gamma, const float *beta, void *y, int instances,
                        int64_t rows, int c, int groups, float eps, int fuse_silu, void *ws,
                        size_t ws_bytes, void *stream);

/* GroupNorm(+SiLU) of a tensor whose producer left per-tile column sums (sp_gemm_desc.gn_part, `part` = that buffer for
 * the [instances*rows][c] tensor x with c = the producer's n): one small kernel folds the sums of every instance's tiles
 * into (mean, rstd) per (instance, group) in fp64 (fixed order), then the apply pass of sp_groupnorm_f16 runs -- no
 * statistics pass over x.  rows must be a multiple of 256 (an instance = whole tiles).  stats: fp32 scratch of
 * instances*groups*2 floats. */
int sp_groupnorm_tile_sums_f16(const void *x, int64_t ldx, const float *part, const float *gamma, const float *beta, void *y,
                               int instances, int64_t rows, int c, int groups, float eps, int fuse_silu, float *stats,
                               void *stream);
/* The same for a tensor that is the CONCATENATION [a | b] of two producers' outputs (an up block's resnet normalises
 * [hidden | skip]): channels [0, c_a) are summed in `part` (row pitch c_a), channels [c_a, c) in `part_b` (row pitch c - c_a);
 * per-column sums are additive, so a group may straddle the seam. */
int sp_groupnorm_tile_sums2_f16(const void *x, int64_t ldx, const float *part, int c_a, const float *part_b, const float *gamma,
                                const float *beta, void *y, int instances, int64_t rows, int c, int groups, float eps,
                                int fuse_silu, float *stats, void *stream);
/* sp_groupnorm_fold_linear_f16 (below) with the statistics folded from such column sums instead of a pass over x. */
int sp_groupnorm_fold_linear_tile_sums_f16(const float *part, const float *gamma, const float *beta, int instances, int64_t rows,
                                           int c, int groups, float eps, const void *w, const float *bias, int n, void *w_out,
                                           float *bias_out, float *stats, void *stream);
/* GroupNorm (no activation) folded into the nn.Linear that consumes it -- diffusers TransformerSpatioTemporalModel:
 * hidden = proj_in(norm(x)) -- so that the normalised tensor is never written or read:
 *   GN(x)[r][c] = (x[r][c] - mean[i][g(c)]) * rstd[i][g(c)] * gamma[c] + beta[c]      (i = instance of row r)
 *   proj_in(GN(x))[r][n] = sum_c x[r][c] * w_out[i][n][c] + bias_out[i][n]
 *   w_out[i][n][c]  = fp16( w[n][c] * gamma[c] * rstd[i][g(c)] )
 *   bias_out[i][n]  = bias[n] + sum_c beta[c]*w[n][c] - sum_c mean[i][g(c)] * float(w_out[i][n][c])
 * (the mean term uses the ROUNDED weights, so it cancels exactly what the MFMA adds for a constant offset of the group).
 * One statistics pass over x (the same kernels as sp_groupnorm_f16's first pass) + one small kernel that writes the
 * instances * n * c scaled weights; the caller then runs sp_gemm_f16 on the RAW x with w = w_out, w_group_rows = rows,
 * w_group_stride = n*c, bias = NULL, bias2 = bias_out, bias2_rows = rows.  x: fp16 [instances*rows][ldx] (C channels at
 * the head of each row); w: fp16 [n][c]; gamma, beta, bias: fp32 (bias may be NULL); ws as for sp_groupnorm_f16. */
int sp_groupnorm_fold_linear_f16(const void *x, int64_t ldx, const float *gamma, const float *beta, int instances,
                                 int64_t rows, int c, int groups, float eps, const void *w, const float *bias, int n,
                                 void *w_out, float *bias_out, void *ws, size_t ws_bytes, void *stream);

/* LayerNorm over the last dim (torch.nn.LayerNorm in BasicTransformerBlock /
 * TemporalBasicTransformerBlock).  Optional pre-add of a per-frame vector
 * (`hidden_states_mix = hidden_states + emb`): xin = x + addvec[row / addvec_rows]; if `sum_out`
 * is non-NULL the pre-norm sum is stored there as well.  fp16 in/out, fp32 affine. */
int sp_layernorm_f16(const void *x, const void *addvec, int64_t addvec_rows, void *sum_out,
                     const float *gamma, const float *beta, void *y, int64_t rows, int c, float eps,
                     void *stream);
/* Statistics only, for a LayerNorm that is folded into the next GEMM (sp_gemm_desc.ln_stats): stats[row] = (mean,
 * 1/sqrt(var + eps)) over the C channels of xin (same optional pre-add / sum_out as sp_layernorm_f16).  One read of
 * x instead of a read and a write. */
int sp_ln_stats_f16(const void *x, const void *addvec, int64_t addvec_rows, void *sum_out, float *stats,
                    int64_t rows, int c, float eps, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Attention.  Replaces F.scaled_dot_product_attention / xformers (svd_unet.py:142) for
 *  - spatial self-attention: sequences of `seq` tokens, `batch` of them (one per frame),
 *    q,k,v,o fp16 [batch*seq][heads*64] with row stride ld* (so q,k,v may alias one fused QKV buffer)
 *  - temporal self-attention: sequences run ACROSS frames for every pixel; token (f, p) lives at
 *    row f*hw + p, so no permute is materialised.
 * head_dim is fixed at 64 (all SVD levels).  softmax scale = 1/8.  zero_page: SP_ZERO_PAGE_BYTES of
 * zero-filled device memory (padding rows are read from it).
 * ------------------------------------------------------------------------------------------- */
int sp_attn_spatial_f16(const void *q, const void *k, const void *v, void *o, int64_t ldq,
                        int64_t ldk, int64_t ldv, int64_t ldo, int batch, int seq, int heads,
                        float scale, const void *zero_page, void *stream);
int sp_attn_temporal_f16(const void *q, const void *k, const void *v, void *o, int64_t ldq,
                         int64_t ldk, int64_t ldv, int64_t ldo, int batch, int frames, int64_t hw,
                         int heads, float scale, const void *zero_page, void *stream);
/* sp_attn_spatial_f16 for LONG rows (csrc/attention_long.hip): same arguments, same results to fp16 rounding.
 * Two query blocks per wave, one or two waves per SIMD (sp_attn_long_set_occupancy below); after a warm-up over the
 * workgroup's own tokens and tile 0 (ordinary online softmax) each row's reference is frozen at the maximum seen so far and the remaining K/V tiles run without
 * row maximum or rescale.  A later score more than 16 (log2 units) above that reference overflows fp16, is detected
 * through the row sum, and the 256-row block is recomputed by sp_attn_spatial_f16's kernel inside the same call, so
 * accuracy never depends on the data (only the time does).  Applies to seq >= 4096 with seq % 256 == 0; every other
 * shape is passed to sp_attn_spatial_f16's kernel unchanged (workspace unused).  workspace: >=
 * sp_attn_long_ws_bytes(batch, seq, heads) bytes, 4-byte aligned, owned by the caller and private to the call until
 * it has completed on `stream` (one flag word per 256 query rows; zeroed by the call). */
int64_t sp_attn_long_ws_bytes(int batch, int seq, int heads);
int sp_attn_spatial_long_f16(const void *q, const void *k, const void *v, void *o, int64_t ldq, int64_t ldk,
                             int64_t ldv, int64_t ldo, int batch, int seq, int heads, float scale,
                             const void *zero_page, void *workspace, int64_t workspace_bytes, void *stream);
/* Test / micro-benchmark hook (no counterpart in the reference): the frozen-reference kernel exists in two
 * instantiations with identical arithmetic and bit-identical results, "attn_long_kernel<2, 1>" (one wave per SIMD, one
 * workgroup per CU) and "attn_long_kernel<2, 2>" (256 registers per wave, two workgroups per CU).  occ = 1 or 2 pins
 * the one sp_attn_spatial_long_f16 launches, 0 restores the library's default.  Process-wide, not thread-safe: set it
 * before the calls it should affect. */
int sp_attn_long_set_occupancy(int occ);
/* Name of the kernel the calling thread's last sp_attn_spatial_long_f16 launched first: one of the two above, or
 * "attn_spatial_kernel" for a shape it passed on (static string). */
const char *sp_attn_long_last_kernel(void);
/* fp8 (OCP e4m3fn) MFMA variant of sp_attn_spatial_f16 for BASELINE config 5 ("fp8 MFMA attention path"; the
 * reference has no fp8 path of its own, its attention is diffusers/xformers behind svd_unet.py:142-199).
 * Same arguments and fp16 inputs/outputs; q/k/v are quantised per call into `workspace` (Q8, K8 row-major,
 * V8 transposed per head) and S^T = K.Q^T, O^T += V^T.P^T run on v_mfma_f32_32x32x16_fp8_fp8 with fp32
 * accumulation and fp32 softmax.  workspace: >= sp_attn_fp8_ws_bytes(batch, seq, heads) bytes, 16-byte aligned,
 * owned by the caller (never allocated here).  Tolerance vs the fp32 oracle: rel-L2 <= 3e-2. */
int64_t sp_attn_fp8_ws_bytes(int batch, int seq, int heads);
int sp_attn_spatial_fp8(const void *q, const void *k, const void *v, void *o, int64_t ldq, int64_t ldk,
                        int64_t ldv, int64_t ldo, int batch, int seq, int heads, float scale,
                        void *workspace, int64_t workspace_bytes, const void *zero_page, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Layout / elementwise glue around the UNet (svd_unet.py:382-439).
 * ------------------------------------------------------------------------------------------- */
/* latent (B,4,F,H,W) * in_scale  ++  image_latents (B,4,F,H,W)  ->  NHWC rows [B*F*H*W][cpad]
 * (channels 0-3 scaled latent, 4-7 image latents, rest zero): svd_unet.py:382,414-415 */
int sp_pack_input_f16(const void *latent, const void *image_latents, void *out, float in_scale,
                      int b, int frames, int h, int w, int cpad, void *stream);
/* The sampler tails behind stored eps rows: one kernel (csrc/sampler_tail.hip; arithmetic: csrc/sampler_math.h).  All five
 * entry points refuse, without launching: null pointers, eps_uncond without guidance, ld_eps no positive multiple of 4,
 * dimensions that are not positive, ld_guidance in (0, frames), sigma <= 0, an out that overlaps the input unless it IS the input.
 * v-prediction Euler update with optional CFG, fp32 math (svd_unet.py:410-411,425-439):
 * eps = eps_u + gs[f]*(eps_c - eps_u) if eps_uncond!=NULL else eps_c;
 * x' = x + ((x - (eps*c_out + x*c_skip))/sigma)*dt.  eps_* are NHWC [B*F*H*W][ld_eps]; latent and
 * out are (B,4,F,H,W). */
int sp_euler_step_f16(const void *latent, const void *eps_cond, const void *eps_uncond,
                      int64_t ld_eps, const float *guidance /*[F] or NULL*/, void *out, float sigma,
                      float sigma_next, int b, int frames, int h, int w, void *stream);
/* sp_euler_step_f16 with one guidance row per video: gs[b*ld_guidance + f] (guidance fp32 [B][ld_guidance],
 * ld_guidance >= frames); ld_guidance = 0 is sp_euler_step_f16 (one row [F] shared by every video). */
int sp_euler_step_rows_f16(const void *latent, const void *eps_cond, const void *eps_uncond,
                           int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out, float sigma,
                           float sigma_next, int b, int frames, int h, int w, void *stream);
/* DPM-Solver++(2M) update, the second-order multistep sampler with one UNet evaluation per step.  The
 * solver's history rides in the latent: state and out_state are fp16 (B,8,F,H,W), channels 0-3 the sample x, channels
 * 4-7 the previous step's denoised estimate D_prev.  Per element, fp32 math on fp16 storage:
 *   e  = eps_u + g[b,f]*(eps_c - eps_u)   evaluated in fp16 exactly as sp_euler_step_rows_f16 does; e = eps_c if !eps_uncond
 *   D  = x/(sigma^2+1) - e*sigma/sqrt(sigma^2+1)          (v-prediction: the c_skip / c_out of the Euler update)
 *   x' = a*x + b*(c1*D - c2*D_prev)  -> out_state[:, 0:4];     D -> out_state[:, 4:8]
 * a = sigma'/sigma, b = 1 - a, c2 = h/(2*h_last), c1 = 1 + c2 (models/solver_schedule.py); c1 = 1, c2 = 0 at the first and
 * the last step, where x' = a*x + b*D is algebraically the Euler step.  With c2 == 0 channels 4-7 of state are NOT read
 * (step 0's are don't-care).  eps rows, guidance rows and ld_guidance as for sp_euler_step_rows_f16.  Refused: sigma <= 0,
 * a outside [0, 1), c2 < 0, out_state overlapping state unless it IS state (in place). */
int sp_dpmpp2m_step_rows_f16(const void *state, const void *eps_cond, const void *eps_uncond,
                             int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out_state,
                             float sigma, float a, float b, float c1, float c2,
                             int batch, int frames, int h, int w, void *stream);
/* Long videos: the two sampler tails behind overlapping frame windows.  A latent
 * of frames_total frames is cut into n_win = (frames_total - window)/stride + 1 windows of `window` frames, window k covering
 * global frames k*stride .. k*stride + window - 1 (1 <= stride <= window, (frames_total - window) % stride == 0); the UNet ran
 * on every window and left its eps rows in ONE buffer, NHWC rows [n_win][B][window][H*W][ld_eps]: window k of all videos
 * starts at row k*B*window*H*W.  weights is the normalised fp32 table [n_win][window] of models/window_plan.py (over the
 * windows covering a global frame it sums to 1).  Per element of global frame f = k*stride + p:
 *   e_k = eps_u + g[b,p]*(eps_c - eps_u)   per window, in fp16, rounding for rounding as sp_euler_step_rows_f16; e_k = eps_c
 *                                          if !eps_uncond.  Guidance follows the POSITION p in the window (guidance is
 *                                          [window] with ld_guidance 0, or [B][ld_guidance >= window]), not the global frame
 *   e   = sum over the covering k, ascending, of weights[k][p]*e_k     fp32 fmaf from 0, never rounded to fp16
 * and the update is that of the single-window function with e in place of its eps: latent/out (B,4,frames_total,H,W) for
 * Euler, state/out_state (B,8,frames_total,H,W) for DPM-Solver++(2M) (D -> channels 4-7; with c2 == 0 channels 4-7 of state
 * are not read).  With n_win == 1 (weights 1.0) the bytes are those of sp_euler_step_rows_f16 / sp_dpmpp2m_step_rows_f16.
 * Every element of the input is read before the thread that owns it stores: out may be the input itself.  Refused, without
 * launching: null pointers (weights included), stride outside [1, window], window > frames_total, a total that is not window
 * plus whole strides, n_win other than the plan's, ld_guidance in (0, window), out overlapping the input unless it IS the
 * input, and everything the single-window functions refuse. */
int sp_euler_step_windows_f16(const void *latent, const void *eps_cond, const void *eps_uncond,
                              int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out, float sigma,
                              float sigma_next, int b, int frames_total, int h, int w,
                              int window, int stride, int n_win, const float *weights /*[n_win][window]*/, void *stream);
int sp_dpmpp2m_step_windows_f16(const void *state, const void *eps_cond, const void *eps_uncond,
                                int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out_state,
                                float sigma, float a, float b, float c1, float c2,
                                int batch, int frames_total, int h, int w,
                                int window, int stride, int n_win, const float *weights /*[n_win][window]*/, void *stream);
/* The stochastic samplers: the two tails above with fresh noise at every step, n*z added in fp32 inside
 * the update.  z is standard normal and a pure function of (the video's 64-bit seed, `step`, the element's position in the
 * video's latent): Philox4x32-10 (csrc/noise.h) with, for element (c, f, p) of the video's (4, frames_total, H, W) latent,
 * e = (c*frames_total + f)*H*W + p, f the GLOBAL frame: counter (e >> 2, step, 1, 0), key (seed & 0xffffffff, seed >> 32),
 * lane e & 3 of the block's four Box-Muller normals.  Nothing depends on the video's row in the batch, on the windows or on
 * who calls.  seeds is [batch] on the device, 8-byte aligned.  Arguments as for the _windows_ functions; weights == NULL with
 * n_win == 1 and window == frames_total is the unwindowed form (eps rows [B][F][H*W][ld_eps], guidance indexed by the frame).
 *   Euler ancestral:  t = x + (x - x0)/sigma*(sigma_down - sigma) in fp32, out = fp16(noise_scale*z + t), one rounding;
 *                     sigma_down and noise_scale = s_noise*sigma_up from models/solver_schedule.py
 *   2M SDE:           x' = noise_scale*z + (a*x + b*(c1*D - c2*D_prev)); D -> channels 4-7 without noise
 * noise_scale == 0 launches the deterministic kernel: the bytes of the _windows_ / _rows_ functions for the same constants,
 * seeds not read (may be NULL).  Refused besides what those refuse: null seeds with noise_scale != 0, misaligned seeds, a
 * negative or non-finite noise_scale, 4*frames_total*H*W > 2^34. */
int sp_euler_ancestral_step_f16(const void *latent, const void *eps_cond, const void *eps_uncond,
                                int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out, float sigma,
                                float sigma_down, int b, int frames_total, int h, int w,
                                int window, int stride, int n_win, const float *weights /*[n_win][window] or NULL*/,
                                float noise_scale, const uint64_t *seeds /*[batch], device*/, uint32_t step, void *stream);
int sp_dpmpp2m_sde_step_f16(const void *state, const void *eps_cond, const void *eps_uncond,
                            int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out_state,
                            float sigma, float a, float b, float c1, float c2,
                            int batch, int frames_total, int h, int w,
                            int window, int stride, int n_win, const float *weights /*[n_win][window] or NULL*/,
                            float noise_scale, const uint64_t *seeds /*[batch], device*/, uint32_t step, void *stream);
/* Large frames: the tails behind overlapping spatial tiles times the frame windows.  Per axis the
 * rule of the frame windows: total T, tile t, stride s, 1 <= s <= t <= T, (T - t) % s == 0, n = (T - t)/s + 1 tiles, tile k
 * covering cells k*s .. k*s + t - 1.  The UNet ran on every patch (kf, ky, kx) -- frame window kf, tile (ky, kx) -- and left
 * its eps rows in ONE buffer, NHWC rows [n_patch][B][window][tile_h*tile_w][ld_eps], patch k = (kf*n_ty + ky)*n_tx + kx of all
 * videos starting at row k*B*window*tile_h*tile_w.  The weights are separable: three normalised fp32 tables on the device
 * (models/tile_plan.py), wf [n_win][window], wy [n_ty][tile_h], wx [n_tx][tile_w]; without frame windows n_win = 1, window =
 * stride = frames_total and wf is all 1.0.  Per element of global frame f and pixel (y, x) of the LARGE latent:
 *   e_k = eps_u + g[b,p]*(eps_c - eps_u)    per covering patch, in fp16, as in the _windows_ functions; p = f - kf*stride
 *   w_k = (wf[kf][p] * wy[ky][y - ky*stride_y]) * wx[kx][x - kx*stride_x]      fp32 products in this order
 *   e   = fmaf(w_k, e_k, e) from 0 over the covering patches, kf ascending outermost, then ky, then kx; never rounded to fp16
 * and the update of the _windows_ functions follows, or with noise_scale != 0 that of the stochastic ones (sigma_next_or_down
 * is then sigma_down); the noise address stays (c*frames_total + f)*h*w + y*w + x with the large h, w, so z does not depend on
 * the tiling.  One tile that is the whole frame (wy = wx = {1.0}) gives the bytes of the _windows_ / stochastic functions.
 * out may be the input itself.  Refused, without launching: a null plan or table, a stride outside [1, tile] on any axis, a
 * total that is not tile plus whole strides, a tile count other than the plan's, ld_guidance in (0, window), 4*frames_total*h*w
 * > 2^34, out overlapping the input unless it IS the input, and everything the _windows_ and stochastic functions refuse. */
typedef struct sp_tile_plan {
  int frames_total, window, stride, n_win;
  int h, w, tile_h, tile_w, stride_y, stride_x, n_ty, n_tx;
  const float *wf, *wy, *wx;
} sp_tile_plan;
size_t sp_tile_plan_size(void);
int sp_euler_step_tiles_f16(const sp_tile_plan *plan, const void *latent, const void *eps_cond, const void *eps_uncond,
                            int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out, float sigma,
                            float sigma_next_or_down, int batch, float noise_scale,
                            const uint64_t *seeds /*[batch], device, or NULL with noise_scale 0*/, uint32_t step, void *stream);
int sp_dpmpp2m_step_tiles_f16(const sp_tile_plan *plan, const void *state, const void *eps_cond, const void *eps_uncond,
                              int64_t ld_eps, const float *guidance, int64_t ld_guidance, void *out_state,
                              float sigma, float a, float b, float c1, float c2, int batch, float noise_scale,
                              const uint64_t *seeds /*[batch], device, or NULL with noise_scale 0*/, uint32_t step, void *stream);
/* out (B,4,F,H,W) fp16 = fp16(scale*z), the product rounded once, with z of counter (e >> 2, step, purpose, 0) as above: the initial latent of a video
 * from its seed (scale = init_noise_sigma, step 0, purpose 0), or with purpose 1 the normals a tail adds at `step`.  Refused:
 * null or misaligned pointers, a negative or non-finite scale, 4*F*H*W > 2^34. */
int sp_randn_f16(void *out, const uint64_t *seeds /*[batch], device*/, float scale, int batch, int frames, int h, int w,
                 uint32_t step, uint32_t purpose, void *stream);
/* The generator's raw words, out [batch][n_blocks][4] (16-byte aligned): block j of video b is Philox4x32-10 of counter
 * (j, step, purpose, 0) under the key of seeds[b]; n_blocks <= 2^32. */
int sp_philox_blocks_u32(uint32_t *out, const uint64_t *seeds, int batch, int64_t n_blocks, uint32_t step,
                         uint32_t purpose, void *stream);
/* channel concat of two NHWC tensors (torch.cat([hidden, skip], dim=1) in the up blocks) */
int sp_concat_channels_f16(const void *a, int ca, const void *b, int cb, void *out, int64_t rows,
                           void *stream);
/* y = x + vec[c] broadcast over rows (used for the degenerate single-token cross-attention) */
int sp_add_rowvec_f16(const void *x, const float *vec, void *y, int64_t rows, int c, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Temporal VAE decoder on the last stage: /root/reference/scripts/generate_video_demo.py:154-195
 * calls diffusers AutoencoderKLTemporalDecoder.decode; its convolutions, GroupNorms and projections are the kernels
 * above, the two below are what it needs besides.
 * ------------------------------------------------------------------------------------------- */
/* in-place softmax over each of `rows` rows of x (fp16 [rows][ld], `cols` <= 16384 columns, multiple of 8): the
 * [tokens][tokens] scores of the mid block's single-head attention (attention_processor.py Attention, heads = 1,
 * dim_head = 512), which sp_gemm_f16 wrote already scaled by 1/sqrt(dim_head).  fp32 statistics. */
int sp_softmax_rows_f16(void *x, int64_t ld, int64_t rows, int cols, void *stream);
/* The same attention with logits that never pass through fp16 (the reference runs this VAE in fp32 because trained
 * weights overflow fp16: scripts/generate_video_demo.py:171-175):
 *   sp_gemm_f32out_f16: D[m][n] (fp32, row pitch n) = A[m][k] . W[n][k]^T, raw fp32 sums, no bias / epilogue
 *                       (a fp16 [m][lda], w fp16 [n][k]; n a multiple of 256, k a multiple of 64, d 16-byte aligned);
 *   sp_softmax_rows_f32: out[r][c] = fp16(softmax_c(scale * x[r][c])), x fp32 [rows][ld], out fp16 [rows][ldo], fp32
 *                       statistics, nothing clamped (a NaN stays a NaN).  out may be x itself with ldo = 2*ld: the
 *                       probabilities of a row then overwrite the front of that row's logits (no second matrix). */
int sp_gemm_f32out_f16(const void *a, int64_t lda, const void *w, void *d, int m, int n, int k, const void *zero_page,
                       void *stream);
int sp_softmax_rows_f32(const float *x, int64_t ld, void *out, int64_t ldo, int64_t rows, int cols, float scale, void *stream);
/* sp_softmax_rows_f32 for rows of any length: the same arguments and the same contract (fp32 statistics, nothing clamped, a
 * NaN stays a NaN, out may be x itself with ldo = 2*ld), with `cols` a multiple of 4 from 4 to 16,777,216 (2^24).  The row
 * is not held in registers but streamed three times (maximum, sum, store) in pieces of 256 x 4 logits, with the register
 * kernel's assignment of elements to threads and its order of accumulation and reduction: for cols <= 16,384 it returns the
 * bytes of sp_softmax_rows_f32.  Frames of more than 16,384 cells in the VAE's mid-block attention (models/vae_hip.py). */
int sp_softmax_rows_long_f32(const float *x, int64_t ld, void *out, int64_t ldo, int64_t rows, int cols, float scale,
                             void *stream);
/* Both ends of one decoder call work on `n` consecutive entries g = flat0 .. flat0+n-1 of the flattened (batch, frame)
 * list of a video tensor with F frames per batch item (generate_video_demo.py:162-181 cuts that flat list into chunks
 * of decode_chunk_size); entry g is batch item g / F, frame g % F, and element (g, channel c, pixel p) of the tensor
 * sits at  base + (g/F)*sb + c*sc + (g%F)*sf + p  (element strides: (B,C,F,H,W) has sb = C*F*hw, sc = F*hw, sf = hw;
 * (B*F,C,H,W) has sb = F*C*hw, sc = hw, sf = C*hw).
 * pack: latent channels 0-3 * scale (= 1/scaling_factor) -> channels-last rows [n*h*w][cpad], other channels zero. */
int sp_vae_pack_latent_f16(const void *latent, void *rows, float scale, int64_t flat0, int n, int F, int64_t sb,
                           int64_t sc, int64_t sf, int h, int w, int cpad, void *stream);
/* frames out: time_conv_out = Conv3d(3 -> 3, kernel (3,1,1), zero padding over the `frames` of each of the call's
 * `batch` items, n = batch*frames) applied to the channels-last rows conv_out produced (fp16 [n*h*w][ld], channels
 * 0-2), written into the video tensor `out` (fp16, or fp32 when out_fp32 != 0) at the strides above.
 * weight: fp32 [3][3][3] = [out][in][tap], bias fp32 [3]. */
int sp_vae_frames_out_f16(const void *rows, int64_t ld, const float *weight, const float *bias, void *out,
                          int out_fp32, int batch, int frames, int h, int w, int64_t flat0, int F, int64_t sb,
                          int64_t sc, int64_t sf, void *stream);
/* The same time_conv_out values as 8-bit frames: each fp32 value goes through the arithmetic of sp_frames_to_u8 (below) and
 * is stored at out[((flat0 + i)*h*w + p)*3 + c] for entry i of the call, pixel p, channel c -- a dense (B*F, H, W, 3) uint8
 * tensor, a quarter of the fp32 video's bytes.  Byte for byte what sp_frames_to_u8 makes of sp_vae_frames_out_f16(out_fp32 = 1):
 * both kernels share one device function for the value and one for the level. */
int sp_vae_frames_out_u8(const void *rows, int64_t ld, const float *weight, const float *bias, void *out, int batch,
                         int frames, int h, int w, int64_t flat0, void *stream);

/* Encoder half (vae.encode(image).latent_dist.mode(), generate_video_demo.py:139-148).  flip != 0 mirrors the image in
 * both axes between the tensor and the rows (pixel (y,x) <-> row (H-1-y)*W + (W-1-x)): the engine runs the encoder on
 * the mirrored image, where Downsample2D's bottom/right padding is the stride-2 kernel's top/left padding.
 * pack: image fp16 (batch,3,h,w) -> channels-last rows [batch*h*w][cpad] (channels 3.. zero). */
int sp_vae_image_pack_f16(const void *image, void *rows, int batch, int h, int w, int cpad, int flip, void *stream);
/* latent out: rows fp16 [batch*h*w][ld], channels 0..channels-1 -> out fp16 (batch, channels, frames, h, w), every frame
 * a copy (image_latents.unsqueeze(2).repeat(1,1,num_frames,1,1), generate_video_demo.py:148). */
int sp_vae_latent_out_f16(const void *rows, int64_t ld, void *out, int batch, int channels, int frames, int h, int w,
                          int flip, void *stream);

/* ---------------------------------------------------------------------------------------------
 * CLIP image encoder on the first stage: /root/reference/scripts/generate_video_demo.py:108-112 calls
 * transformers CLIPVisionModelWithProjection (ViT-H/14); its contractions and LayerNorms are the kernels above.
 * ------------------------------------------------------------------------------------------- */
/* im2col of non-overlapping patches: pixels fp16 (batch,3,h,w) -> rows fp16 [batch*(h/patch)*(w/patch)][kpad],
 * k = c*patch*patch + ky*patch + kx (= the flattened Conv2d weight of CLIPVisionEmbeddings.patch_embedding), zeros
 * from 3*patch*patch up to kpad. */
int sp_patchify_f16(const void *pixels, void *rows, int batch, int h, int w, int patch, int kpad, void *stream);
/* softmax(q k^T * scale) v for short sequences (seq <= 512) and any head width that is a multiple of 8 up to 128
 * (ViT-H: 257 tokens, 16 heads of 80): row (b*seq + i), head hh of q/k/v/o starts at column hh*head_dim.  fp32 math,
 * fp16 in/out; K and V of one (batch item, head) must fit in LDS. */
int sp_attn_small_f16(const void *q, const void *k, const void *v, void *o, int64_t ldq, int64_t ldk, int64_t ldv,
                      int64_t ldo, int batch, int seq, int heads, int head_dim, float scale, void *stream);
/* y = gelu(x) elementwise over n fp16 values (n a multiple of 8): exact erf form (hidden_act "gelu"), or
 * x*sigmoid(1.702 x) when quick != 0 ("quick_gelu"). */
int sp_gelu_f16(const void *x, void *y, int64_t n, int quick, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Image in, 8-bit frames out: the host-side image handling of /root/reference/scripts/generate_video_demo.py on the device
 * (load_and_preprocess_image :71-89, the CLIPImageProcessor / ToTensor / Normalize of encode_image :108-126, and the
 * uint8 conversion of save_video :198-209).  Images are uint8 RGB, interleaved [h][w][3]; row pitches are in BYTES and may be
 * any value >= 3*w (no alignment is assumed), so a crop is a pointer into a larger image plus that image's pitch.
 * ------------------------------------------------------------------------------------------- */
enum { SP_FILTER_BICUBIC = 0 /* a = -0.5, support 2 */, SP_FILTER_LANCZOS3 = 1 /* support 3 */ };
/* Pillow's antialiased separable resize (Image.resize with BICUBIC / LANCZOS): the horizontal pass writes src_h x dst_w
 * pixels to `tmp`, the vertical pass reads them; a pass whose size does not change is a copy.  Per axis, with scale =
 * in/out, fs = max(scale, 1), support = S*fs: output i has centre = (i + 0.5)*scale and taps k in [max(0, int(centre -
 * support + 0.5)), min(in, int(centre + support + 0.5))) weighted filter((k - centre + 0.5)/fs), normalised by the sum of
 * the taps kept; the result is floor(v + 0.5) clipped to [0, 255] and is stored as uint8 between the passes as well.
 * Geometry in fp64, weights and sums in fp32: within one level of Pillow (whose weights are 22-bit fixed point).
 * tmp: >= sp_image_resample_tmp_bytes(src_h, dst_w) = src_h*dst_w*3 bytes, owned by the caller. */
size_t sp_image_resample_tmp_bytes(int src_h, int dst_w);
int sp_image_resample_u8(const void *src, int64_t src_pitch, int src_h, int src_w, void *dst, int64_t dst_pitch, int dst_h,
                         int dst_w, int filter, void *tmp, size_t tmp_bytes, void *stream);
/* uint8 [h][w][3] -> fp16 planar (3, h, w): out[c][y][x] = fp16((float(v)/255.0f - mean[c]) / std[c]).  torchvision's
 * ToTensor + Normalize([0.5], [0.5]) (the VAE's input) and the rescale + normalize of the CLIPImageProcessor. */
int sp_image_to_tensor_f16(const void *src, int64_t src_pitch, int h, int w, void *out, float mean0, float mean1, float mean2,
                           float std0, float std1, float std2, void *stream);
/* video (B, 3, F, H, W) fp16 (is_fp32 == 0) or fp32 -> uint8 (B, F, H, W, 3): v = ((x + 1.0f)/2.0f)*255.0f in fp32, clamped to
 * [0, 255] and truncated, as ((frames + 1) / 2 * 255).clamp(0, 255).to(torch.uint8) does; a NaN gives 0. */
int sp_frames_to_u8(const void *frames, int is_fp32, void *out, int batch, int frames_n, int h, int w, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Video files out: baseline JPEG of uint8 frames that are in device memory (the reference hands its frames to imageio /
 * ffmpeg: /root/reference/scripts/generate_video_demo.py:198-222).  Sequential DCT, 8 bit, YCbCr 4:2:0: an MCU is 16x16
 * pixels and holds six 8x8 blocks in the order Y00 Y01 Y10 Y11 Cb Cr; mcu_rows = ceil(h/16), mcu_cols = ceil(w/16); h and w
 * are 1..65535 (what SOF0 can say).  Two stages: coefficients, then the entropy-coded segment of the scan.  Marker
 * segments (SOI .. SOS, EOI) and containers are written by the host from the two table queries below.
 * ------------------------------------------------------------------------------------------- */
/* Host only.  quality 1..100 -> the two quantisation tables in natural (row-major) order, libjpeg's scaling of the Annex K
 * tables: s = quality < 50 ? 5000/quality : 200 - 2*quality; t = clamp((base*s + 50)/100, 1, 255), integer arithmetic.  The
 * kernel below evaluates the same function. */
int sp_jpeg_quant_tables(int quality, uint8_t *luma64, uint8_t *chroma64);
/* Host only.  The Annex K Huffman table `which` (0 DC luminance, 1 DC chrominance, 2 AC luminance, 3 AC chrominance) as a
 * DHT segment carries it: bits16[i] = number of codes of length i+1, then the symbols in code order (at most 162).
 * Returns the number of symbols, or SP_EINVAL. */
int sp_jpeg_huffman_table(int which, uint8_t *bits16, uint8_t *vals162);
/* n * mcu_rows * mcu_cols * 6 * 64 * 2 bytes; 0 for sizes the calls below refuse */
size_t sp_jpeg_coef_bytes(int n, int h, int w);
/* frames: uint8 [n][h][w][3] RGB -> coef: int16 [n][mcu_rows][mcu_cols][6][64], every block in zigzag order.
 * Sample (y, x) of the MCU grid reads pixel (min(y, h-1), min(x, w-1)).  Per pixel, in integers (libjpeg's jccolor):
 *   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *   Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 * chroma is box-averaged 2x2 as (a + b + c + d + bias) >> 2, bias 1 in even output columns and 2 in odd ones (h2v2_downsample).
 * Each 8x8 block minus 128 goes through the orthonormal 2-D DCT-II in fp32 (row pass, then column pass, 8-term fma chains);
 * a coefficient is divided by its table entry (fp32 division) and rounded half away from zero; AC terms are clamped to
 * +-1023, the largest magnitude baseline Huffman codes. */
int sp_jpeg_dct_quant_u8(const void *frames, int n, int h, int w, int quality, void *coef, void *stream);
/* Bytes of entropy-coded data no frame can exceed: a block is at most 20 + 63*26 = 1658 bits (luminance: DC 9-bit code + 11
 * bits, AC 16-bit code + 10 bits per coefficient; chrominance: DC 11 + 11 bits, but at most 12 + 10 per coefficient, 1408
 * in all), 208 bytes, and byte stuffing at most doubles it:
 *   416 * 6 * mcu_rows * mcu_cols + 2 * (intervals - 1),   intervals = ceil(mcu_rows * mcu_cols / restart_mcus)
 * 0 for sizes sp_jpeg_entropy refuses. */
size_t sp_jpeg_stream_bytes(int h, int w, int restart_mcus);
/* Scratch of sp_jpeg_entropy: two int32 per (frame, interval), rounded up to 256 bytes, then a staging slot of
 * 416 * 6 * min(restart_mcus, mcu_rows * mcu_cols) bytes per (frame, interval). */
size_t sp_jpeg_entropy_ws_bytes(int n, int mcu_rows, int mcu_cols, int restart_mcus);
/* coef as above -> for frame i the entropy-coded segment of its scan at out + i*cap and its length in out_len[i] (int32,
 * device).  MCUs in raster order; the DC of each component is coded as the difference to the previous block of that
 * component, all three predictors being 0 at the start of every restart interval of restart_mcus (1..65535) MCUs; Annex K
 * tables, ZRL for 16 zeros, EOB unless coefficient 63 is non-zero; every interval is padded to a byte with 1-bits, every
 * 0xFF byte of coded data is followed by 0x00, and 0xFF 0xD0+(k mod 8) stands between interval k and k+1.  Nothing follows
 * the last interval (the host appends EOI).  cap (bytes per frame) below sp_jpeg_stream_bytes is refused, so no input can
 * make a frame leave its slot; bytes of a slot beyond out_len[i] are not written.  Coefficients outside the baseline range
 * (AC beyond +-1023, DC differences beyond +-2047) give a stream no decoder accepts, within the same bound. */
int sp_jpeg_entropy(const void *coef, int n, int mcu_rows, int mcu_cols, int restart_mcus, void *out, size_t cap, void *out_len,
                    void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Pictures in: a baseline JPEG file decoded on the device from its compressed bytes (the reference opens its input with
 * Pillow on the host: scripts/generate_video_demo.py:75 there).  Decoded: SOF0, 8-bit samples and tables, one component
 * (grey, returned as R = G = B) or three (YCbCr, chrominance sampled 1x1, luminance 1x1, 2x1 or 2x2), one interleaved scan,
 * any restart interval or none.  The host walks the markers and hands over the header's numbers and tables (a "plan", host
 * memory) and the entropy-coded segment (device memory); a copy of the plan in device memory goes to every call as plan_dev.
 * Four calls, in this order on one stream; all leave at once while the status block reports an error, so a broken stream is
 * never followed, and no call reads or writes outside its buffers, whatever the bytes are.
 *
 * The status block is the first 64 int32 of ws: [0] error bits (1 an 0xFF that neither 0x00 nor RSTn follows, 2 RSTn out of
 * order, 4 number of RSTn, 8 an unassigned code / a zigzag index past 63 / a size above 11 (DC) or 10 (AC), 16 an interval
 * whose blocks do not come to its MCUs x blocks per MCU), [1] a pass found the fixed point reached, [2] passes executed,
 * [3] bytes of the clean stream, [4] RSTn markers, [5] subsequences, [6] subsequences of the longest interval,
 * [10] coefficients written.
 * ------------------------------------------------------------------------------------------- */
size_t sp_jpeg_decode_plan_bytes(void);
/* Host only.  fields: 17 int32 = width, height, components (1 or 3), luminance sampling h, v, restart interval (0: none),
 * bytes of the entropy-coded segment (1..2^28-1), subseq_bits (a multiple of 32 in 32..2^20), quantisation table selector
 * per component [3], DC table selector per component [3], AC table selector per component [3] (Huffman selectors 0 or 1).
 * quant4x64: tables 0..3 in natural (row-major) order; bits4x16 / vals4x256: the DHT specifications of DC 0, DC 1, AC 0,
 * AC 1; have_quant / have_huff: bit i set where table i was defined.  Writes sp_jpeg_decode_plan_bytes() bytes to plan.
 * SP_EINVAL for numbers outside the scope above, a selector without its table, or a specification no canonical code has
 * (which includes one that assigns an all-ones code). */
int sp_jpeg_decode_plan(const int32_t *fields, const uint8_t *quant4x64, int have_quant, const uint8_t *bits4x16,
                        const uint8_t *vals4x256, int have_huff, void *plan);
/* Scratch of the four calls / bytes of the coefficients, int16 [mcu_rows][mcu_cols][blocks_per_mcu][64] (zigzag order, DC
 * absolute; for 2x2 sampling the layout of sp_jpeg_dct_quant_u8).  0 for a pointer that is no plan. */
size_t sp_jpeg_decode_ws_bytes(const void *plan);
size_t sp_jpeg_decode_coef_bytes(const void *plan);
/* 1. Unstuff and split.  Clears the status block; removes the 0x00 behind every 0xFF of coded data and the RSTn markers
 * (flags, an exclusive scan), writes the clean bytes and the byte range of every restart interval (one interval without
 * DRI), checks that the markers count 0..7 in order and are as many as the intervals need; then cuts every interval into
 * subsequences of subseq_bits. */
int sp_jpeg_decode_split(const void *plan, const void *plan_dev, const void *segment, void *ws, size_t ws_bytes, void *stream);
/* 2. Synchronisation passes first_pass .. first_pass + passes - 1 (passes 1..4096; the first call starts at 0, a further
 * one where the last ended).  One lane per subsequence.  Pass 0: every lane decodes from its nominal first bit in state
 * (block 0 of the MCU, zigzag index 0) -- true of an interval's first subsequence only -- until it has stepped past its
 * end, and records where (bit position, block of the MCU, zigzag index) and how many blocks it completed.  Pass q: lane i
 * starts from lane i-1's record of pass q-1.  A pass that changes no record has reached the fixed point, which by induction
 * from each interval's first lane is the serial decode; every later pass leaves at once.  A lane stops where a code plus
 * its extra bits would pass the interval's end.  A lane that started at a wrong bit meets things no valid stream holds and
 * has to find the true walk all the same, so it notes them in its record and goes on: an unassigned code is passed over
 * by one bit, a size above 11 (DC) / 10 (AC) is taken as it is, an index past 63, a ZRL past the block's end or an EOBn
 * ends the block.  The note is not part of the state the next lane starts from; at the fixed point every lane started
 * from the true state, and a note still set is error bit 8 (stage 3 reports it).  The host reads the status block to learn whether more passes are needed
 * (never more than the subsequences of the longest interval, plus the one that finds nothing changed). */
int sp_jpeg_decode_sync(const void *plan, const void *plan_dev, void *ws, size_t ws_bytes, int first_pass, int passes, void *stream);
/* 3. Coefficients; last_pass is the last pass enqueued.  Does nothing unless the fixed point is reached (status [10] stays
 * 0).  Exclusive scan of the lanes' block counts; an interval whose chain is not exactly its MCUs x blocks per MCU sets
 * error bit 16; the lanes walk once more and store (every store guarded by its interval's last block and by the index
 * 0..63); then a segmented scan per component turns DC differences into values: predictors 0 at every interval start,
 * sums in 32 bits, clamped to int16. */
int sp_jpeg_decode_coefficients(const void *plan, const void *plan_dev, void *ws, size_t ws_bytes, int last_pass, void *coef,
                                void *stream);
/* 4. Pixels: coef -> rgb uint8 [h][w][3].  Per block, in integers: a coefficient times its table entry, then libjpeg's
 * accurate inverse DCT (jidctint): constants of 13 fraction bits (0.298631336 = 2446 ... 3.072711026 = 25172), the column
 * pass first, descaled by 11 bits (two extra bits kept), then the row pass, descaled by 18, plus 128, through libjpeg's
 * range table (a clamp to 0..255 for values within +-512 of it).  Chrominance is upsampled with libjpeg's triangle filter
 * at the component's own size cw x ch = ceil(w/2) x ceil(h/2 or h), edges replicated there and not at the MCU grid:
 *   2x1: out[2i] = (3 c[i] + c[i-1] + 1) >> 2,  out[2i+1] = (3 c[i] + c[i+1] + 2) >> 2,  out[0] = c[0], out[2cw-1] = c[cw-1]
 *   2x2: s[i] = 3 c[j][i] + c[j'][i], j' = j-1 for an even output row and j+1 for an odd one (clamped to 0..ch-1);
 *        out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4, at the two ends (4 s[i] + 8 or 7) >> 4
 * and where cw <= 2 samples are repeated instead, as libjpeg does.  Then JFIF's conversion in 16-bit fixed point:
 *   R = Y + ((91881 Cr' + 32768) >> 16)        G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16)
 *   B = Y + ((116130 Cb' + 32768) >> 16)       Cb' = Cb - 128, Cr' = Cr - 128, clamped to 0..255. */
int sp_jpeg_decode_pixels(const void *plan, const void *plan_dev, void *ws, size_t ws_bytes, const void *coef, void *rgb,
                          void *stream);

/* ---------------------------------------------------------------------------------------------
 * Animated GIF of uint8 frames that are in device memory (the reference's save_gif hands its frames to imageio:
 * scripts/generate_video_demo.py:212-222 there).  Two stages: a 256-colour palette and the pixels' indices per
 * frame, then the LZW-coded image data of the frame's image block.  Headers, extensions, descriptors and the trailer are
 * written by the host.  h and w are 1..65535 (what a descriptor can say) with h*w <= 2^24 (the per-bin channel sums stay
 * inside 32 bits); strip_rows >= 1 (a value above h means h).  The size functions need no GPU and give 0 for arguments the
 * calls refuse.
 * ------------------------------------------------------------------------------------------- */
/* Scratch of both calls for n frames: per frame the histogram (32^3 bins x two 64-bit words), four summed-volume tables of
 * 33^3 words and the bin -> index table; then, for the LZW stage, three int32 arrays and a staging slot per (frame, strip)
 * of the strip's worst case in whole words plus one.  The two stages use disjoint parts. */
size_t sp_gif_ws_bytes(int n, int h, int w, int strip_rows);
/* Bytes of image data no frame can exceed.  Bits: the opening CLEAR, 9; at most one code per pixel of at most 12 bits; a
 * CLEAR of 12 bits whenever 3838 codes have filled a dictionary, at most floor(h*w / 3838) of them; one CLEAR or EOI of at
 * most 12 bits per strip, strips = ceil(h / strip_rows):
 *   bytes = ceil((9 + 12*h*w + 12*floor(h*w / 3838) + 12*strips) / 8),   result = 1 + bytes + ceil(bytes / 255) + 1
 * (the minimum code size in front, a length byte per sub-block of 255, the terminator). */
size_t sp_gif_stream_bytes(int h, int w, int strip_rows);
/* frames: uint8 [n][h][w][3] RGB -> palette: uint8 [n][256][3], indices: uint8 [n][h][w].  Integer arithmetic only.  Per frame:
 *   histogram  32 x 32 x 32 bins at (r>>3, g>>3, b>>3), each with its pixel count and the sums of the three 8-bit values;
 *   boxes      a box is an inclusive range of bins per axis, always shrunk to the occupied bins inside it.  From the shrunk
 *              cube, split until there are 256 boxes or none can be split: among the boxes whose longest extent
 *              e = max(hi - lo) is above 0 take the largest count * e (the lowest index among equals); the axis is the first
 *              of R, G, B with extent e; cut after plane lo + c, c the smallest offset with
 *              2 * (pixels in planes lo .. lo+c) >= count, at most e - 1; the lower part keeps the index, the upper part is
 *              appended, both are shrunk;
 *   palette    entry i = (2*sum + count) / (2*count) per channel over box i, integer division; unused entries are 0;
 *   mapping    an occupied bin's colour is its own rounded mean, computed the same way; the bin takes the entry in use with
 *              the least squared distance to it (the lowest index among equals); a pixel's index is its bin's.
 * ws needs the quantiser's part of sp_gif_ws_bytes (any strip_rows), 8-byte aligned. */
int sp_gif_quantise_u8(const void *frames, int n, int h, int w, void *palette, void *indices, void *ws, size_t ws_bytes,
                       void *stream);
/* indices: uint8 [n][h][w] -> for frame i the image data of a GIF image block at out + i*cap and its length in out_len[i]
 * (int32, device): the minimum code size 08, the LZW stream in sub-blocks of at most 255 bytes each behind its length byte,
 * and the terminator 00.  The frame is cut into strips of strip_rows rows (the last may be shorter), each coded with a
 * dictionary of its own, so that the strips can be coded concurrently.  The stream: CLEAR (256) at 9 bits; then the strips in
 * order, each ordinary GIF LZW from an empty dictionary (first free code 258, width 9; after a code is written and its entry
 * made, the width grows when the next free code is above 2^width; when the next free code is 4096, CLEAR is written at 12
 * bits and the dictionary starts again); after a strip's last code comes CLEAR, or EOI (257) after the frame's last strip, at
 * the width in force once that last code's own entry has been counted.  Codes are packed least significant bit first, strips
 * are joined bit by bit, the last byte is padded with zeros.  cap below sp_gif_stream_bytes is refused; bytes of a slot
 * beyond out_len[i] are not written.  ws: sp_gif_ws_bytes, 8-byte aligned. */
int sp_gif_lzw(const void *indices, int n, int h, int w, int strip_rows, void *out, size_t cap, void *out_len, void *ws,
               size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * PNG / APNG frames of uint8 frames that are in device memory (the lossless output: the reference writes frames through
 * imageio / Pillow on the host).  Three stages: the filtered rows of every frame, the complete zlib stream of a frame's
 * filtered bytes, and the files around the streams (sp_png_wrap: signature, chunks and their CRC-32, see sp_crc32_rows; a
 * caller may stop after the second stage and put the chunks together on the host).  The Adler-32 inside the stream covers the
 * filtered bytes, which never leave the device, and is made there.
 * h and w are 1..65535 with h*w <= 2^24; strip_rows >= 1 (a value above h means h).  The size functions need no GPU and give
 * 0 for arguments the kernels refuse.
 * ------------------------------------------------------------------------------------------- */
/* Scratch of the deflate stage for n frames: per (frame, strip) four int32 (bits, bit offset, two Adler partials), an int32
 * per frame, and a staging slot per (frame, strip) of the strip's worst case in whole words plus one. */
size_t sp_png_ws_bytes(int n, int h, int w, int strip_rows);
/* Bytes of zlib stream no frame can exceed.  Bits per strip: a block header of at most
 *   3 + 14 + 19*3 + (286 + 2) * 14 = 4106
 * (BFINAL and BTYPE; HLIT, HDIST, HCLEN; 19 lengths of 3 bits; per code length a run-length symbol of at most 7 bits and at
 * most 7 extra bits), at most 15 bits per token and at most one token per byte (a literal has at most 15 bits; a match has
 * at most 15 + 5 + 1 and covers at least 3 bytes), and an end-of-block code of at most 15 bits.  With strips =
 * ceil(h / strip_rows):
 *   result = 2 + ceil((strips * (4106 + 15) + 15 * h * (1 + 3*w)) / 8) + 4. */
size_t sp_png_stream_bytes(int h, int w, int strip_rows);
/* frames: uint8 [n][h][w][3] RGB -> filtered: uint8 [n][h][1 + 3*w], the rows of an 8-bit RGB image without interlace, each
 * behind its filter type.  Every row takes the type (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth; bpp = 3) with the least sum of
 * min(b, 256 - b) over its filtered bytes, the lowest type among equals.  The row above is the frame's own (zeros above row
 * 0), so every row is independent. */
int sp_png_filter_u8(const void *frames, int n, int h, int w, void *filtered, void *stream);
/* filtered: uint8 [n][h][1 + 3*w] -> frame i's complete zlib stream at out + i*cap, its length in out_len[i] (int32, device):
 * 78 9C, the deflate blocks of the strips joined bit by bit, zero bits up to a byte, the Adler-32 of the frame's filtered
 * bytes, big-endian.  A strip is strip_rows rows, tags included (the last may be shorter), and one dynamic-Huffman block
 * (BTYPE 2); BFINAL is set on the frame's last strip only.  Nothing refers back across the start of a strip.
 *   tokens   the strip's first byte is a literal.  At a later position p, r is the number of bytes from p on that equal byte
 *            p-1, capped at 258 and at the strip's end: r >= 3 gives a match of length r at distance 1 and p += r, else the
 *            literal at p.  (Per run of n equal bytes: a literal, floor((n-1) / 258) matches of 258, then the remainder as a
 *            match if it is at least 3, else as literals.)
 *   codes    literal/length code lengths: plain Huffman over the strip's counts with end-of-block counted once.  The two
 *            least nodes are joined until one is left; nodes are ordered by weight, then by age: the leaves, in order of
 *            (count, symbol), are older than every joined node, and joined nodes age in order of their making.  A code with
 *            fewer than two symbols in use gives count 1 to its lowest unused symbols first.  While a length passes 15,
 *            every non-zero count f becomes (f + 1) >> 1 and the code is made again.  Codes are the canonical ones of RFC
 *            1951 3.2.2.  The distance code is constant: symbols 0 and 1 with one bit each; a match's distance is the bit 0.
 *   header   HLIT and HCLEN trimmed as in RFC 1951, HDIST = 1; the code lengths in zlib's run-length form (16 / 17 / 18;
 *            the literal/length lengths and the two distance lengths are scanned separately); the 19-symbol code by the
 *            same construction with limit 7.
 * Deflate packs least significant bit first; Huffman codes go in most significant bit first.  cap below
 * sp_png_stream_bytes is refused; bytes of a slot beyond out_len[i] are not written.  ws: sp_png_ws_bytes, 8-byte aligned. */
int sp_png_deflate(const void *filtered, int n, int h, int w, int strip_rows, void *out, size_t cap, void *out_len, void *ws,
                   size_t ws_bytes, void *stream);
/* Bytes no still file can exceed: sp_png_stream_bytes + 57 (signature 8, IHDR 25, IDAT 12 around its payload, IEND 12). */
size_t sp_png_file_bytes(int h, int w, int strip_rows);
/* Bytes no animation of n frames can exceed, S = sp_png_stream_bytes: signature 8, IHDR 25, acTL 20, IEND 12, per frame an
 * fcTL of 38 and a data chunk of 12 + S, and 4 more in each of the n - 1 fdAT:
 *   result = 65 + n * (50 + S) + 4 * (n - 1);  0 for n <= 0. */
size_t sp_apng_file_bytes(int n, int h, int w, int strip_rows);
/* Scratch of sp_png_wrap for n streams in slots of cap bytes: 16 bytes per frame (the stream's place, the seed and the CRC of
 * its chunk) rounded up to 256, and sp_crc32_ws_bytes(n, cap). */
size_t sp_png_wrap_ws_bytes(int n, size_t cap);
/* streams: n zlib streams as sp_png_deflate leaves them (stream i at streams + i*cap, lens[i] bytes of it, int32 on the
 * device; a length outside 0..cap counts as the nearer end) -> complete files, made on the device from the first byte to the
 * last.  8-bit RGB without interlace, h x w.
 *   animate == 0   slot i of files (at files + i*file_cap) is one still: signature, IHDR, one IDAT (length, type, stream i,
 *                  CRC-32 over type and stream), IEND; file_len[i] = lens[i] + 57.  file_cap >= cap + 57.
 *   animate != 0   files is ONE animated PNG that loops for ever: signature, IHDR, acTL (n frames, num_plays 0); per frame an
 *                  fcTL (sequence number, the whole frame at offset 0, delay delay_num / delay_den seconds, dispose 0, blend
 *                  0) and its stream, in IDAT for frame 0 and in fdAT behind a sequence number for the others; IEND.
 *                  Sequence numbers count the fcTL and fdAT chunks in file order from 0 (frame i > 0: fcTL 2i - 1, fdAT 2i).
 *                  file_len[0] is the file's length; the frames' places are an exclusive sum of the lengths made on the
 *                  device.  file_cap >= 65 + n * (50 + cap) + 4 * (n - 1) <= 2^31 - 1.  delay_num is 1..65535, delay_den
 *                  0..65535 (which the format reads as 100).
 * Either way the bytes equal those the host puts together from the same streams (image_io.png_file / write_apng); bytes of a
 * file (slot) beyond file_len are not written.  file_len: int32 [n] on the device (animate: only [0] is written).  ws:
 * sp_png_wrap_ws_bytes, 8-byte aligned.  Nothing about the lengths reaches the host. */
int sp_png_wrap(const void *streams, size_t cap, const void *lens, int n, int h, int w, int animate, int delay_num, int delay_den,
                void *files, size_t file_cap, void *file_len, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * CRC-32 of rows of bytes in device memory: the checksum of PNG chunks, gzip and zip (reflected polynomial 0xEDB88320; seed
 * and result in zlib's convention: crc[i] == zlib.crc32(row_i[:lens[i]], seed[i])).  Row i is data + i*pitch, of which the
 * first lens[i] bytes count; pitch is 1..2^31-1 and need not be a multiple of 4.  lens (int32 [n]) is read on the device: a
 * negative length counts as 0 and one above pitch as pitch, so that nothing outside a row is read; a length of 0 gives
 * seed[i].  seed: uint32 [n] on the device, or NULL for 0.  crc: uint32 [n].  The work is parallel within a row (pieces of 64
 * bytes, each piece's register multiplied by x^(8 * bytes behind it) mod P, all XORed), so one long row is as good as many.
 * ------------------------------------------------------------------------------------------- */
/* Scratch: one uint32 per (row, span of 16384 bytes of pitch); 0 for arguments the kernel refuses. */
size_t sp_crc32_ws_bytes(int n, size_t pitch);
int sp_crc32_rows(const void *data, size_t pitch, const void *lens, const void *seed, int n, void *crc, void *ws,
                  size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Lossless WebP of uint8 frames that are in device memory (the full-colour animated output: still .webp files and one
 * animated .webp).  Two stages: the transforms of every frame (subtract green, spatial prediction), then the complete VP8L
 * bitstream of a frame from its signature byte 0x2f on.  The RIFF container around it (RIFF / WEBP / VP8L, and VP8X / ANIM /
 * ANMF for an animation) has no checksum and is host work.  h and w are 1..16384 (the format's 14-bit fields) with
 * h*w <= 2^24; pred_bits is 2..9; group_bits is 0 or 2..9.  The size functions need no GPU and give 0 for arguments the
 * kernels refuse.
 * ------------------------------------------------------------------------------------------- */
/* Scratch for n frames: two uint64 sums per frame (all that the transform stage uses), per segment of the stream (2 + 2G per
 * frame, G = groups) two int32 (bits, bit offset), and a staging slot per segment of its worst case in whole words plus two. */
size_t sp_webp_ws_bytes(int n, int h, int w, int pred_bits, int group_bits);
/* Bytes of VP8L stream no frame can exceed.  A prefix code's header is at most 4 bits in the simple form with a 1-bit symbol,
 * 11 with an 8-bit symbol, and in the normal form 1 + 4 + 19*3 + 1 + 14*A for an alphabet of A symbols (the form bit, the
 * count of 19-symbol lengths, those lengths, the max_symbol bit, per code length a run-length symbol of at most 7 bits and at
 * most 7 extra bits): 3983 for green's 280, 3647 for 256.  The main image's alpha is always 0 and its distance symbol always
 * 1, so those two codes are simple and cost no bits per token; a group's five codes take at most
 *   3983 + 2*3647 + 4 + 4 = 11285
 * bits, and a token at most 45 per pixel (a literal: three codes of at most 15 bits; a copy: 15 + 10 extra bits for at least
 * 3 pixels).  A sub-image (the mode image, the entropy image) has blue 0 and alpha 255 throughout: its codes take at most
 *   3983 + 3647 + 4 + 11 + 4 = 7649
 * bits and a token at most 30.  With bh x bw blocks of 2^pred_bits, G = ceil(h / 2^group_bits) groups and
 * E = ceil(w / 2^group_bits) (G = 1 and no entropy image for group_bits = 0):
 *   bits = 40 + 3 + 6 + 1 + 7649 + 30*bh*bw          signature and sizes, subtract green, predictor, cache bit, mode image
 *        + 3                                         no more transforms, no colour cache, entropy image or not
 *        + (3 + 1 + 7649 + 30*G*E  if group_bits)    its block size, its cache bit, the entropy image
 *        + G*11285 + 45*h*w
 *   result = ceil(bits / 8). */
size_t sp_webp_stream_bytes(int h, int w, int pred_bits, int group_bits);
/* frames: uint8 [n][h][w][3] RGB -> flags: int32 [n], modes: uint8 [n][bh][bw] (bh = ceil(h / 2^pred_bits), bw likewise),
 * residual: uint8 [n][h][w][4], per pixel the residual bytes of B, G, R and of alpha, which is always 0.
 *   flags    1 if green is taken out of red and blue before the prediction.  Over the frame, sum min(d, 256 - d) of the
 *            left-neighbour differences d (mod 256) of the R and B bytes, once of R - G and B - G and once of R and B as they
 *            are, in 64 bits; the flag is set when the first sum is the smaller one (ties take the plain form).
 *   modes    pixels are ARGB with A = 255.  A block of 2^pred_bits pixels square takes, of the format's 14 predictors, the
 *            one with the least sum of min(b, 256 - b) over its residual bytes, the lowest among equals (the first row and
 *            column of the frame have the same residuals under every mode).  Edges are the format's: the top-left pixel
 *            predicts 0xff000000, the top row L, the left column T, and the top-right neighbour of a row's last pixel is
 *            the first pixel of the current row.  Predictor 13's (a - TL) / 2 truncates toward zero.
 * ws: at least 16*n bytes, 8-byte aligned (sp_webp_ws_bytes covers it). */
int sp_webp_transform_u8(const void *frames, int n, int h, int w, int pred_bits, void *residual, void *modes, void *flags,
                         void *ws, size_t ws_bytes, void *stream);
/* residual, modes, flags as above (a residual's alpha byte is ignored and coded as 0) -> frame i's complete VP8L stream at
 * out + i*cap, its length in out_len[i] (int32, device).  In order: the signature 0x2f, w-1 and h-1 in 14 bits each, alpha 0,
 * version 0; the subtract-green transform if flags[i]; the predictor transform with its mode image (the mode in green,
 * alpha 255) as a sub-image with one code set; no further transform; the main image without colour cache.  For group_bits > 0
 * an entropy image of blocks of 2^group_bits gives every block of block row g the group g (green = g & 255, red = g >> 8,
 * alpha 255), so that a frame is coded in strips of 2^group_bits rows, each with five prefix codes of its own; group_bits = 0
 * is one group and no entropy image.  All groups' codes come first, then the strips' pixels in order.
 *   tokens   as sp_png_deflate's, in pixels: a strip's (or sub-image's) first pixel is a literal.  At a later position p, r is
 *            the number of pixels from p on that equal pixel p-1, capped at 4096 and at the strip's end: r >= 3 gives a copy
 *            of length r at distance 1 (plane code 2: distance symbol 1, no extra bits) and p += r, else the literal at p.
 *            Runs of 1 or 2 are literals.  Nothing refers back across the start of a strip; there is no colour cache.
 *   codes    an alphabet with fewer than two symbols in use, that symbol below 256, takes the simple form with one symbol
 *            (symbol 0 if none is in use) and no bits per token: always so for alpha and distance.  Otherwise a normal code
 *            by sp_png_deflate's construction (plain Huffman with its order of equal weights, count 1 for the lowest unused
 *            symbols of a one-leaf code, halving while a length passes 15, canonical codes), its lengths for the whole
 *            alphabet (max_symbol unused) in zlib's run-length form (16 / 17 / 18) under a 19-symbol code of the same
 *            construction with limit 7, whose lengths are sent in the format's order, trailing zeros trimmed down to 4.
 * Bits are packed least significant first; Huffman codes go in most significant bit first; the last byte is padded with
 * zeros.  cap below sp_webp_stream_bytes is refused; bytes of a slot beyond out_len[i] are not written.  ws:
 * sp_webp_ws_bytes, 8-byte aligned. */
int sp_webp_code(const void *residual, const void *modes, const void *flags, int n, int h, int w, int pred_bits, int group_bits,
                 void *out, size_t cap, void *out_len, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Frames between the frames: one round doubles the frame rate of uint8 frames that are in device memory (n frames become
 * 2n - 1: out[2i] = frames[i], out[2i + 1] the motion-compensated midpoint of the pair (i, i + 1)).  The reference leaves
 * this to a separate tool behind its mp4.  Classical and all-integer: a bilateral block motion search, a vector median, an
 * overlapped blend; tests/interp_model.py states it in numpy and the kernels equal it bit for bit.  n is 2..32768; h and w
 * are multiples of 8 from 16 to 16384; range is 1..24; lam is 0..255.
 *   luma     Y = (77 R + 150 G + 29 B + 128) >> 8
 *   search   per pair (A, B) and 8x8 block (by, bx) of the midpoint's grid, over all v = (vy, vx) in [-range, range]^2:
 *              cost(v) = sum_q |YA[clamp(q - v)] - YB[clamp(q + v)]| + lam * (|vy| + |vx|)
 *            q over the 16x16 window with origin (8 by - 4, 8 bx - 4), unclamped; clamp acts once, on the displaced
 *            coordinate, per axis, to the image.  key(v) = cost * 4096 + ((vy + range) * (2 range + 1) + (vx + range)); the
 *            block's raw vector is the v of least key (cost < 2^17 and the index < 2^12: a key fits 32 bits and the least
 *            is unique whatever the order of reduction).
 *   median   the component-wise 5th smallest over the 3x3 neighbourhood of raw vectors, block coordinates clamped to the grid
 *   blend    pixel (y, x): ty = y + 4, by0 = (ty >> 3) - 1, wy1 = 2 (ty & 7) + 1, wy0 = 16 - wy1, likewise x; over the four
 *            blocks (by0 + {0, 1}, bx0 + {0, 1}) clamped to the grid, with weights wy * wx (they sum to 256):
 *              out_c = (sum_k w_k * (A_c[clamp(p - v_k)] + B_c[clamp(p + v_k)]) + 256) >> 9
 * ------------------------------------------------------------------------------------------- */
/* Scratch of sp_interp_motion_u8: n luma planes of (h + 2 range + 8) rows of w + 2 range + 8 bytes rounded up to 4 (replicate
 * padding by range + 4, so that the search reads without clamping), the sum rounded up to 16, and the raw vectors,
 * 4 (n - 1) (h / 8) (w / 8) bytes.  Needs no GPU; 0 for arguments the calls refuse. */
size_t sp_interp_ws_bytes(int n, int h, int w, int range);
/* frames: uint8 [n][h][w][3] RGB -> vectors, and raw_vectors unless it is NULL: int16 [n - 1][h / 8][w / 8][2] in (vy, vx)
 * order, after and before the median.  Three launches: the luma of all n frames, the search of all n - 1 pairs, the median.
 * ws: sp_interp_ws_bytes, 4-byte aligned. */
int sp_interp_motion_u8(const void *frames, int n, int h, int w, int range, int lam, void *vectors, void *raw_vectors, void *ws,
                        size_t ws_bytes, void *stream);
/* frames and vectors as above -> out: uint8 [2n - 1][h][w][3], the copies of the frames and the midpoints between them.  A
 * vector may be any int16: reads are clamped to the image.  out may not overlap frames. */
int sp_interp_compensate_u8(const void *frames, int n, int h, int w, const void *vectors, void *out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement aid (bench.py `roofline.clock_ghz_live`; the reference has no counterpart -- its benchmark reads no clocks,
 * /root/reference/src/modes/benchmark.py:170-262).  One time stamp in stream order: `blocks` one-wave workgroups each write
 * four u64 words to out[block][4]: the id of the place the workgroup ran on (bits 3:0 the XCD, HW_REG_XCC_ID; bits 11:4 the
 * CU within it, HW_REG_HW_ID's CU, array and shader engine), the shader-clock counter (s_memtime), the constant 100 MHz
 * counter (s_memrealtime), and 1.  Two stamps taken on the same CU before and after a stretch of work give the shader clock
 * held in between: GHz = 0.1 * (shader ticks) / (100-MHz ticks); the counters of two CUs need not share an origin.
 * ------------------------------------------------------------------------------------------- */
int sp_clock_stamp(void *out, int blocks, void *stream);

/* ---------------------------------------------------------------------------------------------
 * DummyUNet (simulator-path model, /root/reference/src/models/dummy_unet.py:37-59), fp32 NCDHW:
 * out = x + gain*Conv3d(SiLU(Conv3d(x))) + LayerNorm_C(x).  hidden: scratch [B][hidden][F][H][W].
 * ------------------------------------------------------------------------------------------- */
int sp_dummy_unet_f32(const float *x, float *out, float *hidden, const float *w1, const float *b1,
                      const float *w2, const float *b2, const float *ln_w, const float *ln_b,
                      float ln_eps, int use_ln, float gain, int b, int c, int hidden_c, int frames,
                      int h, int w, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SVDPIPE_H */
