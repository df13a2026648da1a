/*
 * pairnet_hip.h -- C ABI of libpairnet_hip.so: hand-written gfx950 (MI355X) kernels
 * for the Pair-Net inference hot path.
 *
 * Conventions (SURVEY.md 8b "operator-level boundary"):
 *   - every entry point is extern "C", returns a hipError_t value as int (0 = ok;
 *     -1 = argument contract violated, nothing launched);
 *   - plain device pointers + sizes, no torch types; `stream` is a hipStream_t;
 *   - no allocation, no global state, caller-owned buffers, re-entrant per stream,
 *     asynchronous (the caller synchronises), graph-capturable;
 *   - all floating-point data is fp32 (the reference runs fp32, no AMP:
 *     configs/mask2former/pairnet.py has no fp16 key); indices are int64, as torch
 *     produces them; token / pixel tensors are channel-last ("token-major").
 *
 * The reference has exactly one native operator boundary on this path, the
 * third-party mmcv extension `ms_deform_attn_forward` (reached from
 * configs/mask2former/pairnet.py:43-54 via pairnet_head.py:94,262); every other
 * native kernel it runs is an ATen/cuDNN/cuBLAS kernel behind a torch call.  Each
 * entry below names the reference call site(s) (file:line under /root/reference)
 * whose arithmetic it replaces.  INTEGRATION.md shows the reference-side binding.
 */
#ifndef PAIRNET_HIP_H_
#define PAIRNET_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PN_ABI_VERSION 34
int pn_abi_version(void);

/* ------------------------------------------------------------------------- *
 * Dense contraction (f32 MFMA 32x32x2, exact fp32 accumulate)
 *   C[z][m][n] = act( sum_k (A[z][m][k] + Aadd[m % aadd_rows][k]) * W[z][n][k]
 *                     + bias[n] ) + Res[z][m][n]
 * Replaces every nn.Linear / 1x1 Conv2d / einsum / matmul on the path:
 *   pairnet_head.py:240-243 (cls_embed, mask_embed, einsum "bqc,bchw->bqhw"),
 *   :323-327 (sub/obj MLPs, importance matmul), :378 (rel_cls_embed), the packed
 *   in_proj / out_proj of nn.MultiheadAttention and the FFNs behind :302-312 and
 *   :367-376, and the pixel decoder's value_proj / sampling_offsets /
 *   attention_weights / output_proj / FFN / 1x1 convs behind :262.
 * `Aadd` fuses the positional add the reference does before a projection
 * (query + query_pos, key + key_pos: facebook_detr.py:329-332).
 * ------------------------------------------------------------------------- */
#define PN_GEMM_RELU       1   /* act = ReLU (else identity)                        */
#define PN_GEMM_A_COLMAJOR 2   /* A is stored [K][lda] (an NCHW feature map)        */
#define PN_GEMM_FORCE_TILE 4   /* testing: force the 128x128 tile of the LDS kernel (128x64
                                * where aadd_from_col is an odd multiple of 64)      */
#define PN_GEMM_FORCE_SKINNY 8 /* testing: force the 32x32 split-K-in-block kernel  */
#define PN_GEMM_FORCE_TILE64 16     /* tuning: 64x64 tile (row-major A)             */
#define PN_GEMM_FORCE_TILE128x64 32 /* tuning: 128x64 tile                          */
#define PN_GEMM_RELU_AFTER_RES 128  /* ReLU after the residual add: relu(act(..)+Res)  */
#define PN_GEMM_GELU 256           /* act = exact (erf) GELU; Swin FFN                  */
/* Scheduling hint carried PER CALL in `flags` (performance only, results unchanged): leave
 * `n` (a multiple of 8, < 8192) of the persistent tile kernels' resident workgroup slots
 * unoccupied, so that the small latency-bound kernels of a concurrent stream (the query
 * chains) find a free slot without waiting for a kernel boundary.  There is no
 * process-wide knob: two callers in one process cannot change each other's grids. */
#define PN_GEMM_RESERVE_SHIFT 16
#define PN_GEMM_RESERVE(n) ((((n) / 8) & 0x3ff) << PN_GEMM_RESERVE_SHIFT)
/* Tuning: force the number of K slices of the split-K path (1 = never split; 0 = the
 * library's own choice; needs splitk_scratch). */
#define PN_GEMM_KSPLIT_SHIFT 26
#define PN_GEMM_KSPLIT(n) (((n) & 31) << PN_GEMM_KSPLIT_SHIFT)

typedef struct pn_gemm_desc {
  const float* A;     int64_t lda;    int64_t strideA;    /* [M][K] (or [K][M])    */
  const float* Aadd;  int64_t ldaadd; int32_t aadd_rows;  /* optional, may be NULL */
  int32_t aadd_from_col;  /* Aadd only feeds output columns >= this (multiple of 64;
                             0 = all): one GEMM for [value_proj | offsets+logits]       */
  const float* W;     int64_t ldw;    int64_t strideW;    /* [N][K]                */
  const float* bias;                                      /* [N] or NULL           */
  const float* Res;   int64_t ldres;  int64_t strideRes;  /* optional residual     */
  float*       C;     int64_t ldc;    int64_t strideC;    /* [M][N]                */
  int32_t M, N, K, batch, flags;
  /* optional split-K workspace (NULL = never split): problems whose M x N gives too few
   * 64x64 tiles to fill 256 CUs (the backbone's late stages, the C5/C4 input convs)
   * contract K in up to 16 slices into this scratch and sum them in slice order */
  float* splitk_scratch;  int64_t splitk_scratch_floats;
} pn_gemm_desc;

int pn_gemm_f32(const pn_gemm_desc* d, void* stream);

/* `count` (<= 18) independent row-major problems in ONE launch of the persistent 64x64
 * tile kernel (all their tiles share the grid): used for the 18 key/value projections of
 * the 9 decoder layers, whose per-problem tile counts do not fill 256 CUs evenly.  Every problem
 * needs K >= 32 (the tile kernel stages 32 columns of a row at a time); else PN_BAD_ARG. */
int pn_gemm_group_f32(const pn_gemm_desc* d, int count, void* stream);

/* Resident workgroups per CU the persistent 64x64-tile kernel (plain row-major A) is sized
 * for: pn_gemm_grid_size(d) = min(tiles, CUs * this - reserved slots) rounded to 8. */
int pn_gemm_wgs_per_cu(void);

/* Which kernel pn_gemm_f32 would launch for `d` (for profiling / roofline
 * attribution; +1 = the column-major-A instantiation). */
#define PN_GEMM_VARIANT_SKINNY        0  /* k_gemm_skinny<A>                 */
#define PN_GEMM_VARIANT_TILE_128x64   2  /* k_gemm_tile<128,64,64,32,A>      */
#define PN_GEMM_VARIANT_TILE_128x128  4  /* k_gemm_tile<128,128,64,64,A>     */
#define PN_GEMM_VARIANT_TILE_64x64    6  /* k_gemm_tile<64,64,32,32,A> (default) */
int pn_gemm_variant(const pn_gemm_desc* d);
/* Workgroups the persistent 64x64 tile kernel is launched with for `d` (introspection: a
 * function of the descriptor alone, PN_GEMM_RESERVE included). */
int pn_gemm_grid_size(const pn_gemm_desc* d);

/* Implicit-GEMM KHxKW convolution, stride 1, zero padding, channel-last:
 *   out[b][y][x][co] = act(sum_{ky,kx,ci} in[b][y+ky-pad][x+kx-pad][ci]
 *                          * Wp[co][(ky*KW+kx)*Cin+ci] + bias[co])
 * Replaces the pixel decoder's 3x3 output conv (behind pairnet_head.py:262) and
 * the 64->64 7x7 layer of the Matrix Learner (cnn_factory.py:31-41).
 * Cin % 32 == 0. */
int pn_conv2d_nhwc_f32(const float* in, const float* Wp, const float* bias,
                       float* out, int B, int H, int W, int Cin, int Cout,
                       int KH, int KW, int pad, int relu, int flags /* 0, PN_GEMM_FORCE_TILE*,
                       PN_GEMM_RESERVE(n) */, void* stream);

/* Winograd F(2x2, 3x3) form of the same 3x3 "same" convolution (C % 4 == 0; odd H / W: the
 * last tile row / column is padded with zeros and clipped), T = B*ceil(H/2)*ceil(W/2) tiles:
 *   pn_winograd_f23_input_f32:  V [16][T][Cin]  = B^T d B of every 4x4 patch
 *   16 GEMMs (one batched pn_gemm_f32 call, batch = 16):  M_xi = V_xi . U_xi^T with
 *       U [16][Cout][Cin] = G g G^T of the weights (computed once by the caller)
 *   pn_winograd_f23_output_f32: out [B][H][W][Cout] = act(A^T M A + bias)
 * 2.25x fewer multiplications than the direct form; fp32, differs from it by fp32
 * re-association only. */
int pn_winograd_f23_input_f32(const float* in, float* V, int B, int H, int W, int C,
                              void* stream);
int pn_winograd_f23_output_f32(const float* M, const float* bias, float* out, int B, int H,
                               int W, int C, int relu, void* stream);
/* Weight transform U = G g G^T of a 3x3 convolution weight w [Co][Ci][3][3] on the device (double
 * arithmetic, rounded once): form 2 -> F(2x2,3x3), U [16][Co][Ci]; form 4 -> F(4x4,3x3), U [36][Co][Ci]
 * (what pn_conv3x3_winograd* take).  Used at pack time and after every optimizer step of a trained
 * backbone. */
int pn_winograd_weights_f32(const float* w, float* U, int Co, int Ci, int form, void* stream);
/* F(4x4, 3x3): 36 positions (V, M: [36][B*ceil(H/4)*ceil(W/4)][C], U [36][Cout][Cin]), 4x fewer
 * multiplications than the direct form; any H, W (edge tiles are padded / clipped).  Its
 * transform constants (up to 8 and 1/24) cost about one more decimal digit than F(2x2). */
int pn_winograd_f43_input_f32(const float* in, float* V, int B, int H, int W, int C,
                              void* stream);
int pn_winograd_f43_output_f32(const float* M, const float* bias, float* out, int B, int H,
                               int W, int C, int relu, void* stream);

/* ------------------------------------------------------------------------- *
 * Backbone: ResNet-50, style "pytorch", frozen BatchNorm
 * (configs/mask2former/pairnet.py:9-19; mmdet's ResNet is third-party, restated in
 * oracle/backbone.py).  BatchNorm is folded into the convolution weights / bias by the
 * caller; activations are channel-last.
 * ------------------------------------------------------------------------- */
/* General form of the convolution above: stride >= 1, 0 <= 2 pad <= min(KH, KW) - 1 (a larger
 * pad is refused with PN_BAD_ARG: the loader reads the pixel (oy stride, ox stride) in place of a
 * tap outside the image, which must itself lie inside it),
 *   Ho = (H + 2 pad - KH) / stride + 1 (same for W),
 *   out = [relu_after](act(conv + bias) + res),  res/out [B][Ho][Wo][Cout],
 * flags: PN_GEMM_RELU (act), PN_GEMM_RELU_AFTER_RES, tile selectors, PN_GEMM_RESERVE(n),
 * PN_GEMM_KSPLIT(n). */
int pn_conv2d_nhwc_ex_f32(const float* in, const float* Wp, const float* bias,
                          const float* res, float* out, int B, int H, int W, int Cin,
                          int Cout, int KH, int KW, int stride, int pad, int flags,
                          float* splitk_scratch /* or NULL */,
                          int64_t splitk_scratch_floats, void* stream);
/* Output of the FIRST bottleneck of a stage (the one with a projection shortcut) in one launch:
 *   out = relu(t2 . W3^T + b3 + (x[:, ::stride, ::stride] . Wsc^T + bsc))
 * x [B][H][W][Cin] (the block input), t2 [B][Ho][Wo][planes] (the 3x3 convolution's output),
 * Wsc [Cout][Cin], W3 [Cout][planes], out [B][Ho][Wo][Cout], Ho = (H - 1) / stride + 1; Cin and
 * planes % 32 == 0.  Bit for bit the result of the two launches it replaces (pn_gemm_f32 /
 * pn_conv2d_nhwc_ex_f32 for the shortcut into `idt`, pn_gemm_f32 with Res = idt for conv3): each
 * tile contracts the shortcut, keeps acc + bias in registers, clears the accumulators and
 * contracts conv3; `idt` is not touched.  Where the library's rules would give either of the two
 * launches, or this one, the split-K path or the skinny kernel, the two launches are issued
 * instead and `idt` [B][Ho][Wo][Cout] is their intermediate (it may be NULL only if that cannot
 * happen).  flags: PN_GEMM_RESERVE(n), PN_GEMM_KSPLIT(n). */
int pn_bottleneck_proj_f32(const float* x, const float* Wsc, const float* bsc, const float* t2,
                           const float* W3, const float* b3, float* idt, float* out, int B,
                           int H, int W, int Cin, int planes, int Cout, int stride, int flags,
                           float* splitk_scratch /* or NULL */, int64_t splitk_scratch_floats,
                           void* stream);
/* Grouped 3x3 convolution, pad 1 (zeros outside the image), stride 1 or 2, channel-last: conv2 of
 * the ResNeXt bottlenecks.  The reference reaches it through mmdet's ResNeXt, configured at
 * configs/deformable_detr/pairnet_rnext101_vg.py:9-21 (type "ResNeXt", groups 32, base_width 8);
 * mmdet is third-party and its layer is restated from memory, unpinned.
 *   out[b][oy][ox][g*Cg + co] = act(sum_{ky,kx,ci} in[b][oy*s+ky-1][ox*s+kx-1][g*Cg + ci]
 *                                   * Wg[g][co][(ky*3+kx)*Cg + ci] + bias[g*Cg + co])
 * in [B][H][W][G*Cg], out [B][Ho][Wo][G*Cg], Ho = (H - 1) / stride + 1 (same for W); Wg
 * [G][Cg][9*Cg] is the PyTorch weight [G*Cg][Cg][3][3] with each row reordered to (ky, kx, ci).
 * Cg in {8, 16, 32, 64}, any G >= 1; KH = KW = 3; stride 1 or 2; flags: 0 or PN_GEMM_RELU; `in`
 * and `Wg` 16-byte aligned; B*H*W*G*Cg < 2^31 (the kernel indexes with int32).  Anything else is
 * PN_BAD_ARG before a launch.  Every output is ONE fixed-order fp32 MFMA chain of 9*Cg products
 * followed by the bias: no atomics, no split, bitwise reproducible.  At Cg = 8 two neighbouring
 * groups share a 16-channel MFMA tile with a block-diagonal weight operand: the other group's
 * inputs meet exact zeros, so a non-finite input there turns this group's outputs into NaN. */
int pn_conv2d_grouped_nhwc_f32(const float* in, const float* Wg, const float* bias, float* out,
                               int B, int H, int W, int G, int Cg, int KH, int KW, int stride,
                               int flags, void* stream);
/* Stem: relu(conv7x7/2 pad 3 (NCHW RGB image) + bias) -> [B][Ho][Wo][64] channel-last.
 * Wp [64][160] = conv1.weight [64][3][7][7] flattened, zero-padded 147 -> 160. */
int pn_stem7x7s2_f32(const float* img_nchw, const float* Wp, const float* bias,
                     float* out, int B, int H, int W, int flags /* 0 or PN_GEMM_RESERVE(n) */,
                     void* stream);
/* F.max_pool2d(x, 3, stride=2, padding=1) on channel-last data, C % 4 == 0. */
int pn_maxpool3x3s2_nhwc_f32(const float* in, float* out, int B, int H, int W, int C,
                             void* stream);

/* ------------------------------------------------------------------------- *
 * Normalisation
 * ------------------------------------------------------------------------- */
/* y[r][:] = LayerNorm(x[r][:]) * gamma + beta, C == 256, eps 1e-5.
 * (norms of BaseTransformerLayer, facebook_detr.py:406-408; post_norm,
 * pairnet_head.py:236.) */
int pn_layernorm_f32(const float* x, const float* gamma, const float* beta,
                     float* y, int64_t rows, int C, float eps, void* stream);

/* The same over rows of any width C % 4 == 0, C <= 3072, with row strides (floats):
 * the norms of the Swin backbone ([3P] mmdet SwinTransformer configured at
 * configs/mask2former/pairnet_swinb.py:203-226: patch_embed.norm, norm1 / norm2 of every
 * block, the output norm of every stage). */
int pn_layernorm_rows_f32(const float* x, int64_t ldx, const float* gamma, const float* beta,
                          float* y, int64_t ldy, int64_t rows, int C, float eps, void* stream);
/* The same LayerNorm written as an S3 operand [rows x C] (three bf16 planes, pn_gemm_s3_f32's A:
 * the Swin blocks' norm1 / norm2 in front of the qkv / FFN GEMMs); C % 16 == 0.  Rows of the last
 * 32-row block beyond `rows` are not written (the GEMM never stores what it computes from them). */
int pn_layernorm_rows_s3_f32(const float* x, int64_t ldx, const float* gamma, const float* beta,
                             void* y_s3, int64_t rows, int C, float eps, void* stream);

/* Swin patch merging up to its Linear: x [B][H*W][C] -> y [B][H2*W2][4C], H2 = ceil(H/2),
 * row (b, y2, x2) = LayerNorm_4C([x(2y2,2x2) | x(2y2,2x2+1) | x(2y2+1,2x2) | x(2y2+1,2x2+1)])
 * with zeros beyond an odd map's edge.  gamma / beta (and the columns of the reduction
 * weight that follows) are in this neighbour-major order: index (row*2+col)*C + c, the
 * permutation of mmdet's nn.Unfold order c*4 + row*2 + col. */
int pn_patch_merge_ln_f32(const float* x, const float* gamma, const float* beta, float* y,
                          int B, int H, int W, int C, float eps, void* stream);

/* Swin patch embedding, im2col half: NCHW RGB image [B][3][H][W] -> rows
 * [B*ceil(H/4)*ceil(W/4)][64], column c*16 + ky*4 + kx (the flattening of the
 * [C][3][4][4] projection weight), columns 48..63 zero, pixels beyond H / W zero (the
 * reference pads bottom / right to a multiple of the patch). */
int pn_patch_im2col4_f32(const float* img, float* out, int B, int H, int W, void* stream);

/* Swin (shifted-)window multi-head attention, head dim 32, on the qkv rows
 * [B*H*W][ldqkv] (q | k | v, each C = heads*32 wide) -> out [B*H*W][ldo]:
 * zero-padding of the map to a multiple of `ws` (padded tokens' q/k/v = qkv_bias, as the
 * reference pads after norm1), cyclic shift by `shift`, window partition, softmax(q k^T *
 * scale + bias_table[head][(dy+ws-1)(2ws-1)+(dx+ws-1)] + (-100 between different
 * wrap-around regions)) v, window merge, un-shift and crop are all index arithmetic.
 * bias_table is [heads][(2ws-1)^2]: the TRANSPOSE of mmdet's
 * relative_position_bias_table parameter.  ws*ws <= 169. */
int pn_window_attention_f32(const float* qkv, int64_t ldqkv, const float* qkv_bias,
                            const float* bias_table, float* out, int64_t ldo, int B, int H,
                            int W, int C, int heads, int ws, int shift, float scale,
                            void* stream);
/* The same with the output written as an S3 operand [B H W x C] (three bf16 planes: the proj GEMM's A
 * operand of pn_gemm_s3_f32, pre-split; bit for bit the split of the fp32 form's output). */
int pn_window_attention_s3_f32(const float* qkv, int64_t ldqkv, const float* qkv_bias,
                               const float* bias_table, void* out_s3, int B, int H, int W, int C,
                               int heads, int ws, int shift, float scale, void* stream);

/* GroupNorm over channel-last x[b][HW][C] with G groups (+ optional ReLU); image b
 * starts at x + b*x_bstride / y + b*y_bstride (floats).  `partials` is caller
 * scratch of B * nblk * G * 2 doubles, nblk = pn_groupnorm_nblk(HW).  (ConvModule norm of the pixel decoder, behind
 * pairnet_head.py:262.) */
int pn_groupnorm_nblk(int64_t HW);
int pn_groupnorm_nhwc_f32(const float* x, const float* gamma, const float* beta,
                          float* y, double* partials, int B, int64_t HW, int C,
                          int G, float eps, int relu, int64_t x_bstride,
                          int64_t y_bstride, void* stream);

/* pn_groupnorm_nhwc_f32 (no ReLU) and the accumulating pn_bilinear_nhwc_f32 behind it in one pass:
 *   y[b][p][:] = GroupNorm(x)[b][p][:] + bilinear-up(coarse [b][hc][wc][C] -> H x W)[p][:]
 * (the FPN's top-down add of the pixel decoder, behind pairnet_head.py:262).  The normalised value
 * and the sample are each rounded as the two kernels round them and then added: bit for bit the
 * result of the pair, with one read and one write of the H x W map instead of two of each.
 * `partials` as above; image b of the coarse map starts at coarse + b*coarse_bstride floats. */
int pn_groupnorm_upadd_nhwc_f32(const float* x, const float* gamma, const float* beta, float* y,
                                double* partials, const float* coarse, int B, int H, int W,
                                int hc, int wc, int C, int G, float eps, int64_t x_bstride,
                                int64_t y_bstride, int64_t coarse_bstride, void* stream);

/* Linear + residual + post-norm of a transformer layer in one launch, N == 256:
 *   y[r][:] = LayerNorm(res[r][:] + x[r][:] W^T + bias) * gamma + beta
 * -- `output_proj` + identity + norms.0, and ffns.0.layers.1 + identity + norms.1, of the
 * pixel decoder's six encoder layers (MultiScaleDeformableAttention.forward /
 * BaseTransformerLayer, [3P] mmcv 1.7.0; configured at configs/mask2former/pairnet.py:40-66,
 * run behind pairnet_head.py:262).  A workgroup owns 32 whole rows, so the pre-norm map never
 * reaches HBM.  Bit for bit pn_gemm_f32 (row-major, residual epilogue) followed by
 * pn_layernorm_f32.  x [M][ldx] (K used), W [256][ldw], res [M][ldres], y [M][ldy]; K % 32 == 0;
 * 16-byte aligned operands, leading dimensions % 4 == 0; y must not alias x.  Meant for
 * chip-filling M (>= 2048 rows: M / 32 workgroups); the query-side chains keep their own
 * kernels. */
int pn_linear_res_ln_f32(const float* x, int64_t ldx, const float* W, int64_t ldw,
                         const float* bias /* nullable */, const float* res, int64_t ldres,
                         const float* gamma, const float* beta, float* y, int64_t ldy,
                         int M, int N, int K, float eps, void* stream);

/* Fused FFN block of a decoder layer for M ~ 100 rows (facebook_detr.py:425-427 +
 * the norm that follows):  y = LayerNorm(x + W2 relu(W1 x + b1) + b2) * gamma + beta.
 * W1 [hidden][256], W2 [256][hidden]; hidden % 64 == 0; scratch =
 * pn_ffn_scratch_floats(M, hidden) floats.  y may alias nothing it reads except x. */
int64_t pn_ffn_scratch_floats(int M, int hidden);
int pn_ffn_ln_f32(const float* x, const float* W1, const float* b1, const float* W2,
                  const float* b2, const float* gamma, const float* beta, float* y,
                  float* scratch, int M, int C, int hidden, float eps, void* stream);
/* The same with a SECOND LayerNorm of the result written to y2 (nullable): the decoder's
 * post_norm that `forward_head` applies to every layer's output (pairnet_head.py:236), bit
 * for bit the arithmetic of pn_layernorm_f32 on y. */
int pn_ffn_ln2_f32(const float* x, const float* W1, const float* b1, const float* W2,
                   const float* b2, const float* gamma, const float* beta, float* y,
                   const float* gamma2, const float* beta2, float* y2, float* scratch, int M,
                   int C, int hidden, float eps, void* stream);

/* y[r][:] = x[r][:] / max(||x[r]||_2, eps)   (F.normalize, pairnet_head.py:325-326) */
int pn_l2normalize_f32(const float* x, float* y, int64_t rows, int C, float eps,
                       void* stream);

/* ------------------------------------------------------------------------- *
 * Multi-scale deformable attention sampling.  THE reference's native boundary:
 * replaces mmcv `ext_module.ms_deform_attn_forward(value, spatial_shapes,
 * level_start_index, sampling_locations, attention_weights, im2col_step)` and
 * fuses what precedes it in MultiScaleDeformableAttention.forward: softmax over
 * the L*P logits and reference_point + offset / (W_l, H_l).
 *   value   [B][N][ld_value]  projected value tokens (first H*D floats of each
 *                             row), levels concatenated
 *   offaw   [B][N][ld_offaw]  raw Linear outputs: H*L*P*2 offsets (x,y) followed
 *                             by H*L*P attention logits
 *   (row strides let both live in one [value | offsets | logits] GEMM output)
 *   out     [B][N][H*D]
 * Queries are the N tokens themselves (encoder self-attention); the reference
 * point of token n is its own pixel centre ((x+.5)/w, (y+.5)/h).
 * H == 8, D == 32, P == 4, L <= 4. */
int pn_msda_f32(const float* value, int64_t ld_value, const float* offaw,
                int64_t ld_offaw, float* out, int B, int L,
                const int32_t* level_h /* host */, const int32_t* level_w /* host */,
                void* stream);
/* The same with a tuning flag: 0 = one workgroup per query pair (what pn_msda_f32 launches);
 * PN_MSDA_PERSISTENT / PN_MSDA_PERSISTENT_BATCHED = persistent workgroups walking their XCD
 * band's query pairs with the next pair's offsets / logits in flight (one / both queries of a
 * pair gathering at a time): measured slower in round 4 (csrc/msda.hip), kept as the A/B.
 * All three give bit-identical output. */
#define PN_MSDA_PERSISTENT 1
#define PN_MSDA_PERSISTENT_BATCHED 2
#define PN_MSDA_LOW_OCCUPANCY 4    /* one-shot form with the compiler's register choice (84 VGPRs, 5
                                      workgroups per CU: rounds 1-3); default: 62 VGPRs, 8 per CU */
#define PN_MSDA_S3_OUT 8           /* `out` is an S3 operand [B * N x 256] (three bf16 planes, see
                                    * pn_gemm_s3_f32): the output_proj GEMM's A operand written pre-split,
                                    * the fp32 map is not written; default (one-shot) form only */
int pn_msda_ex_f32(const float* value, int64_t ld_value, const float* offaw,
                   int64_t ld_offaw, float* out, int B, int L,
                   const int32_t* level_h /* host */, const int32_t* level_w /* host */,
                   int flags, void* stream);

/* The same operator in mmcv's OWN shape -- the entry a maintainer binds behind the
 * unmodified `MultiScaleDeformableAttention.forward` (mmcv/ops/multi_scale_deform_attn.py,
 * `ext_module.ms_deform_attn_forward`, configured at configs/mask2former/pairnet.py:43-54;
 * INTEGRATION.md shows the binding), and the query-side cross-attention of the
 * Deformable-DETR trunk under CrossHeadBBox (pairnet_bbox_head.py:193-359):
 *   value               [B][N][ld_value]      first 8*32 floats of each row
 *   spatial_shapes      [L][2] int64, DEVICE  (H_l, W_l), as mmcv passes them
 *   level_start_index   [L]    int64, DEVICE
 *   sampling_locations  [B][Nq][8][L][4][2]   normalised (x, y) in [0, 1]
 *   attention_weights   [B][Nq][8][L][4]      already soft-maxed
 *   out                 [B][Nq][256]
 * Any number of queries Nq, bilinear sampling with zero padding (grid_sample,
 * align_corners=False).  H == 8, D == 32, P == 4, L <= 4.  (im2col_step is a batching
 * knob of mmcv's CUDA kernel without an arithmetic effect: there is none here.) */
int pn_msda_loc_f32(const float* value, int64_t ld_value, const int64_t* spatial_shapes,
                    const int64_t* level_start_index, const float* sampling_locations,
                    const float* attention_weights, float* out, int B, int N, int Nq, int L,
                    void* stream);

/* Backward of pn_msda_loc_f32, in the shape of mmcv's `ext_module.ms_deform_attn_backward`
 * (mmcv/ops/multi_scale_deform_attn.py, `MultiScaleDeformableAttnFunction.backward`; the second
 * half of the reference's one native boundary -- what the training step of
 * pairnet_head.py:420-757 / tools/train.py:115-241 differentiates through):
 *   grad_output         [B][Nq][256]
 *   grad_value          [B][N][ld_value]   ACCUMULATED into (hardware fp32 atomics): the caller
 *                                          zeroes it first, as mmcv does (zeros_like(value))
 *   grad_sampling_loc   [B][Nq][8][L][4][2]  written
 *   grad_attn_weight    [B][Nq][8][L][4]     written
 * Arithmetic of mmcv's ms_deform_attn_col2im_bilinear (locations outside (-1, H) x (-1, W)
 * contribute nothing); grad_value's summation order is not deterministic (nor is mmcv's), the
 * other two outputs are.  pn_msda_bwd_det_f32 below is the reproducible form. */
int pn_msda_bwd_f32(const float* value, int64_t ld_value, const int64_t* spatial_shapes,
                    const int64_t* level_start_index, const float* sampling_locations,
                    const float* attention_weights, const float* grad_output, float* grad_value,
                    float* grad_sampling_loc, float* grad_attn_weight, int B, int N, int Nq, int L,
                    void* stream);

/* The same backward with a bitwise reproducible grad_value: no floating-point atomics (mmcv's
 * mmcv/ops/csrc/pytorch/cuda/ms_deform_attn_cuda.cu, `ms_deformable_col2im`, adds them with
 * atomicAdd; csrc/msda_grad.hip builds an inverted index per destination instead).  Operands of
 * pn_msda_bwd_f32 plus a caller-owned scratch of at least pn_msda_bwd_det_scratch_bytes(B, N, Nq,
 * L) bytes, 16-byte aligned, which may arrive dirty.  Definition of the result: for every
 * destination (b, token, head) the contributions are the in-map bilinear taps of all (q, l, p)
 * that land on the token (pn_msda_bwd_f32's in-map tests and clamping), taps numbered t = 0..3 in
 * the order (ya,xa), (ya,xb), (yb,xa), (yb,xb); a contribution's id is ((q*L + l)*4 + p)*4 + t and
 * its coefficient coef = w_t * a (bilinear weight times attention weight, one fp32 rounding).
 * Per channel c: acc = 0, then over the destination's contributions in ASCENDING id
 *   acc = fmaf(coef, grad_output[b][q][head*32 + c], acc)
 * and finally grad_value[b][token][head][c] += acc, one read-modify-write by its single owner
 * (so the entry accumulates into a caller-zeroed buffer exactly as mmcv's does); a destination
 * without a contribution is not written.  grad_sampling_loc / grad_attn_weight are overwritten
 * and are bit for bit pn_msda_bwd_f32's.  All launches go on `stream`; nothing is allocated,
 * uploaded or waited for (graph-capturable).  PN_BAD_ARG: whatever pn_msda_bwd_f32 refuses, a
 * NULL, short or misaligned scratch, Nq*L*16, B*Nq*8*L*16 or B*8*N above 2^31 - 1.
 * pn_msda_bwd_det_scratch_bytes returns 0 for such arguments.  Entries added at ABI 34 (adding
 * entries is compatible). */
int64_t pn_msda_bwd_det_scratch_bytes(int B, int N, int Nq, int L);
int pn_msda_bwd_det_f32(const float* value, int64_t ld_value, const int64_t* spatial_shapes,
                        const int64_t* level_start_index, const float* sampling_locations,
                        const float* attention_weights, const float* grad_output,
                        float* grad_value, float* grad_sampling_loc, float* grad_attn_weight,
                        void* scratch, int64_t scratch_bytes, int B, int N, int Nq, int L,
                        void* stream);

/* Diagnostic (bench.py's `roofline_deformable_sampling.gather_peak`): the bare access pattern of
 * the sampling kernels above -- 8 lanes x 16 B per random 128-byte line, 12 independent lines per
 * lane group, no arithmetic but a sum -- over `workgroups` x 256 threads, lines drawn from the
 * first line_mask + 1 (a power of two) lines of `lines`; idx [workgroups][32][12] int32 (any
 * values: masked), out [workgroups][256].  Replaces nothing in the reference: it measures the
 * roof the deformable-attention gather (mmcv ms_deform_attn_forward) sits under here. */
int pn_gather_probe_f32(const float* lines, const int32_t* idx, float* out, int workgroups,
                        int line_mask, void* stream);

/* ------------------------------------------------------------------------- *
 * Positional encoding / resampling
 * ------------------------------------------------------------------------- */
/* out[(y*w+x)][c] = SinePositionalEncoding(num_feats=C/2, normalize=True,
 * temperature, scale=2pi, eps=1e-6)(y,x)[c] + add[c]  (add may be NULL).
 * (pairnet_head.py:278; level_encoding add in the pixel decoder.) */
int pn_sine_pe_f32(float* out, const float* add, int h, int w, int C,
                   float temperature, void* stream);
/* The same with SinePositionalEncoding's `offset` (added to the 1-based row / column index
 * before normalisation; configs/deformable_detr/cross_r101_vg.py:118-120 uses -0.5). */
int pn_sine_pe_offset_f32(float* out, const float* add, int h, int w, int C, float temperature,
                          float offset, void* stream);
/* The same on a padded map: rows >= valid_h / columns >= valid_w are padding
 * (SinePositionalEncoding on a mask: the cumulative sums stop growing there, and the
 * normalisation divides by the valid size). */
int pn_sine_pe_valid_f32(float* out, const float* add, int h, int w, int valid_h, int valid_w,
                         int C, float temperature, float offset, void* stream);

/* Bilinear resize, align_corners=False (F.interpolate semantics).
 * nhwc:   in [b][hi][wi][C] -> out [b][ho][wo][C], out = (accumulate? out:0)+v;
 *         image b at in + b*in_bstride / out + b*out_bstride (floats)
 * planar: in [P][hi][wi]    -> out [P][ho][wo]
 * (FPN top-down add behind pairnet_head.py:262; attention-mask resize :244-246;
 * mask upsampling in _get_bboxes_single :826-843.) */
int pn_bilinear_nhwc_f32(const float* in, float* out, int B, int hi, int wi,
                         int ho, int wo, int C, int accumulate, int64_t in_bstride,
                         int64_t out_bstride, void* stream);
int pn_bilinear_planar_f32(const float* in, float* out, int64_t P, int hi,
                           int wi, int ho, int wo, void* stream);
/* The rows a bilinear resize of a channel-last map reads: out[b][t][p][:] = in[b][tap t of
 * output pixel p][:], t = 0..3 <-> (y0,x0), (y0,x1), (y1,x0), (y1,x1).  As the W operand of the
 * mask-logit GEMM they yield exactly the full-resolution logits `F.interpolate(mask_pred)`
 * reads for a level (pairnet_head.py:244-246) -- Q x 4 N_l instead of Q x H2 W2 per layer;
 * pn_mask_pack_stencil blends, thresholds and packs them. */
int pn_bilinear_stencil_rows_f32(const float* in, float* out, int B, int hi, int wi, int ho,
                                 int wo, int C, int64_t in_bstride, int64_t out_bstride,
                                 void* stream);
/* planar resize + (sigmoid(v) > 0.5  <=>  v > 0) -> uint8 {0,1}  (:834,:842) */
int pn_bilinear_planar_gt0_u8(const float* in, uint8_t* out, int64_t P, int hi,
                              int wi, int ho, int wo, void* stream);
/* The subject / object result masks of one image straight from its mask logits
 * (pairnet_head.py:826-843), without the gathered copies in between:
 *   masks[r]     = resize(mp[clamp(sub_pos[r])]) > 0,  r < R
 *   masks[R + r] = resize(mp[clamp(obj_pos[r])]) > 0
 * mp [Q][hi*wi] fp32; sub_pos / obj_pos int64 [R] on the device, clamped to [0, Q-1] like
 * pn_gather_rows_f32; masks uint8 [2R][ho][wo].  Bit for bit what pn_gather_rows_f32 followed by
 * pn_bilinear_planar_gt0_u8 stores; an object that several slots name is resampled once and
 * stored to each of them.  Q <= 65535, 2R <= 2048.  16-byte stores when wo % 16 == 0 and masks
 * is 16-byte aligned, 4-byte stores when both are multiples of 4, byte stores otherwise. */
int pn_pair_masks_u8(const float* mp, const int64_t* sub_pos, const int64_t* obj_pos,
                     uint8_t* masks, int Q, int R, int hi, int wi, int ho, int wo, void* stream);

/* ------------------------------------------------------------------------- *
 * Attention
 * ------------------------------------------------------------------------- */
/* Bit-pack the boolean attention mask and apply the reference's all-masked fix:
 *   bits[r][w] bit j = (logits[r][32w+j] < 0)   (== sigmoid < 0.5, :256)
 *   rowall[r] = 1 if every one of the Nk keys of row r is masked (:300)
 * logits [R][Nk]; bits [R][nwords], nwords = (Nk+31)/32. */
int pn_mask_pack(const float* logits, uint32_t* bits, int32_t* rowall,
                 int64_t R, int Nk, void* stream);
/* The same from logits4 [R][4][Nk = ho*wo], the four stencil logits per key (tap-major, see
 * pn_bilinear_stencil_rows_f32): bit = (bilinear blend of the four, as pn_bilinear_planar_f32
 * computes it from the (hi, wi) map) < 0.  ho, wo <= 1024. */
int pn_mask_pack_stencil(const float* logits4, uint32_t* bits, int32_t* rowall, int64_t R,
                         int hi, int wi, int ho, int wo, void* stream);

/* The two steps above -- a layer's stencil logits and their blend / threshold / pack -- as ONE
 * launch (round 5): logits = me . rows^T over the level's 4 Nk tap-major stencil rows
 * (pn_bilinear_stencil_rows_f32) on the 64x64 tile loop of pn_gemm_f32 (the same products in
 * the same order: every logit is the bit pattern pn_gemm_f32 would have stored), blended with
 * the single tap_blend definition, thresholded (`< 0`) and bit-packed in the epilogue; the
 * Q x 4 Nk logit map is never written.  Output exactly pn_mask_pack_stencil's: bits
 * [B*Q][ceil(Nk/32)] (padding bits 0), rowall [B*Q] = 1 where every key of the row is masked
 * (set to 1 by a fill launch in front, cleared by any tile that finds an unmasked key).
 *   me [B][Q][ld_me] (K used), rows [B][4*Nk][ld_rows]; (hi, wi) the full-resolution mask map,
 *   (ho, wo) the level's map, Nk == ho * wo; K % 32 == 0.  `flags`: PN_GEMM_RESERVE(n) only.
 * Replaces pairnet_head.py:244-256 (interpolate -> sigmoid < 0.5) + :300 for one layer. */
int pn_mask_stencil_gemm_f32(const float* me, int64_t ld_me, int64_t stride_me, const float* rows,
                             int64_t ld_rows, int64_t stride_rows, uint32_t* bits,
                             int32_t* rowall, int B, int Q, int Nk, int K, int hi, int wi, int ho,
                             int wo, int flags, void* stream);

/* pn_mask_stencil_gemm_f32 without the row copies: `mf` [B][hi*wi][ld_mf] is the full-resolution
 * mask feature itself, and the loader of each 64-column tile computes the row of (tap, key) the
 * way pn_bilinear_stencil_rows_f32 does (make_tap of the key's pixel) and reads it in place --
 * the same K-float rows, hence the same products in the same order and bit-identical bits /
 * rowall; the 4 Nk x K rows per level are neither written nor kept. */
int pn_mask_stencil_gather_gemm_f32(const float* me, int64_t ld_me, int64_t stride_me,
                                    const float* mf, int64_t ld_mf, int64_t stride_mf,
                                    uint32_t* bits, int32_t* rowall, int B, int Q, int Nk, int K,
                                    int hi, int wi, int ho, int wo, int flags, void* stream);

/* softmax(q k^T * scale + mask) v per head, flash-style over key chunks
 * (f32 MFMA for both contractions), then a combine pass.
 *   q [B][Q][ldq], k [B][Nk][ldk], v [B][Nk][ldv]: projected, head h at columns
 *   [32h, 32h+32); out [B][Q][ldo]; 8 heads x 32.
 *   maskbits/rowall from pn_mask_pack (NULL = no mask), shared by the 8 heads.
 *   scratch: pn_attn_scratch_floats(B, Q, Nk) floats.
 * (nn.MultiheadAttention core behind pairnet_head.py:302-312, :367-376.) */
int64_t pn_attn_scratch_floats(int B, int Q, int Nk);
int pn_attention_f32(const float* q, int64_t ldq, const float* k, int64_t ldk,
                     const float* v, int64_t ldv, const uint32_t* maskbits,
                     const int32_t* rowall, float* out, int64_t ldo,
                     float* scratch, int B, int Q, int Nk, float scale,
                     void* stream);

/* ------------------------------------------------------------------------- *
 * Pair Proposal Network
 * ------------------------------------------------------------------------- */
/* Matrix Learner edge layers (cnn_factory.py:22-29, 42-48):
 *   first: in [B][S][S]     -> out [B][S][S][C] = relu(conv7x7(1->C) + b)
 *          w1 [C][49]
 *   last:  in [B][S][S][C]  -> out [B][S][S]    = conv7x7(C->1) + b
 *          w3 [49][C]
 * The C->C middle layer is pn_conv2d_nhwc_f32. */
int pn_mlearner_first_f32(const float* in, const float* w1, const float* b1,
                          float* out, int B, int S, int C, void* stream);
/* Fused front of the PPN (pairnet_head.py:325-333, cnn_factory.py:22-29): per 8 x 8 tile of
 * (subject, object) pairs the L2-normalised query rows its halo needs are staged in LDS,
 * their cosine block is one MFMA tile, and the first Matrix Learner layer is applied to it
 * on chip.  sub_embed / obj_embed [B][Q][256] are the MLP outputs BEFORE F.normalize;
 * importance_raw [B][Q][Q] (the cosine matrix) and c1 [B][Q][Q][64] (first-layer output,
 * ReLU) are written; w1 [64][49], b1 [64].  Equivalent to pn_l2normalize_f32 x 2 +
 * the batched pn_gemm_f32 + pn_mlearner_first_f32. */
int pn_ppn_front_f32(const float* sub_embed, const float* obj_embed, const float* w1,
                     const float* b1, float* importance_raw, float* c1, int B, int Q, float eps,
                     void* stream);
int pn_mlearner_last_f32(const float* in, const float* w3, const float* b3,
                         float* out, int B, int S, int C, void* stream);

/* Top-k pair selection (pairnet_head.py:334-340): for each image the k largest of
 * the n = Q*Q scores, sorted descending; ties broken by the smaller flat index
 * (torch leaves tie order unspecified).  idx/sub/obj [B][k] int64:
 * sub = idx / Q (trunc), obj = idx % Q; pair (nullable) [B][2k] = [sub | obj], the row
 * list of the pair-feature gather (:342-351).  n <= 65536, k <= 256. */
int pn_topk_pairs(const float* scores, int64_t* idx, int64_t* sub, int64_t* obj,
                  int64_t* pair, int B, int Q, int k, void* stream);
/* General form: k largest of n scores per row; quot = idx / div, rem = idx % div
 * (triplet ranking of the sibling head, relation_heads/baseline.py:1033-1037). */
int pn_topk_f32(const float* scores, int64_t* idx, int64_t* quot, int64_t* rem, int B,
                int n, int div, int k, void* stream);
/* Strided form, k <= 512: score i of row b is scores[b*row_stride + i*elem_stride] (floats).
 * (The two-stage proposal selection of the Deformable-DETR trunk under CrossHeadBBox,
 * `torch.topk(enc_outputs_class[..., 0], 300, dim=1)`: mmdet DeformableDetrTransformer,
 * called at pairnet_bbox_head.py:215-228.) */
int pn_topk_strided_f32(const float* scores, int64_t elem_stride, int64_t row_stride,
                        int64_t* idx, int64_t* quot, int64_t* rem, int B, int n, int div, int k,
                        void* stream);

/* out[b][r][:] = in[b][index[b][r]][:], rows of `len` floats
 * (torch.gather at pairnet_head.py:342-351, 380-403). */
int pn_gather_rows_f32(const float* in, const int64_t* index, float* out, int B,
                       int rows_in, int rows_out, int64_t len, void* stream);

/* ------------------------------------------------------------------------- *
 * Post-processing (pairnet_head.py:788-924)
 * ------------------------------------------------------------------------- */
/* softmax over C logits, drop the last (background) column, max/argmax
 * (:811-815, :823-825).  label = argmax + label_offset (the triplet labels are
 * 1-based, `+ 1` at :812 / :815; the panoptic branch :823-825 is 0-based),
 * score = max prob. */
int pn_cls_argmax_f32(const float* logits, int64_t* label, float* score,
                      int64_t rows, int C, int label_offset, void* stream);
/* r_dists[r][0] = 0, r_dists[r][1:] = softmax(logits[r][:])  (:817-820) */
int pn_rel_dists_f32(const float* logits, float* out, int64_t rows, int C,
                     void* stream);
/* CrossHeadBaseline triplet ranking (pairnet/models/relation_heads/baseline.py).
 * probs [rows][C] = softmax(logits); fg [rows][C-1] = probs[:, 1:]  (:1033-1034) */
int pn_softmax_fg_f32(const float* logits, float* probs, float* fg, int64_t rows,
                      int C, void* stream);
/* idx[r] = first index of max(x[r][:])  (torch.max(-1)[1], :398-399) */
int pn_row_argmax_f32(const float* x, int64_t* idx, int64_t rows, int n,
                      void* stream);
/* labels [2k] = [s_label[tri]+1 | o_label[tri]+1]; r_labels = rem+1;
 * r_scores = probs[tri][rem+1]; r_dists [k][C] = probs[tri]  (:1035-1046) */
int pn_triplet_finish(const int64_t* s_label, const int64_t* o_label,
                      const float* probs, const int64_t* tri, const int64_t* rem,
                      int64_t* labels, int64_t* r_labels, float* r_scores,
                      float* r_dists, int k, int C, void* stream);
/* Panoptic id map (:866-871): masks [n][HW] fp32 logits ->
 * m_id[p] = argmax_i softmax_i(masks[:, p]); remap[i] merges stuff duplicates
 * (:873-878); seg[p] = id*1000 + labels[id]; area[i] = #pixels with id i. */
int pn_panoptic_f32(const float* masks, const int64_t* labels,
                    const int32_t* remap, int64_t* seg, int32_t* area, int n,
                    int64_t HW, void* stream);

/* The whole panoptic branch of _get_bboxes_single (:845-905) with no host round trip:
 * keep = (label != num_classes-1) & (score > 0.5) in query order, duplicate stuff
 * classes (label >= 80) merged into their first occurrence, kept masks resized to
 * (ho, wo), per-pixel argmax -> seg = id*1000 + label, then up to `rounds` rounds of
 * "drop segments with area <= 4 and redo the argmax" (the `while True` of :893-905; a
 * round after convergence returns at once).  The reference loops until nothing is
 * dropped: if the enqueued rounds were not enough, state.active is still 1 and
 * pn_panoptic_continue_f32 runs further rounds on the same buffers; state.all_gone
 * means every segment was filtered (the reference raises IndexError there, :882).
 * No kept query -> seg = 1 everywhere (:850).
 *   masks [Q][hi][wi] mask logits; labels/scores from pn_cls_argmax_f32 over all_cls
 *   state: pn_panoptic_state_bytes() bytes; its first int32 words, readable after the
 *          stream has drained: nkeep, active, rounds (that dropped something), all_gone
 *   up_scratch Q*ho*wo floats; area_scratch 256 int32; seg [ho*wo] int64
 *   Q <= 256, 1 <= rounds <= 256, wo <= 2^24 */
int64_t pn_panoptic_state_bytes(void);
int pn_panoptic_device_f32(const float* masks, const int64_t* labels, const float* scores,
                           int Q, int num_classes, int hi, int wi, int ho, int wo,
                           void* state, float* up_scratch, int32_t* area_scratch,
                           int64_t* seg, int rounds, void* stream);
int pn_panoptic_continue_f32(void* state, const float* up_scratch, int32_t* area_scratch,
                             int64_t* seg, int ho, int wo, int rounds, void* stream);
/* The resize step of pn_panoptic_device_f32 on its own: up[j] = resize(masks[kept[j]]) for the
 * j < nkeep planes `state` lists (nkeep = int32 word 0, kept[256] = int32 words 16..271);
 * planes j >= nkeep of `up` are not written.  form 1 (what pn_panoptic_device_f32 launches):
 * workgroups = (strip of output rows, plane) that loop over their strip, so the cost follows
 * nkeep; form 0: the one-workgroup-per-256-pixels grid of earlier rounds, kept for the
 * bit-for-bit comparison.  The same expression per pixel in both. */
int pn_resize_kept_f32(const float* masks, float* up, const void* state, int Q, int hi, int wi,
                       int ho, int wo, int form, void* stream);

/* One fixed-shape fp32 record per image for the all-gather of predicted triplets that
 * replaces mmdet's pickled collect_results_gpu (tools/test.py:256-267):
 * rec = [labels 2R | rel_dists R*C1 | sub_pos R | obj_pos R], 4R + R*C1 floats. */
int pn_pack_triplets_f32(const int64_t* labels, const float* r_dists, const int64_t* sub_pos,
                         const int64_t* obj_pos, float* rec, int R, int C1, void* stream);

/* Byte copy with a bounded CU footprint (`wgs` workgroups): the device -> pinned-host copy of
 * `triplet2Result`'s fields (psgtr.py:15-51; 51 MB per 800x1333 image), which as a
 * hipMemcpyAsync runs as a chip-wide blit kernel that takes workgroup slots from concurrent
 * GEMMs.  `dst` may be pinned host memory (mapped in the device's address space) or device
 * memory; src / dst 16-byte aligned. */
int pn_copy_stream(const void* src, void* dst, int64_t bytes, int wgs, void* stream);

/* `triplet2Result`'s masks (psgtr.py:38-46: 2R x H0 x W0 numpy bool, 49 of the 51 MB) cross
 * PCIe as bits.  Device: `n` mask bytes (any non-zero = set; `bools` 8-byte aligned) ->
 * (n + 7) / 8 bytes, byte i bit j = element 8 i + j.  Host (no GPU call, runs on `threads`
 * host threads, 1..64): the inverse, one 0 / 1 byte per element = numpy bool. */
int pn_pack_bool_bits(const uint8_t* bools, uint8_t* bits, int64_t n, void* stream);
int pn_unpack_bits_host(const uint8_t* bits, uint8_t* bools, int64_t n, int threads);

/* Ground truth from the decoded panoptic PNG (the evaluator's side: pairnet/datasets/psg.py:
 * 354-372; the training-side loader: pairnet/datasets/pipelines/loading.py:128-147):
 *   rgb   [H][W][3] uint8, RGB                 ids / cats [G] int32: the annotation's segments
 *   masks [G][H][W] uint8 0/1 = (id(pixel) == ids[g]),  id = R + 256 G + 65536 B ([3P]
 *         panopticapi rgb2id); every listed segment, an id absent from the image -> zeros
 *   sem   [H][W] int32 or NULL: cats[g] of the LAST listed segment owning the pixel, else 255
 * G <= 256; rgb and masks 4-byte aligned.  G == 0 with sem: sem is filled with 255. */
int pn_pan_masks_u8(const uint8_t* rgb, const int* ids, const int* cats, uint8_t* masks, int* sem,
                    int G, int H, int W, void* stream);

/* Test-time image front end (configs/mask2former/pairnet.py:310-331, mean / std :229-231):
 * mmdet Resize(keep_ratio) [= mmcv.imresize = OpenCV INTER_LINEAR on uint8, fixed point] ->
 * Normalize(to_rgb) -> Pad -> ImageToTensor of one decoded image, fused.
 *   img  [H][W][3] uint8, BGR (cv2 order)        out [3][Hp][Wp] fp32, zero beyond (Hn, Wn)
 *   (Hn, Wn) = mmcv.rescale_size of (H, W); mean3 / stdinv3: HOST pointers, output order */
int pn_preprocess_u8_f32(const uint8_t* img, int H, int W, float* out, int Hn, int Wn, int Hp,
                         int Wp, const float* mean3, const float* stdinv3, int to_rgb,
                         void* stream);

/* Train-time input pipeline (configs/mask2former/pairnet.py:234-306: RandomFlip -> AutoAugment
 * [policy 1: Resize | policy 2: Resize -> RelRandomCrop -> Resize] -> Normalize -> Pad ->
 * RelsFormatBundle -> collate at samples_per_gpu=2).  The draws and the boxes are host work; each
 * entry below refuses (-1) null pointers, non-positive sizes, a window outside the resized image,
 * misaligned bases and a batch tensor smaller than the image.
 *
 * The LAST Resize -> Normalize -> Pad -> collate of one image (pairnet.py:247-266 / :280-298,
 * :302-303; mmcv.imresize = OpenCV INTER_LINEAR on uint8, the arithmetic of
 * pn_preprocess_u8_f32) with RandomFlip (:243; mmcv.imflip, horizontal) folded in as a column
 * permutation of the source:
 *   img [H][W][3] uint8 BGR: the decoded image (policy 1) or the window below (policy 2, flip 0)
 *   out: base of the float32 batch tensor [k][3][Hmax][Wmax]; image `slot` is written at
 *        out + slot * batch_stride (elements, >= 3 Hmax Wmax), zero beyond (Hn, Wn) */
int pn_augment_image_u8_f32(const uint8_t* img, int H, int W, int flip, float* out,
                            int64_t batch_stride, int slot, int Hn, int Wn, int Hmax, int Wmax,
                            const float* mean3, const float* stdinv3, int to_rgb, void* stream);

/* Policy 2's first Resize (pairnet.py:268-273) of the optionally flipped image, evaluated on
 * the crop window of RelRandomCrop only (pairnet/datasets/pipelines/rel_randomcrop.py:27-39):
 *   out [ch][cw][3] uint8, out(y, x) = pixel (y + oy, x + ox) of the [H1][W1] resize;
 *   0 <= oy, oy + ch <= H1, 0 <= ox, ox + cw <= W1. */
int pn_augment_resize_crop_u8(const uint8_t* img, int H, int W, int flip, int H1, int W1, int oy,
                              int ox, uint8_t* out, int ch, int cw, void* stream);

/* Every mask stage of the training pipeline in one gather: the loader
 * (pairnet/datasets/pipelines/loading.py:128-147: rgb2id(PNG) == id), RandomFlip, the
 * BitmapMasks.rescale of both Resizes (OpenCV INTER_NEAREST: source index
 * min(floor(dst * (1.0 / ((double)dst_size / src_size))), src_size - 1), doubles),
 * RelRandomCrop's mask crop (rel_randomcrop.py:76-81), Pad, collate, and `PSGTr.forward_train`'s
 * pad to the batch tensor + nearest resize to half size (frameworks/psgtr.py:126-141, the
 * arithmetic of pn_gt_mask_prepare_u8):
 *   png [H0][W0][3] uint8 RGB            ids [Gk] int32: the segments the crop kept, Gk <= 256
 *   (H1, W1): first Resize; window (oy, ox, ch, cw) inside it; (H2, W2): second Resize of the
 *   window.  Policy 1: window = (0, 0, H1, W1) and (H2, W2) = (H1, W1).
 *   out [Gk][Hb / 2][Wb / 2] uint8 0/1, (Hb, Wb) >= (H2, W2) the batch tensor's size.
 * png, ids and out 4-byte aligned. */
int pn_augment_masks_u8(const uint8_t* png, int H0, int W0, const int* ids, int Gk, int flip,
                        int H1, int W1, int oy, int ox, int ch, int cw, int H2, int W2, int Hb,
                        int Wb, uint8_t* out, void* stream);

/* Evaluator feed (pairnet/evaluation/sgg_metrics.py:1276-1380, mask_iou :1374-1380):
 * masks as bit rows (bit i of word w = pixel 64w+i) and the exact integer counts
 * behind IoU: inter[i][j] = |pred_i & gt_j|, area_pred[i], area_gt[j]. */
int pn_pack_mask_bits(const uint8_t* masks, uint64_t* words, int64_t rows, int64_t HW,
                      void* stream);
int pn_mask_iou_counts(const uint64_t* pred_words, int P, const uint64_t* gt_words, int G,
                       int64_t nwords, int32_t* inter, int32_t* area_pred, int32_t* area_gt,
                       void* stream);

/* Evaluator feed, part 2: SGRecall's triplet matching (sgg_metrics.py:173-252, :1311-1371).
 *   pn_pred_triplets   triplets[r] = (labels[r], 1 + argmax(rel_dists[r][1:]), labels[R+r]),
 *                      scores[r] = that maximum (:207-209, :1292-1294)
 *   pn_mask_or_rows    out[r] = words[a[r]] | words[b[r]]: the union masks of phrase
 *                      detection (:1343-1350)
 *   pn_triplet_match   match[p][g] = classes equal && IoU(subject) >= thr && IoU(object) >= thr
 *                      from the counts of pn_mask_iou_counts (inter [*][ld_inter], areas),
 *                      rows chosen through the *_row tables; phrdet: one IoU (the union
 *                      counts passed as the subject arguments). */
int pn_pred_triplets(const int64_t* labels, const float* r_dists, int32_t* triplets,
                     float* scores, int R, int C1, void* stream);
int pn_mask_or_rows(const uint64_t* words, const int32_t* a, const int32_t* b, uint64_t* out,
                    int rows, int64_t nwords, void* stream);
int pn_triplet_match(const int32_t* pred_triplets, const int32_t* gt_triplets, int P, int G,
                     const int32_t* inter, const int32_t* area_pred, const int32_t* area_gt,
                     int ld_inter, const int32_t* pred_sub_row, const int32_t* pred_obj_row,
                     const int32_t* gt_sub_row, const int32_t* gt_obj_row, double iou_thr,
                     int phrdet, int ignore_rel, uint8_t* match, void* stream);
/* The same triplet match on boxes, for `detection_method="bbox"` (the box-trunk sibling head):
 * `_compute_pred_matches_bbox` (sgg_metrics.py:1212-1273) with mmdet's
 * `bbox_overlaps(mode="iou", eps=1e-6)` in float32; boxes (x1, y1, x2, y2) in rows of ld_*
 * floats (so `refine_bboxes` [2R][5] can be passed as it is); phrdet: union boxes. */
int pn_triplet_match_boxes(const int32_t* pred_triplets, const int32_t* gt_triplets, int P, int G,
                           const float* pred_boxes, int ld_pred, const float* gt_boxes, int ld_gt,
                           const int32_t* pred_sub_row, const int32_t* pred_obj_row,
                           const int32_t* gt_sub_row, const int32_t* gt_obj_row, float iou_thr,
                           int phrdet, int ignore_rel, uint8_t* match, void* stream);

/* Evaluator feed, part 3 (csrc/evaluate.hip): one image's share of the dataset-level metrics as
 * integers that stay on the device until the end of the run.
 * The recall record -- `reduce(np.union1d, pred_to_gt[:k])` of sgg_metrics.py:95-99 fed through
 * `SGMeanRecall._collect_single` (:741-766) -- from the two uint8 match matrices [R][G] that
 * the triplet-match entries above write (graph-constrained sgdet, phrase detection):
 *   gt_predicates [G] int32 in [1, num_rel)      ks [nk] int32, nk <= 8
 *   num_rel = predicates + background, <= 256
 *   hits [2][nk][num_rel] int32: hits[mode][j][n] = distinct ground-truth relations with
 *        predicate n matched by one of the first min(ks[j], R) predictions; slot n = 0 counts
 *        the relations of every predicate (mode 0 sgdet, 1 phrdet)
 *   counts [num_rel] int32: ground-truth relations with predicate n; counts[0] = G.
 * Integer histograms only: the result does not depend on any order of execution. */
int pn_eval_record(const uint8_t* match_sgdet, const uint8_t* match_phrdet, int R, int G,
                   const int32_t* gt_predicates, const int32_t* ks, int nk, int num_rel,
                   int32_t* hits, int32_t* counts, void* stream);
/* The subject / object IoU statistic, `_compute_iou_panseg` (sgg_metrics.py:1087-1131), from
 * the integer counts of the mask-IoU entry above: inter [P][n_obj], area_pred [P], area_gt [n_obj];
 * pred_labels [P] int64, gt_labels [n_obj] int32, gt_sub_row / gt_obj_row [G] the object rows
 * of the G ground-truth relations.  Per side s (0 subject, 1 object) and relation g:
 *   valid [2][G] uint8: the class of that object occurs among pred_labels
 *   best  [2][G] float64: the reference's walk over the predictions of that class in index
 *        order, best = (best > v) ? best : v from 0, v = (double)inter / (double)(area_pred +
 *        area_gt - inter), NaN where the union is empty -- Python's max(v, best), NaN included. */
int pn_eval_iou_best(const int32_t* inter, const int32_t* area_pred, const int32_t* area_gt,
                     int P, int n_obj, const int64_t* pred_labels, const int32_t* gt_labels,
                     const int32_t* gt_sub_row, const int32_t* gt_obj_row, int G, uint8_t* valid,
                     double* best, void* stream);
/* The box form of that statistic (csrc/nogc.hip), `SGObjectIOU.calculate_iou` -> `_compute_iou_bbox`
 * (sgg_metrics.py:1025-1028, :1133-1178), for `detection_method="bbox"`: per side s (0: the subject
 * predictions [0, R), 1: the object predictions [R, 2R)) and ground-truth OBJECT o (objects, not
 * relations).  The reference hard-codes the split at 100; this splits at R, identical at the only
 * R any config uses.  pred_boxes [2R] rows of ld_pred floats, pred_labels [2R] int64, gt_boxes
 * [n_obj] rows of ld_gt floats (x1, y1, x2, y2), gt_labels [n_obj] int32.
 *   valid [2][n_obj] uint8: some prediction of that side has the object's class
 *   best  [2][n_obj] float64: the maximum over those of mmdet's `bbox_overlaps(mode="iou",
 *        eps=1e-6)` in float32 (`bbox_overlaps` restated from memory, unpinned; the device
 *        function pn_triplet_match_boxes uses), as the exact float64 of that float32; 0 where
 *        valid is 0.  Python's `max(row)`: the first value unless a later one is greater.
 * Entry added at ABI 34. */
int pn_eval_iou_best_boxes(const float* pred_boxes, int ld_pred, const int64_t* pred_labels, int R,
                           const float* gt_boxes, int ld_gt, const int32_t* gt_labels, int n_obj,
                           uint8_t* valid, double* best, void* stream);

/* Evaluator feed, part 4 (csrc/nogc.hip): the no-graph-constraint ranking of
 * `SGRecall.calculate_recall` (sgg_metrics.py:254-343), one launch per image.
 *   det [2R] rows of ld >= 5 floats, the object score in column 4 (`refine_bboxes` as it is)
 *   labels [2R] int64      rel_dists [R][C1] float32      sub_row / obj_row [R] int32 in [0, 2R)
 *   per_row = the reference's `nogc_num`, 1 <= per_row <= C1 - 1      1 <= K <= 100 (:306-308)
 * Candidate (r, c), c in 1..C1-1, scores (det[sub_row[r]][4] * det[obj_row[r]][4]) *
 * rel_dists[r][c]: two separately rounded fp32 products in that order (:256-257).  It survives
 * the per-row cut iff fewer than per_row candidates of its row beat it (:258-264).  The survivors
 * are ranked in descending order and the first count = min(K, R * per_row) are written:
 *   triplets [K][3] int32 = (labels[sub_row[r]], c, labels[obj_row[r]])
 *   sub_rows / obj_rows [K] int32      scores [K] float32 (the product)      count [1] int32
 * rows past count are filled with -1 (scores: 0).  Ties (numpy leaves them unspecified, so this
 * is a documented choice, not parity): inside a row and in the ranking the candidate with the
 * smaller (r, c) wins, -0 == +0 -- the rule of pn_topk_pairs.  Scores are finite.
 * R * (C1 - 1) <= 65536.  No float atomics; the result is independent of execution order.
 * Entry added at ABI 34. */
int pn_nogc_triplets_f32(const float* det, int ld, const int64_t* labels, const float* rel_dists,
                         const int32_t* sub_row, const int32_t* obj_row, int R, int C1,
                         int per_row, int K, int32_t* triplets, int32_t* sub_rows,
                         int32_t* obj_rows, float* scores, int32_t* count, void* stream);

/* Panoptic quality (csrc/panoptic_quality.hip): one image's share of PQ / SQ / RQ, the metric of
 * the reference's `--eval PQ` (pairnet/datasets/psg.py:309-335 -> [3P] mmdet's panoptic
 * evaluation), from the panoptic map `pairnet_head.py:882` writes (value = segment *
 * INSTANCE_OFFSET + class; csrc/postproc.hip).  The metric is restated from memory, unpinned;
 * INTEGRATION.md 3a-2 states it in full and is the specification.  Entries added at ABI 34.
 * The confusion table, one pass, every pixel read once:
 *   pred [H][W] int64 (16-byte aligned): s = value / instance_offset < 256, c = value %
 *        instance_offset; c == num_classes is void
 *   gt_rgb [H][W][3] uint8 (4-byte aligned): the panoptic PNG, id = R + 256 G + 65536 B
 *   gt_ids [G] int32, strictly ascending, in [1, 2^24); G <= 255 (G == 0: any readable word)
 *   N [G + 1][257] int32: N[g][p] = pixels of ground-truth row g (0 = void: id 0 or not in
 *        gt_ids; g = 1 + index into gt_ids) under predicted column p (p = s; 256 = void)
 *   col_cat [256] int32: the category of column s, -1 for a segment without pixels
 *   status [1] int32: 0, | 1 a value < 0 or with c > num_classes, | 2 s >= 256, | 4 two
 *        categories under one s; flagged pixels are counted nowhere.
 * All three outputs are written whole (no zeroing by the caller).  Integer atomics only: the
 * result does not depend on any order of execution.  The table is kept in LDS per workgroup
 * for G <= 61 and summed into N at the end; above, the adds go to N directly.
 * flags: PN_PQ_PLAIN = one atomic add per pixel (the form the aggregated one is measured
 * against), else 0.  H * W < 2^31, 1 <= num_classes <= 999 < instance_offset. */
#define PN_PQ_PLAIN 1
int pn_pq_confusion(const int64_t* pred, const uint8_t* gt_rgb, int H, int W,
                    const int32_t* gt_ids, int G, int num_classes, int instance_offset,
                    int flags, int32_t* N, int32_t* col_cat, int32_t* status, void* stream);
/* The image's record from N and col_cat above, gt_cat / gt_crowd [G] int32 (category in
 * [0, num_classes), iscrowd) in gt_ids' order; one workgroup:
 *   area_gt [G + 1], area_pred [257] int32: row and column sums of N
 *   match [G + 1] int32: the column matched to row g, or -1 (row 0: -1).  (g, p) match when g is
 *        not void and not crowd, the categories are equal, N[g][p] > 0 and 2 N[g][p] > union,
 *        union = area_pred[p] + area_gt[g] - N[g][p] - N[0][p] (iou > 0.5, decided in integers)
 *   rec [num_classes][3] int32 = (tp, fp, fn): fn = unmatched non-crowd rows; fp = unmatched
 *        columns unless 2 (N[0][p] + sum over crowd rows of its category N[g'][p]) > area_pred[p]
 *   iou [num_classes] float64: the sum of (double)N / (double)union over the matches, added in
 *        ascending ground-truth id
 *   status [1]: |= 8 for a gt_cat outside [0, num_classes) (not re-zeroed here). */
int pn_pq_record(const int32_t* N, const int32_t* col_cat, const int32_t* gt_cat,
                 const int32_t* gt_crowd, int G, int num_classes, int32_t* area_gt,
                 int32_t* area_pred, int32_t* match, int32_t* rec, double* iou, int32_t* status,
                 void* stream);

/* ------------------------------------------------------------------------- *
 * Box trunk of the sibling head CrossHeadBBox (pairnet_bbox_head.py:193-359): the
 * input-dependent glue of mmdet's two-stage, box-refining DeformableDetrTransformer
 * (built at :66, called at :215-228) between this library's GEMM / deformable-attention
 * entries.  All row-parallel and HBM-bound.
 * ------------------------------------------------------------------------- */
/* out[b][r][:] = valid[b][r] ? x[b][r][:] : 0 on rows of C floats at stride ld (C % 4 == 0);
 * valid: bytes, advancing by valid_bstride per image (0: one table for the batch); x == out
 * allowed.  (gen_encoder_output_proposals: tokens whose proposal box leaves (0.01, 0.99) and
 * padded tokens are zeroed before enc_output; mmcv MultiScaleDeformableAttention zeroes the
 * value rows of padded tokens, `value.masked_fill(key_padding_mask[..., None], 0)`.) */
int pn_zero_rows_f32(const float* x, const uint8_t* valid, float* out, int B, int64_t rows,
                     int C, int64_t ld, int64_t valid_bstride, void* stream);
/* y = sigmoid(x) elementwise (enc_bbox_preds, pairnet_bbox_head.py:345-347; sigmoid(inf) = 1) */
int pn_sigmoid_f32(const float* x, float* y, int64_t n, void* stream);
/* Two-stage queries: ref[r][4] = sigmoid(unact[r][4]) and emb[r][512] =
 * get_proposal_pos_embed(unact) (128 sine features per coordinate, temperature 1e4). */
int pn_box_pos_embed_f32(const float* unact, float* ref, float* emb, int64_t rows, void* stream);
/* Decoder cross-attention operands (mmcv MultiScaleDeformableAttention.forward with 4-d
 * reference boxes): offaw row = [offsets 8*L*4*2 | logits 8*L*4] (stride ld floats);
 * aw [rows][8][L][4] = softmax over each head's L*4 logits; loc [rows][8][L][4][2] =
 * ref.xy + offset / 4 * ref.wh * 0.5 -- the operands of pn_msda_loc_f32. */
int pn_box_sampling_f32(const float* offaw, int64_t ld, const float* ref,
                        const float* valid_ratios, int rows_per_image, float* loc, float* aw,
                        int64_t rows, int L, void* stream);
/* (valid_ratios, nullable: [B][L][2] = (valid width / W_l, valid height / H_l) of a padded
 * batch -- the decoder's `reference_points * cat([valid_ratios, valid_ratios])`; image of row
 * r = r / rows_per_image.)
 * The encoder's self-attention operands on a PADDED batch: for every token of every image the
 * sampling locations / softmax weights with mmdet's get_reference_points,
 * ref = (x + .5) / (vr[lq] * W_lq) * vr[ls], location = ref + offset / (W_ls, H_ls); offaw rows
 * as above, tokens level by level; outputs are pn_msda_loc_f32's operands.  (Unpadded batches
 * use the fused pn_msda_f32, where every valid ratio is 1.) */
int pn_token_sampling_f32(const float* offaw, int64_t ld, const float* valid_ratios, float* loc,
                          float* aw, int B, int L, const int32_t* level_h, const int32_t* level_w,
                          void* stream);
/* Iterative box refinement: ref_out = sigmoid(delta + inverse_sigmoid(ref_in, eps=1e-5)),
 * [rows][4] (DeformableDetrTransformerDecoder.forward; also the last layer's
 * `outputs_coord`, pairnet_bbox_head.py:236-246). */
int pn_box_refine_f32(const float* delta, const float* ref_in, float* ref_out, int64_t rows,
                      void* stream);
/* Query ranking (pairnet_bbox_head.py:252-254): score[b][q] = max over classes of
 * softmax(logits[b], dim = the QUERY axis)[q]; logits [B][Nq][C], C <= 256. */
int pn_query_score_f32(const float* logits, float* score, int B, int Nq, int C, void* stream);
/* CrossHeadBBox._get_bboxes_single (:1056-1086): rows [subjects R | objects R]:
 * labels = argmax softmax + 1, det[row] = (x1, y1, x2, y2, max softmax), boxes cxcywh ->
 * xyxy * (img_w, img_h), clamped to the image, divided by scale_factor[4] (a HOST pointer)
 * when rescale. */
int pn_box_triplets_f32(const float* s_cls, const float* o_cls, const float* s_box,
                        const float* o_box, float* det, int64_t* labels, int R, int C,
                        float img_h, float img_w, const float* scale_factor, int rescale,
                        void* stream);

/* ------------------------------------------------------------------------- *
 * Loss forward of CrossHead2 on device outputs (first slice: the
 * values of `CrossHead2.loss`, pairnet_head.py:419-718; no backward).  The two
 * Hungarian assignments themselves run on the host, as in the reference
 * (`linear_sum_assignment(cost.cpu())`, matcher.py:262-264, and [3P] mmdet
 * MaskHungarianAssigner): these entries produce their cost matrices and the loss
 * scalars.
 * ------------------------------------------------------------------------- */
/* `PSGTr.forward_train`'s ground-truth mask preparation (frameworks/psgtr.py:126-141):
 * masks [G][h][w] uint8 0/1 -> zero-padded on the right / bottom to the batch tensor's
 * [H][W] (F.pad) -> nearest-neighbour resize to [Ho][Wo] (F.interpolate(mode="nearest"):
 * source index min(floor(dst * (float)in / out), in - 1); the reference passes
 * (Ho, Wo) = (H // 2, W // 2)).  out [G][Ho][Wo] uint8.  G, Ho <= 65535. */
int pn_gt_mask_prepare_u8(const uint8_t* masks, uint8_t* out, int G, int h, int w, int H, int W,
                          int Ho, int Wo, void* stream);

/* [3P] mmcv `point_sample` (pairnet_head.py:631-638) = grid_sample(maps, 2 p - 1, bilinear,
 * zero padding, align_corners=False) with ONE point set shared by all maps:
 * maps [P][h][w] float32, or uint8 0/1 when maps_are_u8 (ground-truth masks); pts [Np][2]
 * (x, y) in [0, 1]; out [P][Np]. */
int pn_point_sample_f32(const void* maps, int maps_are_u8, const float* pts, float* out, int P,
                        int h, int w, int Np, void* stream);
/* [3P] mmdet MaskHungarianAssigner's cost matrix (cfg configs/mask2former/pairnet.py:200-206;
 * called at pairnet_head.py:641-643): cost [Q][G] =
 *   -softmax(cls[q])[gt_labels[g]] w_cls + mean_p BCEwithLogits(pred_pts[q][p], gt_pts[g][p]) w_mask
 *   + (1 - (2 sum s t + eps) / (sum s + sum t + eps)) w_dice,  s = sigmoid(pred_pts[q]). */
int pn_mask_match_cost_f32(const float* cls /* [Q][ncls] */, int ncls,
                           const int64_t* gt_labels /* [G] */, const float* pred_pts /* [Q][Np] */,
                           const float* gt_pts /* [G][Np] */, float* cost, int Q, int G, int Np,
                           float w_cls, float w_mask, float w_dice, float dice_eps, void* stream);
/* `IdMatcher.assign` cost (approaches/matcher.py:250-258; called at pairnet_head.py:662-671):
 * cost [R][G] = -softmax(sub[r])[gt_sub[g]] w_sub - softmax(obj[r])[gt_obj[g]] w_obj
 *               - softmax(rel[r])[gt_rel[g]] w_rel. */
int pn_id_match_cost_f32(const float* sub, const float* obj /* [R][ncls] */, const float* rel
                         /* [R][nrel] */, int ncls, int nrel, const int64_t* gt_sub,
                         const int64_t* gt_obj, const int64_t* gt_rel, float* cost, int R, int G,
                         float w_sub, float w_obj, float w_rel, void* stream);
/* [3P] mmdet CrossEntropyLoss, softmax form, reduction "mean" (`subobj_cls_loss`,
 * pairnet_head.py:518-527): out[0] = loss_weight * mean over rows with target >= 0 of
 * class_weight[y] (logsumexp(x) - x[y]); rows with target < 0 are the unmatched queries the
 * reference masks out (`r_label_weights_mask`).  rows <= 4096. */
int pn_ce_mean_f32(const float* logits, int64_t ld, const int64_t* target,
                   const float* class_weight /* [C] or NULL */, float* out, int rows, int C,
                   float loss_weight, void* stream);
/* [3P] mmdet SeesawLoss, `loss_cls_classes` (`rel_cls_loss`, pairnet_head.py:529-536) over the
 * rows with target >= 0; cum_samples [C] = the loss's persistent label counts INCLUDING this
 * batch (the caller accumulates them, as seesaw_loss.py does before weighing).  C <= 64. */
int pn_seesaw_mean_f32(const float* logits, int64_t ld, const int64_t* target,
                       const float* cum_samples, float* out, int rows, int C, float p, float q,
                       float eps, float loss_weight, void* stream);
/* `BCEWithLogitsLoss` (losses/seg_losses.py:153-166) with the reference's
 * pos_weight = numel / #(target > 0) (pairnet_head.py:541-552): out[0] = loss_weight * mean,
 * out[1] = pos_weight. */
int pn_bce_posw_mean_f32(const float* logits, const float* target, float* out /* [2] */, int64_t n,
                         float loss_weight, void* stream);

/* SURVEY 8 f-4, first backward slice: the gradients of the three reductions above with respect to
 * their logits (`loss_sub_cls` / `loss_obj_cls`, `loss_r_cls`, `loss_match`; pairnet_head.py:518-552):
 *   CE      g[r][c] = loss_weight / n * class_weight[y] * (softmax(x_r)[c] - [c == y])
 *   Seesaw  g[r][j] = loss_weight / n * (softmax(x'_r)[j] - [j == y]), the seesaw weights constants of
 *           the backward pass ([3P] seesaw_ce_loss uses softmax(cls_score.detach()))
 *   BCE     g[i]    = loss_weight / n * ((1 - t) - (1 + (pos_weight - 1) t) sigmoid(-x))
 * rows with target < 0 get zeros; n = rows with target >= 0 (CE, Seesaw) / all elements (BCE).
 * Checked against autograd through the reference-pinned loss oracle (tests/test_losses_gpu.py). */
int pn_ce_mean_grad_f32(const float* logits, int64_t ld, const int64_t* target,
                        const float* class_weight /* [C] or NULL */, float* grad, int64_t ldg,
                        int rows, int C, float loss_weight, void* stream);
int pn_seesaw_mean_grad_f32(const float* logits, int64_t ld, const int64_t* target,
                            const float* cum_samples, float* grad, int64_t ldg, int rows, int C,
                            float p, float q, float eps, float loss_weight, void* stream);
int pn_bce_posw_mean_grad_f32(const float* logits, const float* target, float* grad, int64_t n,
                              float loss_weight, void* stream);

/* ------------------------------------------------------------------------- *
 * Loss targets on the device (csrc/assign.hip, ABI 33): the two Hungarian assignments and the index
 * bookkeeping of `_get_target_single`, so that a training step does not wait for the host.
 * ------------------------------------------------------------------------- */
/* Batched rectangular linear sum assignment: what `linear_sum_assignment(cost.cpu())` returns at
 * approaches/matcher.py:262-264 (IdMatcher) and in [3P] mmdet mask_hungarian_assigner.py
 * (MaskHungarianAssigner.assign; both called from pairnet_head.py:645-718), for P problems in one
 * launch, one wavefront each.  scipy's algorithm (shortest augmenting paths on float64 duals over the
 * fp32 costs) step for step: row_ind / col_ind EQUAL scipy's, ties included.
 *   cost [cost_len] fp32; table [P][4] int64 on the device = {offset of the row-major rows x cols
 *   matrix in cost, rows, cols, offset of the problem's min(rows, cols) output entries};
 *   row_ind (ascending) / col_ind [out_len] int32; status [P] int32: 0 solved, 1 a NaN or -inf entry,
 *   2 infeasible (scipy raises on both; the outputs are filled with -1), 3 a descriptor outside
 *   cost_len / out_len or a side above 1024 (nothing else is written).
 * max_cells: the largest rows * cols of the table (a hint: matrices of up to 24576 entries are
 * staged in LDS).  Static loop bounds, no atomics: ends on any input. */
int pn_lsa_f32(const float* cost, int64_t cost_len, const int64_t* table, int P, int64_t max_cells,
               int32_t* row_ind, int32_t* col_ind, int64_t out_len, int32_t* status, void* stream);
/* The bookkeeping behind the assignments (pairnet_head.py:645-718 and the SeesawLoss label counts of
 * [3P] seesaw_loss.py's forward) for a batch of B images.  lsa_table / row_ind / col_ind / lsa_status:
 * pn_lsa_f32's operands with problem 2b = image b's Q x G mask assignment and 2b+1 its R x T triplet
 * assignment; tgt_table [B][4] int64 = {offset of gt_labels [G], offset of gt_rels [T][3], G, T},
 * offsets into gt [gt_len] int64.  Writes
 *   importance [B][Q][Q]: 0, then 1 at (query_of_gt[s], query_of_gt[o]) of every ground-truth
 *     relation (query_of_gt: the matched query, 1 for an unmatched object as `torch.ones_like`, :648);
 *   labels [3][B*R] int64: r_labels (gt relation - 1) | sub_ids | obj_ids, -1 for unmatched queries;
 *   cum_samples [C + 1] += the histogram of the r_labels >= 0 (before pn_seesaw_mean_f32 reads it);
 *   batch_status [1]: the OR of lsa_status, | 4 for a ground-truth index out of range.  Non-zero:
 *     the fills only, counts untouched.
 * G <= 1024, 2 <= Q, R <= 1024, C <= 254. */
int pn_loss_targets(const int64_t* lsa_table, const int32_t* row_ind, const int32_t* col_ind,
                    const int32_t* lsa_status, const int64_t* tgt_table, const int64_t* gt,
                    int64_t gt_len, int B, int Q, int R, int C, float* importance, int64_t* labels,
                    float* cum_samples, int32_t* batch_status, void* stream);

/* ------------------------------------------------------------------------- *
 * SURVEY 8 f-4, second backward slice (csrc/grad.hip): what the backward of Pair-Net's own tail
 * needs beside the forward kernels above -- the Relation Fusion decoder
 * (pairnet_head.py:353-378; layers: facebook_detr.py:378-432), the Pair Proposal Network
 * (pairnet_head.py:322-333) and the Matrix Learner (frameworks/cnn_factory.py:6-53).  In the
 * reference this is torch.autograd behind `losses.backward()` (mmcv's OptimizerHook, configs/
 * _base_/schedules/schedule_1x.py); pair-net_amd/grad.py composes these entry points with
 * pn_gemm_f32 (dX = dY W and dW = dY^T X on transposed operands) and pn_conv2d_nhwc_ex_f32.
 * Every reduction runs in a fixed order (no atomics).  Checked against autograd through the
 * reference-pinned oracle (tests/test_grad_gpu.py).
 * ------------------------------------------------------------------------- */
/* out[c][r] = in[r][c] for in [rows][ldi >= cols]; out [cols][ldo], columns rows .. out_cols-1 of
 * every output row are zero-filled (out_cols >= rows: pads a contraction length to 4). */
int pn_transpose_f32(const float* in, int64_t ldi, float* out, int64_t ldo, int rows, int cols,
                     int out_cols, void* stream);
/* out[c] (+)= sum_r x[r][c]  (bias / LayerNorm-weight gradients, second stage of the tap correlations);
 * scratch (nullable): up to 64 * cols floats, lets a tall matrix be summed in row chunks by many
 * workgroups + one combining launch (fixed order either way). */
int pn_colsum_f32(const float* x, int64_t ld, float* out, int rows, int cols, int accumulate,
                  float* scratch, int64_t scratch_floats, void* stream);
/* dx[i] = y[i] > 0 ? dy[i] : 0  (y: the ReLU's output; dx may alias dy) */
int pn_relu_bwd_f32(const float* dy, const float* y, float* dx, int64_t n, void* stream);
/* out[i] = a[i] + b[i % bn]  (x + row-periodic table; bn == n: a plain sum, out may alias a) */
int pn_add_periodic_f32(const float* a, const float* b, float* out, int64_t n, int64_t bn,
                        void* stream);
/* out[i] (+)= sum_b x[b][i], i < n  (gradient of a table broadcast over the batch) */
int pn_batch_sum_f32(const float* x, float* out, int B, int64_t n, int accumulate, void* stream);
/* nn.LayerNorm(256) backward from the saved INPUT x [rows][256]: dx, and gxhat = dy * xhat whose
 * column sum is d weight (d bias = column sum of dy). */
int pn_layernorm256_bwd_f32(const float* dy, const float* x, const float* gamma, float* dx,
                            float* gxhat, int rows, float eps, void* stream);
/* nn.MultiheadAttention core backward, 8 heads x 32 channels, from the saved projections
 * q [B*Nq][ldq], k / v [B*Nk][ldk / ldv] and the gradient of the concatenated head outputs dout
 * [B*Nq][ldo]: dq, dk, dv (same row layouts).  bits / rowall: the forward's boolean mask as
 * pn_mask_pack wrote it (both NULL: no mask).  scratch: 2 * B * 8 * Nq * Nk floats. */
int pn_mha_bwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                   int64_t ldv, const float* dout, int64_t ldo, float* dq, int64_t lddq, float* dk,
                   int64_t lddk, float* dv, int64_t lddv, const uint32_t* bits,
                   const int32_t* rowall, float* scratch, int B, int Nq, int Nk, float scale,
                   void* stream);
/* The same backward WITHOUT a mask, the keys split into chunks of pn_mha_keysplit_chunk() across
 * workgroups (csrc/attn_grad.hip): the relation decoder's cross-attentions of the sibling head
 * over a memory level (baseline.py:372-386; Nq = 100, Nk up to 16 700, no attention mask).  The
 * probabilities and dS stay on chip; the softmax's row maximum and sum and the row term
 * sum_j P dP are recomputed per chunk and combined in ascending chunk order.  The logits' dots,
 * dP = dout . v, the row term and the difference dP - row term are formed in float64 (the row term
 * is NOT taken as dout . out from a saved output): under a peaked softmax an fp32 difference
 * leaves whole dk rows with a relative error of 1e-5.  dq / dk / dv are accumulated in fp32; no
 * atomics, two launches give equal bits, every element of dq / dk / dv is written.  All seven row
 * strides are free (>= 256, multiples of 4; bases 16-byte aligned); any Nq, Nk >= 1, B <= 65535.
 * scratch: pn_mha_bwd_keysplit_scratch_floats(B, Nq, Nk) = B * 8 * Nq * (6 + 32 * chunks) floats
 * (the row statistics and the per-chunk dq partials); a smaller `scratch_floats` is refused before
 * any launch. */
int pn_mha_keysplit_chunk(void);
int64_t pn_mha_bwd_keysplit_scratch_floats(int B, int Nq, int Nk);
int pn_mha_bwd_keysplit_f32(const float* q, int64_t ldq, const float* k, int64_t ldk,
                            const float* v, int64_t ldv, const float* dout, int64_t ldo,
                            float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv,
                            int64_t lddv, float* scratch, int64_t scratch_floats, int B, int Nq,
                            int Nk, float scale, void* stream);
/* pn_mha_bwd_keysplit_f32 UNDER the forward's packed boolean mask: the nine masked decoder layers'
 * cross-attentions (pairnet_head.py:302-312 / baseline.py:254-296).  bits [B * Nq][(Nk + 31) / 32]
 * and rowall [B * Nq] exactly as pn_mask_pack writes them: a set bit = the key is not attendable,
 * shared by the 8 heads; a row with rowall == 1 ignores its bits (as pn_mha_bwd_f32 and the
 * forward do).  Both NULL: no mask, the launches and bits of pn_mha_bwd_keysplit_f32; one given
 * without the other is PN_BAD_ARG before any launch.  A masked (query, key) pair has P = 0 and
 * dS = 0 exactly; a key masked in every row gets zero dk / dv rows, which are still written; a
 * chunk whose keys are all masked for a row has the weight 0 in the combination (no exponential of
 * (-inf) - (-inf) is formed).  Same float64 places, same fixed summation orders (no atomics, two
 * launches give equal bits), same operand rules and the same scratch size as the unmasked entry. */
int pn_mha_bwd_keysplit_masked_f32(const float* q, int64_t ldq, const float* k, int64_t ldk,
                                   const float* v, int64_t ldv, const float* dout, int64_t ldo,
                                   float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv,
                                   int64_t lddv, float* scratch, int64_t scratch_floats, int B,
                                   int Nq, int Nk, float scale, const uint32_t* bits,
                                   const int32_t* rowall, void* stream);
/* Backward of pn_gather_rows_f32: out[b][row][0:length] (+)= sum_{s: index[b][s] == row}
 * src[b][s][0:length]; src [B*slots][ld_src], out [B*rows_out][ld_out]. */
int pn_scatter_rows_add_f32(const float* src, int64_t ld_src, const int64_t* index, float* out,
                            int64_t ld_out, int B, int rows_out, int slots, int length,
                            int accumulate, void* stream);
/* Cosine block backward (pairnet_head.py:325-333): x [B][Q][256] this side's rows BEFORE
 * F.normalize, other_hat [B][Q][256] the other side's normalised rows, draw [B][Q][Q] the gradient
 * of importance_raw (transposed != 0: this side indexes draw's columns, i.e. the objects). */
int pn_cosine_bwd_f32(const float* draw, const float* x, const float* other_hat, float* dx, int B,
                      int Q, int transposed, float eps, void* stream);
/* Matrix Learner last layer (64 -> 1): gradient w.r.t. its input c [B][S][S][64] (a ReLU output:
 * masked where c == 0) from g [B][S][S]; w3 [49][64] as pn_mlearner_last_f32 takes it. */
int pn_mlearner_last_bwd_data_f32(const float* g, const float* w3, const float* c, float* dc, int B,
                                  int S, void* stream);
/* part[b*S + y][tap][c] = sum_x F[b][y][x][c] g[b][y + sgn (kh-3)][x + sgn (kw-3)], F [B][S][S][64],
 * g [B][S][S]; column-summed over its B*S rows it is d w3 [49][64] (F = the layer's input, g = d
 * importance, sgn = -1) or (d w1)^T (F = d c1, g = importance_raw, sgn = +1). */
int pn_tapcorr1_f32(const float* F, const float* g, float* part, int B, int S, int sgn,
                    void* stream);
/* Pixel decoder (pairnet_head.py:262; mmcv MultiScaleDeformableAttention.forward): from pn_msda_bwd_f32's
 * grad_sampling_loc / grad_attn_weight back to the gradient of the [offsets 8*L*4*2 | logits 8*L*4]
 * projection rows (stride ld) that pn_token_sampling_f32 turned into those operands on an unpadded
 * batch: d offset = d loc / (W_l, H_l), d logit = aw (d aw - sum aw d aw) per head. */
int pn_msda_offaw_bwd_f32(const float* grad_loc, const float* grad_aw, const float* aw,
                          float* d_offaw, int64_t ld, int64_t rows, int L,
                          const int32_t* level_h /* host */, const int32_t* level_w /* host */,
                          void* stream);
/* Backward of pn_groupnorm_nhwc_f32 (no ReLU) from its INPUT x: dx [B][HW][256] (dense), gxhat = dy *
 * xhat (column sum over B*HW rows: d weight; d bias: column sum of dy); stats: B * G * 4 floats of
 * scratch; x / dy images start at multiples of x_bstride / dy_bstride floats. */
int pn_groupnorm_nhwc_bwd_f32(const float* x, const float* dy, const float* gamma, float* dx,
                              float* gxhat, float* stats, int B, int64_t HW, int G, float eps,
                              int64_t x_bstride, int64_t dy_bstride, void* stream);
/* Backbone backward (mmdet ResNet behind configs/mask2former/pairnet.py:9-19, frozen BatchNorm folded
 * into the convolutions; pair-net_amd/grad.py BackboneGrad) and the Matrix Learner's 64 -> 64 7x7 layer
 * (cnn_factory.py:30-41).  Weight gradient of a K x K convolution
 * (stride, pad) between channel-last maps dY [B][Ho][Wo][Co] and X [B][Hi][Wi][Ci] (Ci, Co % 64 == 0):
 * part[chunk][co][tap][ci] over chunks of rows_per output rows per image, B * ceil(Ho / rows_per)
 * chunks of Co*K*K*Ci floats; their column sum is dW [Co][K*K][Ci]. */
int pn_conv_wgrad_f32(const float* dY, const float* X, float* part, int B, int Hi, int Wi, int Ho,
                      int Wo, int Ci, int Co, int K, int stride, int pad, int rows_per, void* stream);
/* out[b][y][x][:] (+)= in[b][y/2][x/2][:] at even (y, x), 0 elsewhere: [B][Ho][Wo][C] -> [B][Hi][Wi][C] */
int pn_dilate2_f32(const float* in, float* out, int B, int Hi, int Wi, int Ho, int Wo, int C,
                   int accumulate, void* stream);
/* out[b][i][j][:] = in[b][2i][2j][:]: [B][Hi][Wi][C] -> [B][Ho][Wo][C] */
int pn_subsample2_f32(const float* in, float* out, int B, int Hi, int Wi, int Ho, int Wo, int C,
                      void* stream);
/* x[r][0:cols] *= s[r] */
int pn_scale_rows_f32(float* x, const float* s, int64_t rows, int64_t cols, void* stream);
/* Swin backbone backward (csrc/swin_grad.hip; pair-net_amd/grad.py SwinBackboneGrad): the last stage
 * that configs/mask2former/pairnet_swinb.py:201-240 trains (frozen_stages=3: stages.3 + norm3 of
 * [3P] mmdet SwinTransformer).
 * LayerNorm backward over rows of any width C % 4 == 0, C <= 3072 (SwinBlock norm1 / norm2, the
 * stage's output norm3) from the saved INPUT x: dx, and gxhat = dy * xhat whose column sum is
 * d weight (d bias = column sum of dy).  Row strides in floats. */
int pn_layernorm_rows_bwd_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx,
                              const float* gamma, float* dx, int64_t lddx, float* gxhat,
                              int64_t ldg, int64_t rows, int C, float eps, void* stream);
/* Exact (erf) GELU of the Swin FFN (mmcv FFN act_cfg=dict(type='GELU'), between ffn.layers.0.0 and
 * ffn.layers.1): y = x Phi(x), and its backward dx = dy (Phi(x) + x phi(x)) from the saved
 * pre-activation x (dx may alias dy). */
int pn_gelu_f32(const float* x, float* y, int64_t n, void* stream);
int pn_gelu_bwd_f32(const float* dy, const float* x, float* dx, int64_t n, void* stream);
/* Backward of pn_window_attention_f32 (ShiftWindowMSA / WindowMSA.forward), same operand
 * conventions: qkv [B*H*W][ldqkv] and qkv_bias (padding tokens' q/k/v), bias_table [heads][(2ws-1)^2],
 * dout [B*H*W][lddo] the gradient of the attention output, out [B*H*W][ldo] the saved output (or
 * NULL: recomputed) ->
 *   dqkv [B*Hp*Wp][lddqkv]: d q | d k | d v over the PADDED, un-shifted grid (Hp, Wp: H, W rounded
 *     up to multiples of ws).  Every row is written, padding rows included: the reference pads
 *     before the qkv Linear, so their gradient belongs to d qkv.bias (the column sum over all rows);
 *   dtable_part [B][nwin][heads][(2ws-1)^2]: the bias-table gradient of each (image, window, head),
 *     nwin = (Hp/ws)(Wp/ws), to be column-summed (pn_colsum_f32) in a fixed order.
 * No atomics: bitwise reproducible.  ws*ws <= 169; needs (2 N 32 + N (N|1) + (2ws-1)^2 + 3N) * 4
 * bytes of LDS per workgroup (N = ws^2; 163 388 at ws = 13). */
int pn_window_attention_bwd_f32(const float* qkv, int64_t ldqkv, const float* qkv_bias,
                                const float* bias_table, const float* dout, int64_t lddo,
                                const float* out, int64_t ldo, float* dqkv, int64_t lddqkv,
                                float* dtable_part, int B, int H, int W, int C, int heads, int ws,
                                int shift, float scale, void* stream);
/* Backward of pn_patch_merge_ln_f32 ([3P] mmdet PatchMerging: nn.Unfold(2, stride 2) + LayerNorm(4C),
 * before its reduction Linear), for a Swin backbone whose lower stages train
 * (configs/deformable_detr/cross_swinb_vg.py:202-226, frozen_stages=-1; grad.py SwinStagesGrad).
 * Added at ABI 34 (additive).  dy [B*H2*W2][4C] the gradient of the merged, normalised rows
 * (H2 = ceil(H/2), W2 = ceil(W/2)), x [B][H*W][C] the saved un-merged map, gamma [4C] in the
 * forward's neighbour-major order ->
 *   dx [B][H*W][C]: every row written exactly once (accumulate != 0: added to what is there -- the
 *     stage output also feeds its output norm).  The gradient of the zero padding beyond an odd
 *     map's edge is dropped; the padding still counts in the rows' moments and backward sums;
 *   part [nblocks][2][4C]: per-workgroup sums of dy xhat | dy, neighbour-major; their column sum
 *     (pn_colsum_f32 over nblocks rows of 8C floats) is d gamma | d beta.
 * nblocks (the launch's workgroups, 1 .. 65535; any value is correct): pair-net_amd/hip.py
 * patch_merge_ln_bwd_nblocks gives min(ceil(rows / 4), 512).  The gathered [rows][4C] input is never
 * formed; no atomics, two launches give equal bits.  Refuses (-1, nothing written) C % 4 != 0,
 * 4C > 3072, B / H / W < 1, null or mis-aligned (16 B) pointers. */
int pn_patch_merge_ln_bwd_f32(const float* dy, const float* x, const float* gamma, float* dx,
                              float* part, int nblocks, int B, int H, int W, int C, float eps,
                              int accumulate, void* stream);
/* out[ci][T-1-t][co] = in[co][t][ci]: a "same" convolution's weight as its data gradient reads it */
int pn_conv_weight_bwd_layout_f32(const float* in, float* out, int Co, int T, int Ci, void* stream);
/* Training-mode dropout of the Relation Fusion decoder's FFN (csrc/dropout.hip): mmcv FFN.layers'
 * two nn.Dropout(ffn_drop) -- after the ReLU on the hidden rows and on the FFN's output before the
 * identity shortcut -- under configs/mask2former/pairnet.py:121-129 (relation_decoder ffn_cfgs
 * ffn_drop=0.1; every other rate of that file is 0.0).  Stateless: the keep bit of element i is
 * word i % 4 of Philox4x32-10 at counter (i / 4, subseq, site, step), key (seed & 0xffffffff,
 * seed >> 32), kept <=> word >= (uint32)((double)p * 2^32); no mask is stored, the backward pass is
 * the same call on the gradient.  With s = (float)(1 / (1 - (double)p)):
 *   y[i] = kept ? x[i] * s : 0            (res == NULL)
 *   y[i] = kept ? fmaf(x[i], s, res[i]) : res[i]
 * y may alias x.  x / res / y 16-byte aligned, 0 < n <= 2^34, 0 <= p < 1 (p == 0: y == x resp.
 * x + res bitwise). */
int pn_dropout_f32(const float* x, const float* res /* may be NULL */, float* y, int64_t n, float p,
                   uint64_t seed, uint32_t subseq, uint32_t step, uint32_t site, void* stream);
/* keep[i] = 1 where pn_dropout_f32 with the same (p, seed, subseq, step, site) keeps element i, else
 * 0 (the mask made visible: tests, the float64 gradient oracle; same nn.Dropout call sites). */
int pn_dropout_keep_u8(uint8_t* keep, int64_t n, float p, uint64_t seed, uint32_t subseq,
                       uint32_t step, uint32_t site, void* stream);

/* ------------------------------------------------------------------------- *
 * The optimizer step (csrc/optim.hip) over one flat fp32 parameter buffer: what mmcv's
 * OptimizerHook(grad_clip=dict(max_norm=0.1, norm_type=2)) + torch.optim.AdamW do per iteration
 * (configs/mask2former/pairnet.py:353-368; paramwise lr_mult / norm_decay_mult as per-segment
 * multipliers).  pair-net_amd/train.py drives it.
 * ------------------------------------------------------------------------- */
/* out[0] = || pre * g ||_2, out[1] = min(1, max_norm / (out[0] + 1e-6)) (1 if max_norm <= 0);
 * scratch: 256 doubles.  Deterministic (two-stage sum in double, fixed order). */
int pn_grad_norm_clip_f32(const float* g, int64_t n, float pre, float max_norm, float* out,
                          double* scratch, void* stream);
/* AdamW (torch.optim.AdamW's arithmetic) on p / g / m / v [n] with the effective gradient
 * pre * clip[1] * g (clip: the device pair written by pn_grad_norm_clip_f32, or NULL); segment s
 * covers [seg_off[s], seg_off[s+1]) and uses lr * seg_lr[s], weight_decay * seg_wd[s]; `step`
 * counts from 1 (bias corrections).  The betas are doubles (ABI 34): 1 - beta, 1 - beta^step and
 * sqrt(1 - beta2^step) are formed in double and rounded to fp32 once, as torch forms the scalars
 * it applies to fp32 tensors.  0 <= beta < 1, step >= 1, n > 0. */
int pn_adamw_f32(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* seg_off,
                 const float* seg_lr, const float* seg_wd, int nseg, float lr, double beta1,
                 double beta2, float eps, float weight_decay, int step, const float* clip, float pre,
                 void* stream);
/* pn_adamw_f32 behind a device-side guard (ABI 33): with *guard != 0 -- pn_loss_targets' batch status:
 * a cost matrix on which `linear_sum_assignment` (matcher.py:262-264) raises in the reference, before
 * any parameter moves -- nothing is read or written, so p / m / v stay bitwise as they are. */
int pn_adamw_guarded_f32(float* p, const float* g, float* m, float* v, int64_t n,
                         const int64_t* seg_off, const float* seg_lr, const float* seg_wd, int nseg,
                         float lr, double beta1, double beta2, float eps, float weight_decay,
                         int step, const float* clip, float pre, const int32_t* guard, void* stream);

/* ------------------------------------------------------------------------- *
 * fp32 GEMMs on the bf16 matrix pipe from PRE-SPLIT operands (csrc/gemm_s3.hip, round 6)
 *
 * Arithmetic: every fp32 number is exactly x0 + x1 + x2 with bf16 pieces (each the
 * round-to-nearest-even bf16 of what is left); a product of bf16 numbers is exact in fp32; of the
 * nine piece products of a*b the six largest are summed by v_mfma_f32_32x32x16_bf16 into fp32
 * accumulators, the three dropped ones are together < 2^-26 |ab|.  Measured against fp64 the
 * result is at or below the error of the exact-fp32 MFMA of pn_gemm_f32 on every shape of the
 * path (profiles/r06_gemm_s3_error.txt).  Same call sites as pn_gemm_f32 /
 * pn_linear_res_ln_f32 for the pixel decoder's encoder (value_proj / sampling_offsets /
 * attention_weights / output_proj / FFN behind pairnet_head.py:262).
 *
 * "S3" operand of an [R x K] matrix (K % 16 == 0): blocks of 32 rows x 16 k, block (rb, kb) at
 * byte (rb * K/16 + kb) * 3072; three 1 KiB planes (x0, x1, x2) per block; inside a plane 16
 * bytes (8 consecutive k) per MFMA lane, lane = (k % 16 / 8) * 32 + r % 32.  Rows are padded to
 * a multiple of 32 (pn_s3_bytes); A and W operands use the same layout.
 * ------------------------------------------------------------------------- */
int64_t pn_s3_bytes(int rows, int K);
/* S = split(X[r][0:K] + add[r % add_rows][0:K]) for fp32 rows X [rows][ld] (add may be NULL;
 * ld % 4 == 0, 16-byte aligned).  Rows of the last block beyond `rows` are written as zeros. */
int pn_s3_split_f32(const float* X, int64_t ld, const float* add, int add_rows, void* S, int rows,
                    int K, void* stream);
/* Both at once from one read of X: S = split(X), S_add = split(X + add[r % add_rows]) (add
 * required); bit for bit the two pn_s3_split_f32 calls. */
int pn_s3_split2_f32(const float* X, int64_t ld, const float* add, int add_rows, void* S, void* S_add,
                     int rows, int K, void* stream);
/* The exact fp32 values back: X[r][0:K] = x0 + x1 + x2. */
int pn_s3_join_f32(const void* S, float* X, int64_t ld, int rows, int K, void* stream);
/*   out[m][n] = act( sum_k A*[m][k] W[n][k] + bias[n] ),   A* = A2 for n >= a2_from_col, else A
 * or, with gamma != NULL (N == 256):
 *   out[m][:] = LayerNorm(sum_k A[m][k] W[:][k] + bias + res[m][:]) * gamma + beta
 * (two-pass moments, eps inside the square root: [3P] nn.LayerNorm).  Any subset of three outputs:
 *   C      fp32 rows [M][ldc]
 *   CS     S3 [M x N] of out                      (the next GEMM's A operand)
 *   CS_pos S3 [M x N] of out + pos[m % pos_rows]  (the next layer's query operand, `query + query_pos`)
 * A, A2, W, res_s3 are S3 operands ([M x K], [M x K], [N x K], [M x 256]); K % 32 == 0, N % 32 == 0,
 * a2_from_col % 256 == 0.  pos is in "P8" order: [pos_rows / 32][N / 16][2][32][8] (the S3 piece
 * order with fp32 elements; pair-net_amd/hip.py pos8()).  One workgroup of 8 waves per 96 x 256 tile
 * (192 x 256 with W shared by two row groups when N >= 512 and there is no row epilogue); up to 64
 * columns beyond the last whole 256-column tile go to a one-wave-per-block kernel. */
typedef struct pn_gemm_s3_desc {
  const void* A;  const void* A2;  int32_t a2_from_col;
  const void* W;  const float* bias;            /* bias [N] or NULL */
  int32_t M, N, K;
  int32_t relu;
  float* C;       int64_t ldc;
  void* CS;
  void* CS_pos;   const float* pos;  int32_t pos_rows;   /* pos [pos_rows][N] fp32 */
  const void* res_s3;  const float* gamma;  const float* beta;  float eps;
  int32_t flags;                                 /* PN_GEMM_S3_* (tuning / tests), else 0 */
  /* plain epilogue only (round 6, the Swin blocks): out = act(sum + bias) + res[m][n]; act 0 = `relu`
   * decides, 1 ReLU, 2 exact (erf) GELU, 3 = relu(sum + bias + res) (ReLU after the shortcut: a
   * ResNet bottleneck's last convolution); res fp32 rows [M][ldres] or NULL */
  int32_t act;  const float* res;  int64_t ldres;
} pn_gemm_s3_desc;
#define PN_GEMM_S3_TILE96 1   /* force the 96 x 256 tile where the 192 x 256 one would be taken */
#define PN_GEMM_S3_TILE192 2  /* force the 192 x 256 tile (N >= 512, plain epilogue) whatever its tile count */
int pn_gemm_s3_f32(const pn_gemm_s3_desc* d, void* stream);
/* The encoder's FFN as ONE launch (k_gemm_s3_ffn):
 *   out[m][:] = LayerNorm(relu(X[m][:] W1^T + b1) W2^T + b2 + res[m][:]) * gamma + beta
 * X [M x K], W1 [F x K], W2 [N x F], res_s3 [M x N] are S3 operands; C / CS / CS_pos / pos as in
 * pn_gemm_s3_desc.  The F hidden values of a row stay on the chip: a 96-row tile forms them 256
 * columns at a time in registers, pre-split, and hands them to the second GEMM through LDS.
 * Every output is bit for bit that of the two pn_gemm_s3_f32 calls (act = ReLU -> CS, then res_s3 +
 * LayerNorm) it replaces.  Handled: K == 256, N == 256, F % 256 == 0, act == 1 (ReLU), gamma and
 * beta given; anything else returns PN_BAD_ARG without launching. */
typedef struct pn_gemm_s3_ffn_desc {
  const void* X;  const void* W1;  const float* b1;    /* b1 [F] or NULL */
  const void* W2; const float* b2;                      /* b2 [N] or NULL */
  int32_t M, N, K, F;
  int32_t act;                                          /* pn_gemm_s3_desc's codes; 1 (ReLU) only */
  float* C;       int64_t ldc;
  void* CS;
  void* CS_pos;   const float* pos;  int32_t pos_rows;
  const void* res_s3;  const float* gamma;  const float* beta;  float eps;
} pn_gemm_s3_ffn_desc;
int pn_gemm_s3_ffn_f32(const pn_gemm_s3_ffn_desc* d, void* stream);
/* pn_gemm_s3_f32's LayerNorm form with the activation operand as fp32 ROWS (k_gemm_s3_rows):
 *   out[m][:] = LayerNorm(sum_k A[m][k] W[:][k] + bias + res[m][:]) * gamma + beta
 * A fp32 [M][lda] (lda % 4 == 0, lda >= K, 16-byte aligned); W [N x K] and res_s3 [M x N] are S3
 * operands; C / CS / CS_pos / pos as in pn_gemm_s3_desc.  The tile's waves split the rows into the
 * three bf16 planes on their way into LDS, so the pn_s3_split_f32 pass in front of the GEMM and its
 * S3 buffer are not needed.  Only rows 0 .. M-1 of A are read; the rows that pad the last row block
 * enter as zeros, as pn_s3_split_f32 writes them.  Every output, padding rows of CS / CS_pos
 * included, is bit for bit that of pn_s3_split_f32 -> pn_gemm_s3_f32 (gamma given).  Handled:
 * N == 256, K % 32 == 0, gamma and beta given, act == 0; anything else returns PN_BAD_ARG without
 * launching. */
typedef struct pn_gemm_s3_rows_desc {
  const float* A;  int64_t lda;
  const void* W;   const float* bias;                   /* bias [N] or NULL */
  int32_t M, N, K;
  int32_t act;                                          /* 0 only */
  float* C;        int64_t ldc;
  void* CS;
  void* CS_pos;    const float* pos;  int32_t pos_rows;
  const void* res_s3;  const float* gamma;  const float* beta;  float eps;
} pn_gemm_s3_rows_desc;
int pn_gemm_s3_rows_ln_f32(const pn_gemm_s3_rows_desc* d, void* stream);

/* ------------------------------------------------------------------------- *
 * The Mask2Former segmentation losses (csrc/seg_loss.hip; pair-net_amd/seg_losses.py drives them):
 * per-decoder-layer loss_cls / loss_mask / loss_dice with Hungarian matching per (layer, image),
 * importance-sampled mask points and deep supervision, values and d loss / d logits -- the
 * reference's panoptic_heads/mask2former_head.py:157-324 with maskformer_head.py:181-240,305-354
 * (again in relation_heads/baseline.py:588-653) under configs/mask2former/baseline_r50_psg.py:351-389.
 * The matching itself is pn_point_sample_f32 + pn_mask_match_cost_f32 + ONE pn_lsa_f32 launch over
 * the L * B problems.  Fixed-order reductions, no floating-point atomics: bitwise reproducible.
 * Entries added at ABI 34 (adding entries is compatible).
 * ------------------------------------------------------------------------- */
/* The `torch.rand` draws of mask2former_head.py:191 and point_sample.py:61,84-86 as a pure function
 * of their arguments: out[s][i] = (word >> 8) * 2^-24 in [0, 1), word = output word i % 4 of
 * Philox4x32-10 at counter (i / 4, rank, site + s * site_stride, step), key (seed & 0xffffffff,
 * seed >> 32) -- csrc/dropout.hip's scheme.  out [nsites][n]; 0 < n <= 2^34, 0 < nsites <= 65535. */
int pn_uniform_f32(float* out, int64_t n, int nsites, uint32_t site_stride, uint64_t seed,
                   uint32_t rank, uint32_t step, uint32_t site, void* stream);
/* `_get_target_single`'s bookkeeping (mask2former_head.py:205-221 with MaskPseudoSampler) for the
 * P = L * B problems of one pn_lsa_f32 launch.  table [P][6] int64 on the device, problem p = l * B + b:
 * {index of the problem in lsa_status, or -1 for an image without ground truth; offset of its
 * entries in row_ind / col_ind; their number n = min(Q, G); offset of the image's labels in
 * gt_labels; G; offset of its n rows in `matched`}.  Writes
 *   labels [L][B * Q] int64: the matched ground truth's class, num_classes = C for the rest;
 *   matched [Mtot][4] int64: (layer, image, query, index into gt_labels / the concatenated
 *     ground-truth masks) ordered by (layer, image, query ascending) -- the order of
 *     `mask_preds[mask_weights > 0]` and of the concatenated `mask_targets` (:263,283);
 *   mcount [L] int32: assigned rows per layer;  status [1] int32: the OR of the problems'
 *     lsa_status, | 4 for an index or label out of range, | 8 for a table row out of range.
 * A problem with a non-zero status keeps its fills (labels C, matched rows -1).  L <= 64. */
int pn_seg_targets(const int64_t* table, const int32_t* row_ind, const int32_t* col_ind,
                   const int32_t* lsa_status, int nlsa, const int64_t* gt_labels, int64_t gt_len,
                   int64_t out_len, int L, int B, int Q, int C, int64_t Mtot, int64_t* labels,
                   int64_t* matched, int32_t* mcount, int32_t* status, void* stream);
/* get_uncertain_point_coords_with_randomness (panoptic_heads/point_sample.py:32-88) for the M
 * matched masks, one workgroup each: row m samples map (l * B + b) * Q + q of maps [nmaps][h][w]
 * (its `matched` row) at cand [M][S][2], keeps the k candidates with the smallest |logit| (what
 * `torch.topk(-|x|, k)` keeps; exact, ties to the lower candidate index) and writes them in
 * ascending candidate order, followed by tail [M][Np - k][2], to pts [M][Np][2].  keys [M][S]
 * uint32: the sampled |logit| bit patterns (scratch of the four-pass radix select; readable
 * afterwards).  A row with layer < 0: zeros.  0 <= k <= Np, k <= S; tail may be NULL iff k == Np. */
int pn_uncertain_points_f32(const float* maps, int64_t nmaps, const int64_t* matched, int64_t M,
                            int B, int Q, int h, int w, const float* cand, const float* tail, int S,
                            int k, int Np, uint32_t* keys, float* pts, void* stream);
/* [3P] mmcv point_sample with a point set PER ROW (mask2former_head.py:300-306): out[m][i] = map
 * idx[m] of maps [nmaps][h][w] (fp32, or uint8 0/1) sampled at pts[m][i] with pn_point_sample_f32's
 * arithmetic (bilinear, zeros padding, align_corners=False); idx[m] outside [0, nmaps): zeros.
 * M <= 65535. */
int pn_point_sample_rows_f32(const void* maps, int maps_are_u8, int64_t nmaps, const int64_t* idx,
                             const float* pts, float* out, int64_t M, int h, int w, int Np,
                             void* stream);
/* loss_mask ([3P] sigmoid CrossEntropyLoss) and loss_dice ([3P] DiceLoss: use_sigmoid, activate,
 * naive_dice) of L layers over x / t [M][Np], M = L * Ml rows in `matched` order
 * (mask2former_head.py:308-322), s = sigmoid(x):
 *   sums [M][4] = { sum_p BCE(x, t), a = sum_p s t, b = sum_p s, c = sum_p t }
 *   out[l]     = w_mask * sum_m sums[m][0] / (N_l * Np + eps32)
 *   out[L + l] = w_dice * sum_m (1 - (2 a + dice_eps) / (b + c + dice_eps)) / (N_l + eps32)
 *   out[2L + l], out[3L + l]: the two denominators
 * N_l = num_total_masks when > 0, else max(assigned rows of layer l, 1) (:278-279); rows with layer
 * < 0 are skipped.  coef [M][Np] (or NULL) = d (out[l] + out[L + l]) / d x[m][p]. */
int pn_mask_point_loss_f32(const float* x, const float* t, const int64_t* matched, int64_t M, int Np,
                           int L, int Ml, float w_mask, float w_dice, float dice_eps,
                           float num_total_masks, float* sums, float* out /* [4L] */, float* coef,
                           void* stream);
/* The transpose of the bilinear sample (the backward of mask2former_head.py:304): grad [M][h][w] =
 * sum over row m's points of coef[m][p] * the tap weight, taps outside the map dropped.  No
 * floating-point atomics: per mask, a stable counting sort of the points by the pixel of their
 * top-left tap, then every pixel sums its up-to-four bins in that order.  scratch:
 * pn_point_scatter_scratch_ints(M, Np, h, w) int32. */
int64_t pn_point_scatter_scratch_ints(int64_t M, int Np, int h, int w);
int pn_point_scatter_grad_f32(const float* coef, const float* pts, float* grad, int32_t* scratch,
                              int64_t M, int Np, int h, int w, void* stream);
/* loss_cls of L layers (mask2former_head.py:273-276; [3P] mmdet CrossEntropyLoss with class weights,
 * avg_factor = class_weight[labels].sum(), weight_reduce_loss's eps32):
 *   out[l] = loss_weight * sum_r cw[y] (lse(x_r) - x_r[y]) / (sum_r cw[y] + eps32)
 *   grad[l][r][c] = loss_weight * cw[y] / (sum_r cw[y] + eps32) * (softmax(x_r)[c] - [c == y])
 * logits / grad [L][rows][C] contiguous, target [L][rows] in [0, C), class_weight [C];
 * rows <= 4096; one workgroup per layer, rows summed in row order. */
int pn_ce_avg_f32(const float* logits, const int64_t* target, const float* class_weight, float* out,
                  int L, int rows, int C, float loss_weight, void* stream);
int pn_ce_avg_grad_f32(const float* logits, const int64_t* target, const float* class_weight,
                       float* grad, int L, int rows, int C, float loss_weight, void* stream);

/* ------------------------------------------------------------------------- *
 * The relation terms of the sibling head's loss (csrc/rel_loss.hip; pair-net_amd/baseline_losses.py
 * drives them): r_loss_cls, loss_subject_match and loss_object_match of the reference's
 * relation_heads/baseline.py:655-694, 828-907 under configs/mask2former/baseline_r50_psg.py:336-350,
 * 373-378, last decoder layer only (baseline.py:523-526), values and d loss / d logits.  The
 * assignment is ONE pn_lsa_f32 launch over the B images; r_loss_cls is pn_ce_avg_f32 /
 * pn_ce_avg_grad_f32 with L = 1 on the labels written here.  Fixed-order reductions, no
 * floating-point atomics.  Entries added at ABI 34 (adding entries is compatible).
 *
 * tab [B][8] int64 on the device, one row per image: {offset of its R x Gr block in `cost`, Gr,
 * offset of its rows in gt_rels [rel_len][3] = (subject object, object object, predicate), offset
 * of its last-layer rows in pn_seg_targets' `matched` [Mtot][4], their number n = min(Q, G), offset
 * of its objects in the concatenated ground truth (what matched[.][3] counts from), G, offset of
 * its P = min(R, Gr) entries in row_ind / col_ind / pos / row_loss}.  Q, R, G <= 1024.
 * ------------------------------------------------------------------------- */
/* OldIdMatcher's cost (approaches/matcher.py:323-330, ClassificationCost three times) for every
 * image in one launch, laid out as pn_lsa_f32's table wants:
 *   cost[r][k] = (-w_s softmax(sub[b][r])[a[s_k]] - w_o softmax(obj[b][r])[a[o_k]])
 *                - w_r softmax(rel[b][r])[p_k]
 * a = ones_like(gt_labels); a[pos_assigned_gt_inds] = od_pos_inds (baseline.py:829-830), read from
 * the image's `matched` rows.  rel [B][R][C1], sub / obj [B][R][Q].  An image whose matched rows
 * are -1 (its segmentation assignment failed) gets zeros. */
int pn_rel_id_cost_f32(const float* rel, const float* sub, const float* obj, const int64_t* gt_rels,
                       int64_t rel_len, const int64_t* matched, int64_t Mtot, const int64_t* tab,
                       float* cost, int64_t cost_len, int B, int R, int Q, int C1, float w_s,
                       float w_o, float w_r, void* stream);
/* The targets behind the id assignment (baseline.py:866-907): r_labels [B * R] int64 = the matched
 * relation's predicate, 0 for the rest; pos [out_len][4] int32 = (image, relation row, position of
 * the subject's query among the image's matched queries, the object's) per positive row in
 * ascending row order (:883-897), -1 for an image that was skipped.  status [1] int32: the OR of
 * pn_lsa_f32's status of every image, | 4 an index or predicate out of range, | 8 a table row out
 * of range, | 16 a related object's query is not among the matched queries (the reference raises
 * at :886), | 32 the image's last-layer segmentation assignment failed.  An image with a non-zero
 * status keeps its fills. */
int pn_rel_targets(const int64_t* tab, const int32_t* row_ind, const int32_t* col_ind,
                   int64_t out_len, const int32_t* lsa_status, const int64_t* gt_rels,
                   int64_t rel_len, const int64_t* matched, int64_t Mtot, int B, int R, int Q, int C1,
                   int64_t* r_labels, int32_t* pos, int32_t* status, void* stream);
/* loss_subject_match / loss_object_match (baseline.py:655-682): MultilabelCrossEntropy
 * (losses/seg_losses.py:47-57) with a one-hot target on scores[pos_inds][:, od_pos_inds], mean over
 * the image's P rows times the loss weight, then the mean over the B images:
 *   row_loss [pos_len][2] = lse over the n matched columns - the target column's score
 *   out [2] = (1 / B) sum_b w * (sum_i row_loss / P_b), rows then images in ascending order
 *   g_sub / g_obj [B][R][Q] (both or neither NULL) = w / (B P_b) (softmax - onehot) in the matched
 *   columns of the positive rows, 0 everywhere else: every element is written. */
int pn_id_ce_f32(const float* sub, const float* obj, const int64_t* matched, int64_t Mtot,
                 const int64_t* tab, const int32_t* pos, int64_t pos_len, int B, int R, int Q,
                 float w_s, float w_o, float* row_loss, float* out, float* g_sub, float* g_obj,
                 void* stream);

/* -------------------------------------------------------------------------
 * The box head's object assignment cost (csrc/box_loss.hip; pair-net_amd/bbox_losses.py drives it):
 * `self.bbox_assigner.assign(bbox_pred, cls_score, gt_bboxes, gt_labels, img_metas, ...)` at
 * pairnet_bbox_head.py:863-865 -- [3P] mmdet HungarianAssigner under configs/deformable_detr/
 * cross_r101_vg.py:158-163 (FocalLossCost 2.0, BBoxL1Cost 5.0 xywh, IoUCost giou 2.0) -- for every
 * image of the batch in one launch, laid out as pn_lsa_f32's table wants.  Entry added at ABI 34
 * (adding entries is compatible).
 *   cls [B][Q][nc] the kept queries' class logits, box [B][Q][4] cxcywh normalised;
 *   gt_labels [labels_len] int64 and gt_bboxes [boxes_len][4] fp32 (xyxy, pixels): the batch's
 *   concatenated ground truth; factor [B][4] = (img_w, img_h, img_w, img_h) of `img_shape`;
 *   tab [B][4] int64 on the device = {offset of the image's row-major Q x G block in cost, G, offset
 *   of its labels in gt_labels, offset of its boxes in gt_bboxes (in boxes)}.
 * For query q and ground truth g, in fp32 and in this order, without fused multiply-adds:
 *   p        = sigmoid(cls[q][label_g])
 *   cls_cost = ((-log(p + eps)) alpha (1 - p)^gamma - (-log((1 - p) + eps)) (1 - alpha) p^gamma) w_cls
 *   reg_cost = (sum_i |box[q][i] - cxcywh(gt_g / factor)[i]|) w_reg
 *   iou_cost = (-GIoU(xyxy(box[q]) * factor, gt_g)) w_iou      (mmdet bbox_overlaps: union and
 *              enclosing area clamped to >= iou_eps)
 *   cost     = (cls_cost + reg_cost) + iou_cost
 * One cell per lane, no atomics, bitwise reproducible.  max_cells: the largest Q * G of the table,
 * known from shapes (sizes the grid; cells past it are not written).  A table row outside a buffer
 * or with G outside [1, 1024] leaves its block untouched; a label outside [0, nc) gives a NaN cell
 * (pn_lsa_f32 status 1); a NaN operand gives a NaN cell.  2 <= Q <= 1024, nc <= 256. */
int pn_box_match_cost_f32(const float* cls, const float* box, const int64_t* gt_labels,
                          int64_t labels_len, const float* gt_bboxes, int64_t boxes_len,
                          const float* factor, const int64_t* tab, float* cost, int64_t cost_len,
                          int64_t max_cells, int B, int Q, int nc, float w_cls, float w_reg,
                          float w_iou, float alpha, float gamma, float eps, float iou_eps,
                          void* stream);

/* -------------------------------------------------------------------------
 * The triplet matching of PSGTrHead2's loss (csrc/tri_loss.hip; pair-net_amd/psgtr2_losses.py drives
 * it): `_get_target_single` of relation_heads/psgtr_head2.py:879-1018 with `MaskHTriMatcher.assign`
 * of approaches/matcher.py:29-102 under configs/psgtr/psgtr_r50_psg_plus.py:162-177, for every image
 * of the batch.  The assignment is ONE pn_lsa_f32 launch over the B images; the seven loss terms
 * behind it are pn_ce_avg_f32 and the per-mask point entries of csrc/seg_loss.hip, unchanged.
 * Fixed-order reductions, no floating-point atomics.  Entries added at ABI 34 (adding entries is
 * compatible).
 *
 * tab [B][8] int64 on the device, one row per image: {offset of its row-major Q x R_b block in
 * `cost`, R_b, offset of its rows in gt_rels [rel_len][3] = (subject object, object object,
 * predicate), offset of its objects in the concatenated ground truth (labels [SG], masks
 * [SG][hg][wg]), G_b, offset of its min(Q, R_b) entries in row_ind / col_ind / matched, 0, 0}.
 * ------------------------------------------------------------------------- */
/* MaskHTriMatcher's cost (matcher.py:67-83; psgtr_head2.py:909-934 for the samples) of every image,
 * laid out as pn_lsa_f32's table wants: for query q and relation k = (so, oo, p) of image b
 *   cost[q][k] = s_cls + s_mask + s_dice + o_cls + o_mask + o_dice + r_cls, added left to right,
 *   x_cls  = -softmax(logits[b][q])[label] * w           (ClassificationCost; label = gt_labels[so],
 *            gt_labels[oo], p on sub_cls / obj_cls [B][Q][C1] and rel_cls [B][Q][Cr1])
 *   x_mask = (sum_i BCE(x_i, 0) - sum_i x_i t_i) / Np * w        (CrossEntropyLossCost, sigmoid)
 *   x_dice = (1 - (2 sum_i s_i t_i + eps) / (sum_i s_i + sum_i t_i + eps)) * w,  s = sigmoid(x)
 * with x = the query's mask logits (sub_maps / obj_maps [B][Q][h][w], two bases) and t = the
 * object's uint8 mask [hg][wg], both sampled (mmcv point_sample) at the image's points pts
 * [B][Np][2], which subject and object, predictions and ground truth share (:909).  The mask and
 * dice terms are computed once per (side, query, OBJECT) and gathered per relation: mask work is
 * proportional to Q * G_b.  weights (HOST pointer, read before the launches) [9] = s_cls, s_mask,
 * s_dice, o_cls, o_mask, o_dice, r_cls weights, then the s and o dice eps.  Scratch, written in
 * full for every object / row in range: t [SG][Np], tsum [SG], stats [3][B * Q][2], pair
 * [2][SG][Q][2], part [part_floats >= 4 (SG + B) Q pn_tri_pair_splits(B, Q, Np)] (the pair sums of
 * every split of the points, added in ascending split order).  max_G / max_cells: the largest G_b
 * and Q * R_b, known from shapes (they size the grids).  Five launches whatever B, sum R_b and
 * sum G_b are.  A relation whose objects, predicate
 * or labels are out of range gives NaN cells, as a NaN operand does (pn_lsa_f32 status 1); a table
 * row outside a buffer leaves its block untouched. */
int pn_tri_match_cost_f32(const float* sub_cls, const float* obj_cls, const float* rel_cls,
                          const float* sub_maps, const float* obj_maps, const uint8_t* gt_masks,
                          const float* pts, const int64_t* gt_rels, int64_t rel_len,
                          const int64_t* gt_labels, int64_t SG, const int64_t* tab, int B, int Q,
                          int C1, int Cr1, int h, int w, int hg, int wg, int Np, int max_G,
                          int64_t max_cells, const float* weights, float* t, float* tsum,
                          float* stats, float* pair, float* part, int64_t part_floats, float* cost,
                          int64_t cost_len, void* stream);
/* The number of point splits pn_tri_match_cost_f32 uses for its pair sums: a function of the shapes
 * alone (whole 256-point chunks per split, at most 16), so the summation order is too. */
int pn_tri_pair_splits(int B, int Q, int Np);
/* The targets behind the assignment (psgtr_head2.py:967-997, MaskPseudoSampler: positives in
 * ascending query order): labels [3][B * Q] int64 = sub | obj | rel labels with the fills C, C, Cr
 * (:971-984: the relation fill is num_relations, the LAST index); matched [M][4] int64 = (image,
 * query, subject object, object object), objects counted over the batch; side_rows [2][M][4] int64 =
 * (0, image, query, object) per side, the row layout pn_uncertain_points_f32 and
 * pn_mask_point_loss_f32 read with L = 1; rel_idx [M] int64 = the matched relation's index in its
 * image; mcount [1] = the matched rows written; M = sum_b min(Q, R_b).  status [1] int32: the OR of
 * pn_lsa_f32's status of every image, | 4 a relation's object outside [0, G_b), predicate outside
 * [1, Cr], object label outside [0, C) or an assignment index out of range, | 8 a table row out of
 * range.  An image with a non-zero status keeps its fills and its matched rows -1. */
int pn_tri_targets(const int64_t* tab, const int32_t* row_ind, const int32_t* col_ind,
                   int64_t out_len, const int32_t* lsa_status, const int64_t* gt_rels,
                   int64_t rel_len, const int64_t* gt_labels, int64_t SG, int B, int Q, int C, int Cr,
                   int64_t M, int64_t* labels, int64_t* matched, int64_t* side_rows,
                   int64_t* rel_idx, int32_t* mcount, int32_t* status, void* stream);

/* -------------------------------------------------------------------------
 * Backward of the mask logits (csrc/seg_grad.hip): the two products that differentiate
 *   mask_pred = torch.einsum("bqc,bchw->bqhw", mask_embed, mask_feature)
 * (pairnet_head.py:236-243 / baseline.py:254-296, once per decoder layer) from the COMPACT gradient
 * the segmentation loss returns: G [M][P] fp32 (P = h * w) for the matched rows only and mask_rows
 * [M] int64, their row in the [me_rows = L * B * Q][256] mask embeddings, -1 for a row whose
 * assignment failed.  Row m = l * Ml + m_off[b] + j, so the host knows every row's image from L, B
 * and n_b alone and passes `table` (int32, device): [img_off (B + 1) | order (M) | tiles (2 T)] --
 * order = the rows grouped by image (image b owns order[img_off[b] .. img_off[b + 1]), layers
 * ascending), tiles = (image, offset into order) of T row tiles of at most 32 entries of one image
 * (kernel 1 only).  fp32 operands and accumulation on v_mfma_f32_32x32x2_f32, fixed summation
 * order, no float atomics: the same inputs give the same bits.  Both write their whole output.  A
 * row with mask_rows[m] < 0 contributes nothing and its G row is not read.  M <= 65535.
 * ------------------------------------------------------------------------- */
/* pixels per split-K slice of pn_mask_embed_grad_f32 (a constant: the slicing depends on P alone) */
int pn_mask_grad_kslice(void);
/* floats of pn_mask_embed_grad_f32's scratch: ceil(P / kslice) slices of [T * 32][256] */
int64_t pn_mask_embed_grad_scratch_floats(int T, int64_t P);
/* d mask_embed: dme[m][c] = sum_p G[m][p] * MF[b(m)][p][c], MF [B][P][256]; dme [M][256], a failed
 * row comes out as exact zeros.  Per slice an ascending fmaf chain over its pixels, then the slices
 * are added in ascending order. */
int pn_mask_embed_grad_f32(const float* G, const float* MF, const int64_t* mask_rows,
                           const int32_t* table, int64_t table_len, int M, int B, int T, int64_t P,
                           float* scratch, int64_t scratch_floats, float* dme, void* stream);
/* d mask_feature: dMF[b][p][c] = sum over image b's rows m (in `order`) of
 * G[m][p] * me[mask_rows[m]][c]; dMF [B][P][256], zeros for an image without rows.  One ascending
 * fmaf chain per element.  `tiles` is not read (table_len >= B + 1 + M). */
int pn_mask_feature_grad_f32(const float* G, const float* me, const int64_t* mask_rows,
                             const int32_t* table, int64_t table_len, int M, int B, int64_t P,
                             int64_t me_rows, float* dMF, void* stream);

/* -------------------------------------------------------------------------
 * Backward of PSGTrHead2's three class heads (csrc/tri_grad.hip; psgtr_head2.py:309-324:
 * sub_cls_embed, obj_cls_embed, rel_cls_embed on the same post-normed rows qn [N][256], N = B * Q):
 *   dqn[n][:]  = (add ? dqn[n][:] : 0) + sum_j dsub[n][j] Wsub[j][:] + sum_j dobj[n][j] Wobj[j][:]
 *                                      + sum_j drel[n][j] Wrel[j][:]
 *   dW_h[j][:] = sum_n d_h[n][j] qn[n][:]      db_h[j] = sum_n d_h[n][j]      h in {sub, obj, rel}
 * dsub / dobj [N][C1], drel [N][Cr1] contiguous as the loss writes them (no padding), W_h / dW_h
 * [width][256] in the reference's layout, db_h [width]; dW_h and db_h are written whole.  Two
 * launches on v_mfma_f32_32x32x2_f32 (fp32 operands and accumulation): a row-tile kernel for dqn
 * that contracts over the columns of sub, obj, rel in this order, each ascending, and a
 * column-tile kernel for dW / db that contracts over n ascending.  Ragged edges are predicated in
 * the kernels; no float atomics; the same inputs give the same bits.  channels == 256, N <= 4096,
 * C1 <= 256, Cr1 <= 64, add in {0, 1}; anything else returns -1 before a launch.
 * ------------------------------------------------------------------------- */
int pn_triplet_heads_bwd_f32(const float* dsub, const float* dobj, const float* drel,
                             const float* qn, const float* Wsub, const float* Wobj,
                             const float* Wrel, float* dqn, float* dWsub, float* dbsub,
                             float* dWobj, float* dbobj, float* dWrel, float* dbrel, int N,
                             int channels, int C1, int Cr1, int add, void* stream);

/* ---- backward of the pixel decoder's FPN branch (MSDeformAttnPixelDecoder.forward behind
 * pairnet_head.py:262: lateral_convs.0 -> + bilinear-up(finest memory) -> output_convs.0 ->
 * mask_feature; pair-net_amd/seg_grad.py SegPixelDecoderGrad).  No float atomics: bitwise
 * reproducible. ---- */
/* Adjoint of pn_bilinear_nhwc_f32 for an UPsampling (ho >= hi, wo >= wi; equal sizes: identity):
 *   din[b][i][:] = (accumulate ? din : 0) + sum_o T[o][i] dout[b][o][:],
 * T the forward's own fp32 tap matrix (the same make_tap per fine row / column; at the clamped
 * last index both taps land on one coarse pixel and both are added).  dout [b][ho][wo][C] at
 * dout + b*dout_bstride, din [b][hi][wi][C] at din + b*din_bstride (floats, multiples of 4);
 * C % 4 == 0.  Gather form: per coarse element an fmaf chain over its fine columns (ascending)
 * inside each fine row, then one fmaf per fine row (ascending). */
int pn_bilinear_nhwc_bwd_f32(const float* dout, float* din, int B, int hi, int wi, int ho, int wo,
                             int C, int accumulate, int64_t dout_bstride, int64_t din_bstride,
                             void* stream);
/* Backward of pn_groupnorm_nhwc_f32 (+ReLU) from its input x on the forward's row blocking, for
 * the H/4 x W/4 map of the same branch (ConvModule norm + act of lateral_convs.0 / output_convs.0):
 * with gate = relu ? (y > 0) : 1, y the saved output [B][HW][256] (dense; not read without relu),
 *   dx [B][HW][256] (dense) = rstd (gamma dy gate - m1 - xhat m2),
 *   dgamma[c] (+)= sum dy gate xhat,  dbeta[c] (+)= sum dy gate   (`accumulate`: add into them).
 * stats: B * G * 4 floats out (mean, rstd, m1, m2); partials: B * nblk * G * 4 doubles and
 * colpart: B * nblk * 512 floats of scratch, nblk = pn_groupnorm_nblk(HW); x / dy images start at
 * multiples of x_bstride / dy_bstride floats.  C == 256, G <= 32, (256 / G) % 4 == 0. */
int pn_groupnorm_act_nhwc_bwd_f32(const float* x, const float* dy, const float* y,
                                  const float* gamma, float* dx, float* dgamma, float* dbeta,
                                  float* stats, double* partials, float* colpart, int B, int64_t HW,
                                  int G, float eps, int relu, int accumulate, int64_t x_bstride,
                                  int64_t dy_bstride, void* stream);

/* ---- The training log on the device (csrc/train_log.hip; pair-net_amd/runner.py TrainLog).
 * Replaces, behind `log_config = dict(interval=50, hooks=[dict(type="TextLoggerHook"), ...])`
 * (configs/_base_/custom_runtime.py, read by tools/train.py:115-241 through mmcv's runner), mmcv's
 * `TextLoggerHook` over `LogBuffer.update` / `LogBuffer.average`: there every term of every
 * iteration is brought to the host (`.item()` in mmdet's `_parse_losses`); here the terms stay on
 * the device until a window of `interval` iterations is complete.  (mmcv's hook and buffer are
 * restated from memory, unpinned.)  Entries added at ABI 34.  Vector stores only, no atomics.
 *
 * One launch per training step: row `row` of the ring [rows][ld] (32-bit words, ld >= T + 3)
 * receives
 *   [0, T)   the step's T scalars: `scalars` is a HOST array of T device pointers to separate
 *            float32 values (the loss terms, then grad_norm); the launch carries them by value,
 *            1 <= T <= 32
 *   [T]      the sum of the scalars i whose bit i of loss_mask is set, 0 + v_a + v_b + ... in
 *            index order, fp32 (mmdet's `loss`: the terms whose name contains "loss")
 *   [T + 1]  status0[0] | status1[0] as int32 (either pointer may be NULL: no such word, 0)
 *   [T + 2]  1.0f where that word is non-zero (the guarded AdamW launch skipped the step), else 0
 * PN_BAD_ARG before the launch: T outside [1, 32], a NULL among the T pointers, NULL `scalars` or
 * `ring`, ld < T + 3, row outside [0, rows). */
int pn_train_log_row_f32(const float* const* scalars, int T, uint32_t loss_mask,
                         const int32_t* status0, const int32_t* status1, float* ring, int rows,
                         int ld, int row, void* stream);
/* One launch per window: from rows [0, n) of that ring, record (T + 4 32-bit words) =
 *   [0, T]   float32 (((v_0 + v_1) + ...) + v_{n-1}) / n of columns 0 .. T, rows in order
 *   [T + 1]  int32 the number of rows whose skipped flag is set
 *   [T + 2]  int32 the OR of the rows' status words        [T + 3]  int32 n
 * PN_BAD_ARG before the launch: NULL ring / record, T outside [1, 32], ld < T + 3, n outside
 * [1, rows]. */
int pn_train_log_window_f32(const float* ring, int rows, int ld, int n, int T, float* record,
                            void* stream);

/* ------------------------------------------------------------------------- *
 * The plain Deformable-DETR detector (configs/deformable_detr/od_r101_vg.py:3-96, `DeformableDETR`
 * with a `DeformableDETRHead`): its loss ([3P] mmdet `DETRHead.loss_single`; the in-tree statement
 * is the commented text at pairnet_bbox_head.py:596-642) and its box results.  csrc/det_loss.hip;
 * composed in det_losses.py / det_head.py.  Entries added at ABI 34 (adding entries is compatible).
 * ------------------------------------------------------------------------- */
/* pn_box_match_cost_f32's cost, cell for cell and in the same operation order, for P problems of
 * their own row counts in ONE launch: the HungarianAssigner of od_r101_vg.py:87-94 (FocalLossCost
 * 2.0, BBoxL1Cost 5.0 xywh, IoUCost giou 2.0) for every decoder layer and for the per-token
 * proposals (pairnet_bbox_head.py:596-642 states the per-layer term).
 *   cls [rows_len][nc] / box [rows_len][4]   the problems' rows, concatenated
 *   tab [P][6] int64 = {offset of the rows x G block in cost, rows (1 .. 65536), G (1 .. 1024),
 *                       offset of the labels in gt_labels, offset of the boxes in gt_bboxes (in
 *                       boxes), offset of the first row in cls / box}
 *   factor [P][4] = (img_w, img_h, img_w, img_h) of the problem's image
 * A label array of zeros gives the proposal term's binarised labels.  max_cells: the largest
 * rows * G of the table (sizes the grid).  The table lives on the device, so this is the CALLER's
 * contract: cells of a block past max_cells are not written, and the entry cannot tell.  A table row outside a buffer or a range leaves its block
 * untouched; a label outside [0, nc) gives a NaN cell.  One cell per lane, no atomics, bitwise
 * reproducible.  PN_BAD_ARG before the launch: a NULL, a non-positive length, max_cells above
 * 65536 * 1024, P outside [1, 65535], nc outside [1, 256]. */
int pn_det_match_cost_f32(const float* cls, const float* box, int64_t rows_len,
                          const int64_t* gt_labels, int64_t labels_len, const float* gt_bboxes,
                          int64_t boxes_len, const float* factor, const int64_t* tab, float* cost,
                          int64_t cost_len, int64_t max_cells, int P, int nc, float w_cls,
                          float w_reg, float w_iou, float alpha, float gamma, float eps,
                          float iou_eps, void* stream);
/* `loss_cls` of every term in one streaming launch (od_r101_vg.py:80-82: FocalLoss, sigmoid,
 * gamma 2, alpha 0.25, weight 2.0; pairnet_bbox_head.py:596-642: summed over rows * C, divided by
 * the term's avg_factor).  x / grad [rows][C] contiguous and 16-byte aligned; labels [rows] int32
 * (C = background), term [rows] int32 in [0, T), avg [T] (the factors, > 0).
 *   element   mmdet `py_sigmoid_focal_loss`: BCE-with-logits (stable form) * alpha_t * pt^gamma
 *   grad      (w_cls / avg[term]) * d element / d x, every element written (0 for a row whose
 *             term is outside [0, T))
 *   out[t]    w_cls * (sum of term t's elements / avg[t])
 * The sums go through partial [pn_det_focal_partials(rows, C, T)] floats (per workgroup and term)
 * and a second fixed-order pass: no float atomics, bitwise reproducible.  The block is read and
 * written 16 bytes at a time whatever C is (an element's row is its flat index / C); the last
 * (rows * C) % 4 elements go one by one.  A label outside [0, C] makes its row's loss and gradient
 * NaN.  PN_BAD_ARG before the launch: a NULL, rows <= 0, C outside [1, 256], T outside [1, 16],
 * rows * C >= 2^31, a short `partial`, x or grad not 16-byte aligned (pn_det_focal_partials
 * returns 0 for such shapes). */
int64_t pn_det_focal_partials(int64_t rows, int C, int T);
int pn_det_focal_f32(const float* x, const int32_t* labels, const int32_t* term, const float* avg,
                     float* grad, float* partial, int64_t partial_len, float* out, int64_t rows,
                     int C, int T, float w_cls, float alpha, float gamma, void* stream);
/* `loss_bbox` (L1Loss 5.0, od_r101_vg.py:83) and `loss_iou` (GIoULoss 2.0, :84) of every term over
 * the M matched pairs (pairnet_bbox_head.py:596-642): pairs [M][4] int32 = {row of the prediction
 * in box / grad, ground-truth box, row of factor, term}, grouped by term with term t owning
 * [term_off[t], term_off[t + 1]).  Targets are cxcywh(gt / factor); GIoU compares cxcywh_to_xyxy(.)
 * * factor of both sides with mmdet's bbox_overlaps(is_aligned, eps = iou_eps) clamps.
 *   out[t][0] = w_bbox * (sum |pred - target| / avg[t]),  out[t][1] = w_iou * (sum (1 - GIoU) / avg[t])
 * One workgroup per term, fixed order, bitwise reproducible.  grad [rows_len][4] must come zeroed:
 * the matched rows receive d(out[t][0] + out[t][1]) / d cxcywh (|d| has derivative 0 at 0; min /
 * max / clamp as autograd, any subgradient at exact ties).  A pair that points outside a buffer
 * makes its term NaN and writes no gradient.  M == 0 is legal.  PN_BAD_ARG before the launch: a
 * NULL (pairs / gt_bboxes may be NULL at M == 0), T outside [1, 16], a non-positive or >= 2^31
 * length, M < 0. */
int pn_det_box_loss_f32(const float* box, int64_t rows_len, const float* gt_bboxes,
                        int64_t boxes_len, const float* factor, int64_t factor_len,
                        const int32_t* pairs, const int32_t* term_off, int64_t M, int T,
                        const float* avg, float* grad, float* out, float w_bbox, float w_iou,
                        float iou_eps, void* stream);
/* Box results behind the ranking ([3P] mmdet `DETRHead._get_bboxes_single` for a sigmoid classifier,
 * test_cfg max_per_img of od_r101_vg.py:95; the head whose loss pairnet_bbox_head.py:596-642
 * states): idx [B][K] flat indices into the image's Q * C logits, best first (pn_topk_strided_f32).
 *   labels[b][k] = idx % C;  det[b][k] = (clamp(cxcywh_to_xyxy(box[b][idx / C]) * (w, h, w, h), 0,
 *   (w, h, w, h)) [/ scale_factor if rescale], sigmoid(cls[b][idx]))
 * meta [B][6] = {img_h, img_w, scale_factor[0..3]}.  mmdet's operation order, no fused multiply-adds;
 * every element of det [B][K][5] and labels [B][K] (int64) is written (an index outside [0, Q * C):
 * NaN row, label -1).  PN_BAD_ARG: a NULL, a non-positive size, C > 256, Q * C > 65536, K > Q * C,
 * B * K >= 2^24, B * Q * C >= 2^31. */
int pn_det_results_f32(const float* cls, const float* box, const int64_t* idx, const float* meta,
                       float* det, int64_t* labels, int B, int Q, int C, int K, int rescale,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PAIRNET_HIP_H_ */
