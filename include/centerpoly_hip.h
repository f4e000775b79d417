/*
 * centerpoly_hip.h -- C ABI of libcenterpoly_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary of the CenterPoly v2 `polydet` hot path.  Every entry
 * point takes raw DEVICE pointers, explicit sizes and a hipStream_t (passed as
 * void*); the library never allocates, frees or keeps a pointer after the call
 * returns, holds no global mutable state, is re-entrant and asynchronous on the
 * supplied stream.  Return value: CP_OK (0) or a negative CP_E* code; no C++
 * exception crosses this boundary.
 *
 * Which reference interface each entry point replaces (paths are relative to
 * the reference tree, /root/reference):
 *
 *   cp_dcn_v2_forward / cp_dcn_v2_backward
 *       the native extension behind `from .DCNv2.dcn_v2 import DCN`
 *       (src/lib/models/networks/pose_dla_dcn.py:16, call site :354;
 *       src/lib/models/networks/resnet_dcn.py:18,221).  Upstream
 *       CharlesShang/DCNv2 (absent from the tree) exposes
 *       dcn_v2_forward(input, weight, bias, offset, mask, kh,kw, sh,sw, ph,pw,
 *       dh,dw, dg) and dcn_v2_backward(..., grad_output) -> (grad_input,
 *       grad_offset, grad_mask, grad_weight, grad_bias).
 *   cp_depthwise_up_forward
 *       IDAUp's depth-wise ConvTranspose2d `up` + skip add,
 *       src/lib/models/networks/pose_dla_dcn.py:372-375, 381-387.
 *   cp_polydet_decode
 *       _nms + _topk + polydet_decode, src/lib/models/decode.py:13-19, 117-133,
 *       512-670, and the gather helpers src/lib/models/utils.py:12-26.
 *   cp_sigmoid_focal_forward / cp_sigmoid_focal_backward
 *       _sigmoid (src/lib/models/utils.py:8-10) + _neg_loss / FocalLoss
 *       (src/lib/models/losses.py:146-171, 792-799) as used at
 *       src/lib/trains/polydet.py:46,84.
 *   cp_gather_l1_forward / cp_gather_l1_backward
 *       _transpose_and_gather_feat + RegL1Loss (src/lib/models/losses.py:817-830)
 *       and the regression part of PolyLoss (src/lib/models/losses.py:910-949).
 *   cp_poly_iou_order_forward / cp_poly_iou_order_backward
 *       the per-object loop of PolyLoss (src/lib/models/losses.py:868-909) with
 *       WeilPolygonClipper (:373-628) and area (:25-41).
 *
 * All tensors are dense fp32 NCHW unless stated.  "B" is the per-device batch.
 */
#ifndef CENTERPOLY_HIP_H
#define CENTERPOLY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CP_ABI_VERSION 3   /* 3 (round 4): + cp_polydet_decode_ex, cp_dense_l1_*, cp_polydet_dense_targets, cp_conv_direct_forward_ex,
                              cp_conv_mfma_forward_split, cp_activation_split / _unsplit, cp_dla_base_pair_*; no signature changed.
                              Added since, backward compatible (no version change): cp_polydet_targets_ex,
                              cp_class_instance_masks, cp_class_writer_instances, cp_render_overlay_workspace_bytes,
                              cp_render_overlay, cp_render_heatmap, cp_soft_nms_device, cp_merge_detections(_workspace_bytes),
                              cp_dcn_v2_forward_slices(_count), cp_dcn_splitk_reduce, cp_depthwise_up_forward_slices,
                              cp_conv1x1_stream_*, cp_conv3x3_stream_*, cp_instance_map(_workspace_bytes),
                              cp_pixel_confusion(_workspace_bytes), cp_panoptic_pairs(_workspace_bytes), cp_panoptic_match,
                              cp_boundary_overlaps(_workspace_bytes), cp_polygon_overlaps(_workspace_bytes),
                              cp_merge_detections_mask(_workspace_bytes), cp_map_pairs, cp_track_associate, cp_track_update,
                              cp_rle_encode(_workspace_bytes), cp_rle_decode(_workspace_bytes), cp_map_pairs_shifted,
                              cp_track_predict, cp_track_kinematics(_workspace_bytes), cp_png_deflate(_workspace_bytes) */

enum {
  CP_OK = 0,
  CP_EINVAL = -1,       /* null pointer, non-positive size, inconsistent arguments */
  CP_EUNSUPPORTED = -2, /* valid but not implemented shape/option */
  CP_EWORKSPACE = -3,   /* workspace smaller than cp_*_workspace_bytes() */
  CP_EHIP = -4          /* a HIP runtime call or kernel launch failed */
};

/* ------------------------------------------------------------ memory contract --
 * For every entry point, unless its own comment says otherwise (tests/test_memory_contract.py holds each of them to it):
 *   * A `workspace` is scratch.  Its contents on entry are ARBITRARY -- stale data of an earlier call, of another
 *     entry or of nothing at all -- and whatever a call needs zeroed in it the call zeroes itself.  Its contents
 *     after the call mean nothing to the caller.  The exceptions are named where they occur: the CP_DCN_*_PREPARED
 *     modes and `prepared` of cp_dcn_v2_forward_fused read the weights an earlier call left at its head,
 *     cp_dcn_v2_forward_slices leaves its partial sums in it for the caller, and cp_poly_iou_order_backward reads the
 *     object count its forward left.
 *   * A workspace of exactly cp_*_workspace_bytes(...) bytes is enough: no byte before it or from that length on is
 *     read or written, whatever rounding an allocator would have added.
 *   * An output is OVERWRITTEN, every element of the extent its comment gives and from any previous contents, so it
 *     may be handed over uninitialised.  The outputs that are ADDED to instead say so: grad_weight / grad_bias of
 *     the DCN and convolution backward entries, cp_channel_sum_accumulate, grad_feat of cp_gather_l1_backward and
 *     cp_poly_iou_order_backward, conf and bad of cp_pixel_confusion, stat / iou / bad of cp_panoptic_match; and
 *     pred_add_out of cp_poly_iou_order_forward is written in part only (the caller zero-fills it).
 *   * Where a call reports a count or a capacity (counts[0] rows of the mask merge, n_out instances, cap_counts /
 *     cap_bytes of cp_rle_encode, cap_bytes of cp_png_deflate, segments of cp_soft_nms_device), nothing is written
 *     at or beyond the capacity, and elements between a reported count and the capacity hold what the entry's
 *     comment says (dead slots) or are not specified; nothing outside the output's stated extent is ever touched.
 *   * Inputs are never written (in-place forms, such as cp_sigmoid_focal_forward's heat map, are named as such). */

/* representation of the polygon head (src/lib/opts.py `--rep`) */
enum { CP_REP_CARTESIAN = 0, CP_REP_POLAR = 1, CP_REP_POLAR_FIXED = 2 };

/* contraction arithmetic of cp_dcn_v2_forward */
enum {
  CP_DCN_F32 = 0,    /* fp32 MFMA, exact fp32 fma chain                                        */
  CP_DCN_BF16X3 = 1, /* split-bf16: a*b ~ ah*bh + ah*bl + al*bh on bf16 MFMA, fp32 accumulate;
                        ~2^-16 relative error.  The weights are split and permuted into the
                        head of `workspace` by a prologue launch of the call                  */
  CP_DCN_BF16X3_PREPARED = 2, /* the same, and `workspace` still holds the permuted weights of an
                        earlier CP_DCN_BF16X3 call with the same weight tensor and shape
                        (inference: one workspace per layer, prologue paid once)              */
  CP_DCN_BF16X3_REGION = 3, /* CP_DCN_BF16X3 on the LDS-region kernel whatever the map size (the
                        library otherwise picks it only where its tiles fill the chip);
                        CP_EUNSUPPORTED unless 3x3, stride 1, pad 1, dilation 1, Cin % 16 == 0 */
  CP_DCN_BF16X3_REGION_PREPARED = 4 /* ... with the weights already in `workspace`            */
};

/* regression flavour for cp_gather_l1_* */
enum {
  CP_L1_PLAIN = 0,       /* RegL1Loss / PolyLoss cartesian: sum |p*m - t*m|            */
  CP_L1_POLAR = 1,       /* PolyLoss polar: L1 on even slots + sum(1-cos) on odd slots */
  CP_L1_POLAR_FIXED = 2, /* PolyLoss polar_fixed: L1 on even (radius) slots only       */
  CP_L1_RELU20 = 3,      /* PolyLoss 'relu': |p-t| kept only where >= 20               */
  CP_L1_SMOOTH = 4       /* RegLoss (--reg_loss sl1): smooth_l1, divided by sum(mask) + eps (not x D) */
};

int cp_abi_version(void);
const char* cp_strerror(int code);
/* Name of the HIP device architecture the library was built for ("gfx950"). */
const char* cp_build_arch(void);

/* ------------------------------------------------------------------ DCNv2 --
 * Modulated deformable convolution, kernel kh x kw, one deformable group.
 *   x        [B, Cin, H, W]
 *   offset   per-tap (dy, dx) interleaved: channel 2k = dy_k, 2k+1 = dx_k,
 *            k = ky*kw + kx; element (b, ch, ho, wo) at
 *            offset[b*offset_bstride + ch*Ho*Wo + ho*Wo + wo]
 *   mask     [.., kh*kw, Ho, Wo], batch stride mask_bstride; if mask_is_logit != 0
 *            the kernel applies sigmoid itself (lets the caller pass the raw
 *            27-channel conv_offset_mask output: offset = om, mask = om + 18*Ho*Wo,
 *            both batch strides 27*Ho*Wo, without chunk/cat/sigmoid passes)
 *   weight   [Cout, Cin, kh, kw], bias [Cout] or NULL
 *   out      [B, Cout, Ho, Wo]
 * Optional fused epilogue (inference): out = act(acc * ep_scale[co] + ep_shift[co])
 * with ep_scale/ep_shift NULL meaning scale 1 / shift = bias; relu != 0 clamps at 0.
 * When ep_scale/ep_shift are given, bias must already be folded into ep_shift.
 * Small-spatial layers split K over workgroups; their partial sums live in the
 * caller's workspace (cp_dcn_v2_forward_workspace_bytes), behind the permuted weights of the
 * split-bf16 contraction; with CP_DCN_F32 and no K split the workspace may be NULL.
 */
typedef struct cp_dcn_shape {
  int32_t B, Cin, H, W, Cout;
  int32_t kh, kw, stride, pad, dil;
  int32_t deformable_groups; /* only 1 is implemented */
} cp_dcn_shape;

size_t cp_dcn_v2_forward_workspace_bytes(const cp_dcn_shape* s);
/* Which kernel cp_dcn_v2_forward runs for this shape and contraction: 0 = gather kernel, exact fp32 MFMA;
 * 1 = gather kernel, split-bf16; 2 = LDS-region kernel, split-bf16 (dcn_fwd_region.hip: the maps whose 8 x 32 pixel
 * tiles fill the chip).  Lets a caller choose between CP_DCN_F32 and CP_DCN_BF16X3 per layer; negative = CP_E*. */
int cp_dcn_v2_forward_kernel(const cp_dcn_shape* s, int32_t contraction);
int cp_dcn_v2_forward(const cp_dcn_shape* s, const float* x, const float* offset,
                      int64_t offset_bstride, const float* mask, int64_t mask_bstride,
                      int32_t mask_is_logit, const float* weight, const float* bias,
                      const float* ep_scale, const float* ep_shift, int32_t relu,
                      int32_t contraction, float* out, void* workspace, size_t workspace_bytes,
                      void* stream);

/* The K-split launch of cp_dcn_v2_forward WITHOUT its reduce, for a consumer that adds the slices up while it reads them
 * (cp_depthwise_up_forward_slices): no reduce launch, no map written and read back.
 *   cp_dcn_v2_forward_slices_count: the slice count (> 1) where cp_dcn_v2_forward would run the LDS-region kernel with
 *       its input channels split for this shape and contraction; 0 everywhere else.
 *   cp_dcn_v2_forward_slices: cp_dcn_v2_forward's arguments without bias, epilogue and `out`.  Leaves the slices' RAW
 *       sums (no bias, no epilogue) as partial[slice][B][Cout][H][W] in `workspace` (cp_dcn_v2_forward_workspace_bytes),
 *       *partial_offset bytes from its start; they are valid until the next call that uses the workspace.
 *       CP_EUNSUPPORTED where the count is 0.
 *   cp_dcn_splitk_reduce: the reduce on its own, out[b][c][i] = act((sum_s partial[s][b][c][i]) * ep_scale[c] +
 *       ep_shift[c]), slices added in order, NULL = scale 1 / shift 0 -- what cp_dcn_v2_forward launches after the
 *       slices (with shift = bias where no epilogue is given). */
int cp_dcn_v2_forward_slices_count(const cp_dcn_shape* s, int32_t contraction);
int cp_dcn_v2_forward_slices(const cp_dcn_shape* s, const float* x, const float* offset, int64_t offset_bstride,
                             const float* mask, int64_t mask_bstride, int32_t mask_is_logit, const float* weight,
                             int32_t contraction, void* workspace, size_t workspace_bytes, size_t* partial_offset,
                             void* stream);
int cp_dcn_splitk_reduce(const float* partial, int32_t nslices, const float* ep_scale, const float* ep_shift,
                         int32_t relu, float* out, int32_t B, int32_t C, int64_t HW, void* stream);

/* The DCN module of the reference in ONE launch: `DCN.forward` (upstream DCNv2/dcn_v2.py: out = conv_offset_mask(x);
 * o1, o2, mask = chunk(out, 3); offset = cat(o1, o2); mask = sigmoid(mask); dcn_v2_conv(x, offset, mask, ...)), i.e.
 * cp_dcn_v2_forward with the 27-channel 3x3 / pad 1 convolution that produces its offsets and mask logits computed
 * inside the kernel for each tile (split-bf16 x3 like cp_conv3x3_mfma_forward) instead of by a launch of its own.
 *   om_weight [27][Cin][3][3], om_bias [27]: conv_offset_mask's parameters
 *   om_out    NULL, or [B][27][H][W]: receives the convolution's output (what cp_dcn_v2_backward needs as
 *             offset = om_out, mask = om_out + 18 H W, both batch strides 27 H W, mask_is_logit = 1)
 *   prepared  != 0: `workspace` still holds the permuted weights of an earlier call with the same two weight tensors
 * Only where the LDS-region kernel runs (cp_dcn_v2_forward_fused_supported: 3x3, stride 1, pad 1, dilation 1,
 * Cin % 16 == 0, enough tiles to fill the chip); CP_EUNSUPPORTED otherwise -- run the convolution and
 * cp_dcn_v2_forward then. */
int cp_dcn_v2_forward_fused_supported(const cp_dcn_shape* s);
size_t cp_dcn_v2_forward_fused_workspace_bytes(const cp_dcn_shape* s);
int cp_dcn_v2_forward_fused(const cp_dcn_shape* s, const float* x, const float* om_weight, const float* om_bias,
                            const float* weight, const float* bias, const float* ep_scale, const float* ep_shift,
                            int32_t relu, int32_t prepared, float* om_out, float* out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Backward.  grad_* outputs may be NULL to skip that gradient.  grad_x, grad_offset and grad_mask are
 * OVERWRITTEN (the library zero-fills grad_x itself before its kernels accumulate into it: uninitialised memory is
 * fine, a caller that sums two branches adds them itself); grad_weight and grad_bias are ACCUMULATED INTO (caller
 * zero-fills).  mask is the post-sigmoid mask (mask_is_logit == 0) or the logits (then grad_mask is w.r.t. the
 * logits).  flags: 0 = the default kernels (split-bf16 x3 contraction, fp32 accumulate), or a bit-or of CP_DCN_BWD_*. */
enum {
  CP_DCN_BWD_EXACT_F32 = 1,     /* contract on the exact-fp32 MFMA chain instead of split-bf16 x3                 */
  CP_DCN_BWD_NARROW_TILES = 2   /* data gradients: 8-row tiles on every layer (A/B timing of the 12-row form)    */
};
size_t cp_dcn_v2_backward_workspace_bytes(const cp_dcn_shape* s);
int cp_dcn_v2_backward(const cp_dcn_shape* s, const float* x, const float* offset,
                       int64_t offset_bstride, const float* mask, int64_t mask_bstride,
                       int32_t mask_is_logit, const float* weight, const float* grad_out,
                       float* grad_x, float* grad_offset, int64_t grad_offset_bstride,
                       float* grad_mask, int64_t grad_mask_bstride, float* grad_weight,
                       float* grad_bias, int32_t flags, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------- depth-wise up-sampling --
 * IDAUp's `up` (depth-wise ConvTranspose2d, kernel 2f, stride f, padding f/2,
 * groups = C, no bias; src/lib/models/networks/pose_dla_dcn.py:372-375) fused with
 * the `+ layers[i-1]` that follows it (:381-387).
 *   x [B,C,H,W], weight [C,1,2f,2f], skip [B,C,H*f,W*f] or NULL -> out [B,C,H*f,W*f]
 * f in {2,4,8} forward; backward for f in {2,4}: grad_x is overwritten, grad_weight is
 * ACCUMULATED INTO (caller zero-fills); grad_skip = grad_out is the caller's business. */
int cp_depthwise_up_forward(const float* x, const float* weight, const float* skip, float* out,
                            int32_t B, int32_t C, int32_t H, int32_t W, int32_t f, void* stream);
/* The same on an input that is still K-split slices (cp_dcn_v2_forward_slices):
 *   out = up(act((sum_s partial[s]) * ep_scale[c] + ep_shift[c])) + skip,   partial[s] = partial + s * slice_stride
 * (elements), each [B,C,H,W]; NULL scale / shift = 1 / 0.  Bit-identical to cp_dcn_splitk_reduce followed by
 * cp_depthwise_up_forward.  f = 2 with W even, or f = 4; CP_EUNSUPPORTED otherwise (run those two). */
int cp_depthwise_up_forward_slices(const float* partial, int32_t nslices, int64_t slice_stride, const float* ep_scale,
                                   const float* ep_shift, int32_t relu, const float* weight, const float* skip,
                                   float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t f, void* stream);
int cp_depthwise_up_backward(const float* x, const float* weight, const float* grad_out,
                             float* grad_x, float* grad_weight, int32_t B, int32_t C, int32_t H,
                             int32_t W, int32_t f, void* stream);

/* 2x2 / stride 2 max pooling (floor mode) of the DLA trees' `downsample` (src/lib/models/networks/pose_dla_dcn.py:
 * 186-187,203-204), torch's tie rule (first maximum in row-major order, NaN propagates).  The backward recomputes the
 * arg-max from x and OVERWRITES grad_in (every element, also a trailing odd row / column). */
int cp_maxpool2x2_forward(const float* x, float* out, int32_t B, int32_t C, int32_t H, int32_t W, void* stream);
int cp_maxpool2x2_backward(const float* x, const float* grad_out, float* grad_in, int32_t B, int32_t C, int32_t H,
                           int32_t W, void* stream);

/* out = a + nearest-neighbour x2 up-sampling of low: `up1 + nn.Upsample(scale_factor=2)(low3)` of the Hourglass'
 * kp_module (src/lib/models/networks/large_hourglass.py:334-342) in one pass.
 * a, out [B][C][2H][2W]; low [B][C][H][W]; out may alias a. */
int cp_upsample2x_add(const float* a, const float* low, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                      void* stream);

/* y <- act(y + bias[c] + residual) in place (fp32 NCHW, HW = H*W): the epilogue of a library
 * convolution whose BatchNorm was folded (inference).  bias / residual may be NULL. */
int cp_bias_act_inplace(float* y, const float* bias, const float* residual, int32_t B, int32_t C,
                        int64_t HW, int32_t relu, void* stream);
/* backward of y = relu(conv + bias[c]) (cp_bias_act_inplace with relu, no residual; the heads'
 * Conv2d(3x3, bias) -> ReLU in training, src/lib/models/networks/pose_dla_dcn.py:448-451):
 * grad_in = grad_out * [y > 0] (grad_in == grad_out allowed), grad_bias[c] is ACCUMULATED INTO
 * (caller zero-fills).  HW % 4 == 0, 16-byte aligned tensors. */
int cp_bias_relu_backward(const float* y, const float* grad_out, float* grad_in, float* grad_bias,
                          int32_t B, int32_t C, int64_t HW, void* stream);
/* out[c] += sum over images and pixels of x[b][c][p] (fp32 NCHW): the bias gradient of a library
 * convolution (conv_offset_mask of DCN, src/lib/models/networks/pose_dla_dcn.py:354 via DCNv2). */
int cp_channel_sum_accumulate(const float* x, float* out, int32_t B, int32_t C, int64_t HW, void* stream);

/* Direct convolution + bias (+ ReLU) of the full-resolution, low-channel layers of the DLA base at
 * inference (src/lib/models/networks/pose_dla_dcn.py:236-246,266-276: `base_layer` 7x7 3->16,
 * `level0` 3x3 16->16, `level1` 3x3 s2 16->32; Conv2d(bias=False) -> BatchNorm2d -> ReLU with the
 * BatchNorm folded by the caller: scale into `w`, shift into `bias`):
 *   out[b][co][y][x] = act(bias[co] + sum w[co][ci][ky][kx] * x[b][ci][y*stride - pad + ky][x*stride - pad + kx])
 * x [B][Cin][H][W], w [Cout][Cin][k][k], bias [Cout] or NULL, out [B][Cout][Ho][Wo], zero padding.
 * Implemented shapes: (k 7, Cin 3, Cout 16, stride 1, pad 3) and (k 3, Cin 16, Cout 16|32, stride 1|2,
 * pad 1); cp_conv_direct_supported tells, anything else returns CP_EUNSUPPORTED. */
int cp_conv_direct_supported(int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t pad);
int cp_conv_direct_forward(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t Cin,
                           int32_t H, int32_t W, int32_t Cout, int32_t k, int32_t stride, int32_t pad,
                           int32_t relu, void* stream);
/* ABI v3: the same call with the arithmetic as an argument -- split_bf16 != 0 runs the stride-1 3x3 / 16-input-channel
 * layers (level0 of the DLA base) as split-bf16 x3 on the bf16 matrix cores (fp32 in and out, ~2^-16 per product; the
 * stride-2 layers keep the exact kernel, which measured faster); 0 = cp_conv_direct_forward (exact fp32 fma chains). */
int cp_conv_direct_forward_ex(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t Cin,
                           int32_t H, int32_t W, int32_t Cout, int32_t k, int32_t stride, int32_t pad,
                           int32_t relu, int32_t split_bf16, void* stream);

/* 3x3 / stride 1 / pad 1 convolution of float32 NCHW maps on the bf16 matrix cores (split-bf16 x3: float32 in and
 * out, ~2^-16 relative error per product): the dense convolutions of BasicBlock (src/lib/models/networks/
 * pose_dla_dcn.py:38-66), of the heads' `fc` (:445-462), of DCN.conv_offset_mask (DCNv2/dcn_v2.py:137-145) and of
 * large_hourglass.py's convolution / residual (:24-37, :55-81) -- what the reference hands to cuDNN.
 *   out[b][co][y][x] = act(bias[co] + residual[b][co][y][x] + sum w[co][ci][ky][kx] * x[b][ci][y - 1 + ky][x - 1 + kx])
 * The weights are split and permuted once by cp_conv3x3_mfma_prepare into `wperm` (cp_conv3x3_mfma_weight_bytes);
 * with transposed = 1 the prologue reads a [Cin][Cout][3][3] tensor as its transposed, flipped self, so that the
 * same kernel computes the INPUT GRADIENT of the convolution whose weight that tensor is (x := grad_out).
 * The contraction runs in steps of 32 input channels (a ragged last step is zero-filled); tensors must stay within
 * 32-bit byte offsets per image: cp_conv3x3_mfma_supported tells, anything else returns CP_EUNSUPPORTED.
 * bias, residual may be NULL. */
int cp_conv3x3_mfma_supported(int32_t Cin, int32_t Cout, int32_t H, int32_t W);
size_t cp_conv3x3_mfma_weight_bytes(int32_t Cin, int32_t Cout);
int cp_conv3x3_mfma_prepare(const float* weight, int32_t Cin, int32_t Cout, int32_t transposed, void* wperm,
                            void* stream);
int cp_conv3x3_mfma_forward(const float* x, const void* wperm, const float* bias, const float* residual, float* out,
                            int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t relu, void* stream);

/* General form of the above: taps = 9 (3x3 / pad 1) or 1 (1x1), and the input given as the channel concatenation of
 * nsrc (1..4) tensors xs[i] = [B][cs[i]][H][W] read in place -- the torch.cat of `Root.forward`
 * (src/lib/models/networks/pose_dla_dcn.py:148-166) is never materialised.  With nsrc > 1 every cs[i] must be a
 * multiple of 32.  Weights prepared by cp_conv_mfma_prepare with the same taps over Cin = sum cs[i]. */
size_t cp_conv_mfma_weight_bytes(int32_t Cin, int32_t Cout, int32_t taps);
int cp_conv_mfma_prepare(const float* weight, int32_t Cin, int32_t Cout, int32_t taps, int32_t transposed, void* wperm,
                         void* stream);
/* The same for a whole table of weights in ONE launch (a training step uses ~110 forms -- every convolution's forward and
 * transposed one -- each a 4-microsecond launch of its own when prepared per use): `jobs` lives in DEVICE memory, job i's
 * workgroups are first_block .. first_block + cp_conv_mfma_prepare_blocks(Cin, Cout, taps) - 1 (first_block ascending,
 * job 0 at 0), total_blocks their sum.  Cin / Cout / transposed as for cp_conv_mfma_prepare. */
typedef struct cp_conv_prepare_job {
  const float* weight;
  void* wperm;
  int32_t Cin, Cout, taps, transposed, first_block, reserved;
} cp_conv_prepare_job;
int32_t cp_conv_mfma_prepare_blocks(int32_t Cin, int32_t Cout, int32_t taps);
int cp_conv_mfma_prepare_batch(const cp_conv_prepare_job* jobs_device, int32_t njobs, int32_t total_blocks, void* stream);
int cp_conv_mfma_forward(const float* const* xs, const int32_t* cs, int32_t nsrc, const void* wperm, const float* bias,
                         const float* residual, float* out, int32_t B, int32_t H, int32_t W, int32_t Cout,
                         int32_t taps, int32_t relu, void* stream);
/* the same with a stride of 1 or 2 (3x3: the first convolution of DLA levels 2-5, pose_dla_dcn.py:38-46, and of the
 * Hourglass' down-sampling residuals; 1x1: their skip convolutions, large_hourglass.py:55-81);
 * out is [B][Cout][(H - 1) / stride + 1][(W - 1) / stride + 1] */
int cp_conv_mfma_forward_strided(const float* const* xs, const int32_t* cs, int32_t nsrc, const void* wperm,
                                 const float* bias, const float* residual, float* out, int32_t B, int32_t H, int32_t W,
                                 int32_t Cout, int32_t taps, int32_t stride, int32_t relu, void* stream);
/* level0 + level1 of the DLA base at inference as ONE launch (pose_dla_dcn.py:236-246,266-276, BatchNorm folded):
 *   out = relu(conv3x3 stride 2 pad 1 (relu(conv3x3 pad 1 (x, w0) + b0), w1) + b1)
 * x [B][16][H][W] -> out [B][32][(H-1)/2+1][(W-1)/2+1]; w0 [16][16][3][3], w1 [32][16][3][3], b0 / b1 may be null.
 * The 16-channel full-resolution intermediate (the network's largest activation, one consumer) stays in LDS.
 * split-bf16 x3 arithmetic in both layers.  W % 4 == 0 and a 16-byte aligned x (cp_dla_base_pair_supported), else
 * CP_EUNSUPPORTED -- run the two layers through cp_conv_direct_forward_ex. */
int cp_dla_base_pair_supported(int32_t H, int32_t W);
int cp_dla_base_pair_forward(const float* x, const float* w0, const float* b0, const float* w1, const float* b1, float* out,
                             int32_t B, int32_t H, int32_t W, void* stream);
/* base_layer + level0 + level1 of the DLA base at inference as ONE launch (added without an ABI version change):
 *   out = relu(conv3x3 stride 2 pad 1 (relu(conv3x3 pad 1 (relu(conv7x7 pad 3 (image) + stem_bias), w0) + b0), w1) + b1)
 * image [B][3][H][W] -> out [B][32][(H-1)/2+1][(W-1)/2+1]; stem_wperm is what cp_conv7x7_c3_prepare writes for
 * Cout = 16; w0, b0, w1, b1 as cp_dla_base_pair_forward; the three biases may be null.  Both 16-channel full-resolution
 * maps stay in LDS.  The result has the bits of cp_conv7x7_c3_forward (stride 1, ReLU) followed by
 * cp_dla_base_pair_forward.  W % 4 == 0 and a 16-byte aligned image (cp_dla_base_trio_supported), else
 * CP_EUNSUPPORTED -- run those two. */
int cp_dla_base_trio_supported(int32_t H, int32_t W);
int cp_dla_base_trio_forward(const float* image, const void* stem_wperm, const float* stem_bias, const float* w0,
                             const float* b0, const float* w1, const float* b1, float* out, int32_t B, int32_t H,
                             int32_t W, void* stream);
/* SPLIT activations (round 4; inference, between the two convolutions of a BasicBlock, pose_dla_dcn.py:38-66): a
 * float32 tensor [B][C][H][W] kept as two planes [hi | lo] of [B][C / 8][H][W][8 x bf16] (hi = bf16(v), lo =
 * bf16(v - hi): the halves the convolution's staging forms anyway; same bytes as float32; C % 8 == 0).  The producer's
 * epilogue writes them (out_split), the consumer stages them with two 16-byte loads per unit and no conversion
 * arithmetic (x_split: 3x3 / stride 1, Cin % 32 == 0).  Results are bit-identical to the float32 route.
 * cp_conv_mfma_forward_split = cp_conv_mfma_forward_strided for one source; x / out are float32 tensors or split
 * planes as the flags say (out_split: no residual).  cp_activation_split / _unsplit convert (tests, probes). */
int cp_conv_mfma_forward_split(const void* x, int32_t x_split, const void* wperm, const float* bias, const float* residual,
                               void* out, int32_t out_split, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout,
                               int32_t taps, int32_t stride, int32_t relu, void* stream);
int cp_activation_split(const float* x, void* out, int32_t B, int32_t C, int32_t H, int32_t W, void* stream);
int cp_activation_unsplit(const void* in, float* x, int32_t B, int32_t C, int32_t H, int32_t W, void* stream);
/* The 1x1 / stride 1 forward convolution of cp_conv_mfma_forward (taps = 1) streamed through registers -- no LDS staging,
 * the loads of two 32-channel chunks in flight per wave (csrc/conv_stream.hip): `Root` and `Tree.project` at inference
 * (pose_dla_dcn.py:148-166, 206-213).  Every output element is the same sequence of floating-point operations as in
 * cp_conv_mfma_forward: the two give the SAME BITS (same MFMA, chunk order, K split, epilogue order).
 * Every cs[i] is a multiple of 16; byte offsets within an image are 32-bit: cp_conv1x1_stream_supported tells, anything
 * else returns CP_EUNSUPPORTED.  wperm: cp_conv_mfma_prepare's form with taps = 1 (cp_conv1x1_stream_weight_bytes /
 * _prepare forward to it: one prepared buffer serves both kernels).
 * The tile form: nb pixel groups of 32 per wave (1 | 2; a function of (Cout, H * W)) and ks wave groups over
 * interleaved chunks (1 | 2 | 4; the K split cp_conv_mfma_forward picks for (Cin, Cout, H, W, B), which is what its bits
 * depend on).  cp_conv1x1_stream_form returns nb << 8 | ks; cp_conv1x1_stream_forward_form runs a given form (0, 0: that
 * one; tests and probes force the others, whose K splits sum in another order). */
int cp_conv1x1_stream_supported(const int32_t* cs, int32_t nsrc, int32_t Cout, int32_t H, int32_t W);
size_t cp_conv1x1_stream_weight_bytes(int32_t Cin, int32_t Cout);
int cp_conv1x1_stream_prepare(const float* weight, int32_t Cin, int32_t Cout, void* wperm, void* stream);
int cp_conv1x1_stream_forward(const float* const* xs, const int32_t* cs, int32_t nsrc, const void* wperm, const float* bias,
                              const float* residual, float* out, int32_t B, int32_t H, int32_t W, int32_t Cout,
                              int32_t relu, void* stream);
int cp_conv1x1_stream_form(int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t B);
int cp_conv1x1_stream_forward_form(const float* const* xs, const int32_t* cs, int32_t nsrc, const void* wperm,
                                   const float* bias, const float* residual, float* out, int32_t B, int32_t H, int32_t W,
                                   int32_t Cout, int32_t relu, int32_t nb, int32_t ks, void* stream);
/* The 3x3 / stride 1 / pad 1 forward convolution of cp_conv_mfma_forward (taps = 9) for ONE source and Cout <= 32, + bias,
 * streamed through registers -- no LDS staging, no barrier in the K loop, the loads of several taps in flight per wave
 * (csrc/conv3x3_stream.hip): DCN.conv_offset_mask at inference (DCNv2/dcn_v2.py:137-145).  Every output element is the
 * same sequence of floating-point operations as in cp_conv_mfma_forward: the two give the SAME BITS (same MFMA, chunk and
 * tap order, K split, halo multiplied as zeros, epilogue).
 * Byte offsets within an image are 32-bit: cp_conv3x3_stream_supported tells.  Cout > 32, an unsupported shape, a
 * residual or relu != 0 return CP_EUNSUPPORTED and launch nothing (the caller keeps cp_conv_mfma_forward).
 * wperm: cp_conv_mfma_prepare's form with taps = 9 (one prepared buffer serves both kernels).
 * The tile form: nt tiles of 16 pixels per wave (1 | 2 | 4; a function of (H, W); 4 on a width that is a multiple of 4
 * is the row form: 64 consecutive pixels per wave, 16-byte loads, the taps of a row from one split) and ks wave groups over
 * interleaved chunks (1 | 2 | 4; the K split cp_conv_mfma_forward picks for (Cin, Cout, H, W, B), which is what its bits
 * depend on).  cp_conv3x3_stream_form returns nt << 8 | ks; cp_conv3x3_stream_forward_form runs a given form (0, 0: that
 * one; tests and probes force the others, whose K splits sum in another order). */
int cp_conv3x3_stream_supported(int32_t Cin, int32_t Cout, int32_t H, int32_t W);
int cp_conv3x3_stream_form(int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t B);
int cp_conv3x3_stream_forward(const float* x, const void* wperm, const float* bias, const float* residual, float* out,
                              int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t relu, void* stream);
int cp_conv3x3_stream_forward_form(const float* x, const void* wperm, const float* bias, const float* residual, float* out,
                                   int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t relu, int32_t nt,
                                   int32_t ks, void* stream);
/* Weight gradient of a 3x3 / stride 2 / pad 1 convolution (the first convolution of DLA levels 2-5,
 * src/lib/models/networks/pose_dla_dcn.py:32-40; cuDNN's backward-filter in the reference), same arithmetic:
 *   gw[co][ci][ky][kx] += sum_{b,i,j} grad_out[b][co][i][j] * x[b][ci][2 i + ky - 1][2 j + kx - 1]
 * x [B][Cin][H][W], grad_out [B][Cout][(H - 1) / 2 + 1][W / 2]; gw [Cout][Cin][3][3] is ACCUMULATED into (float atomics:
 * zero it first).  Needs W % 8 == 0; cp_conv3x3_s2_wgrad_supported tells, else CP_EUNSUPPORTED. */
int cp_conv3x3_s2_wgrad_supported(int32_t Cin, int32_t Cout, int32_t H, int32_t W);
int cp_conv3x3_s2_wgrad(const float* x, const float* grad_out, float* gw, int32_t B, int32_t Cin, int32_t H, int32_t W,
                        int32_t Cout, void* stream);

/* 7x7 / pad 3 convolution of a 3-channel image (+ bias, + ReLU), stride 1 or 2, on the bf16 matrix cores (split-bf16 x3,
 * the arithmetic above): the Hourglass stem `pre = convolution(7, 3, 128, stride=2)`
 * (src/lib/models/networks/large_hourglass.py:287-290) and DLA's `base_layer` Conv2d(3, 16, 7, stride=1)
 * (src/lib/models/networks/pose_dla_dcn.py:236-241); cuDNN in the reference, BatchNorm folded by the caller:
 *   out[b][co][y][x] = act(bias[co] + sum w[co][ci][ky][kx] * x[b][ci][S y - 3 + ky][S x - 3 + kx])
 * x [B][3][H][W], weight [Cout][3][7][7] (prepared once into wperm), out [B][Cout][(H - 1) / S + 1][(W - 1) / S + 1]. */
int cp_conv7x7_c3_supported(int32_t Cout, int32_t H, int32_t W, int32_t stride);
size_t cp_conv7x7_c3_weight_bytes(int32_t Cout);
int cp_conv7x7_c3_prepare(const float* weight, int32_t Cout, void* wperm, void* stream);
int cp_conv7x7_c3_forward(const float* x, const void* wperm, const float* bias, float* out, int32_t B, int32_t H,
                          int32_t W, int32_t Cout, int32_t stride, int32_t relu, void* stream);

/* Input gradient of a stride-1 convolution (3x3 / pad 1 or 1x1) whose INPUT was the output y of a bias + ReLU epilogue
 * (the heads' Conv2d(3x3, bias) -> ReLU -> Conv2d(1x1), src/lib/models/networks/pose_dla_dcn.py:445-462), with that
 * ReLU's backward and its bias gradient in the kernel's epilogue (threshold_backward + the bias sum in the reference):
 *   grad_y[b][c][p] = [y[b][c][p] > 0] * sum_{co, tap} weight[co][c][tap'] * grad_out[b][co][p + tap]
 *   grad_bias[c]   += sum_{b, p} grad_y[b][c][p]     (NULL: not wanted; accumulated into: zero it first.  Every wave
 *                     leaves its channel sums in the workspace, a second small kernel adds them up)
 *   wperm_t  cp_conv_mfma_prepare(weight [Cout][Cin][k][k], Cin := Cout, Cout := Cin, taps, transposed = 1)
 *   grad_out [B][Cout][H][W], y and grad_y [B][Cin][H][W].  Cout below 32 multiplies zeros up to 32 (the launch is
 *   bound by the two [B][Cin][H][W] streams). */
size_t cp_conv_mfma_input_grad_relu_workspace_bytes(int32_t B, int32_t Cin, int32_t H, int32_t W);
int cp_conv_mfma_input_grad_relu(const float* grad_out, const void* wperm_t, const float* y, float* grad_y,
                                 float* grad_bias, int32_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout,
                                 int32_t taps, void* workspace, size_t workspace_bytes, void* stream);
/* Input gradient of a 3x3 / stride 2 / pad 1 convolution (the first convolution of DLA levels 1-5,
 * src/lib/models/networks/pose_dla_dcn.py:32-40,236-246; cuDNN's backward-data in the reference) in ONE launch: per parity
 * class (py, px) of the gradient's rows / columns it is a stride-1 convolution of grad_out with 1, 2, 2 or 4 of the nine
 * taps; grad_out is staged once per workgroup and feeds the four classes' accumulators tap by tap -- the matrix cores do
 * exactly the forward's flops (no multiplications by inserted zeros), grad_out is read once:
 *   grad_in = (residual ? residual : 0) + conv_transpose2d(grad_out, weight, stride 2, pad 1) cropped to H x W
 *   wperm_t  cp_conv_mfma_prepare(weight [Cout][Cin][3][3], Cin := Cout, Cout := Cin, taps 9, transposed = 6)
 *   grad_out [B][Cout][(H - 1) / 2 + 1][(W - 1) / 2 + 1] -> grad_in [B][Cin][H][W], every element written
 *   residual [B][Cin][H][W] or NULL (may be grad_in itself: every element is read, then written, by the same lane) */
int cp_conv3x3_s2_input_grad(const float* grad_out, const void* wperm_t, const float* residual, float* grad_in, int32_t B,
                             int32_t Cin, int32_t H, int32_t W, int32_t Cout, void* stream);

/* Weight gradient of the same convolution, same arithmetic (what the reference gets from cuDNN's backward-filter):
 *   gw[co][ci][ky][kx] += sum_{b,y,x} go[b][co][y][x] * x[b][ci][y - 1 + ky][x - 1 + kx]
 * gw [Cout][Cin][3][3] is ACCUMULATED into (float atomics: zero it first; the summation order varies from run to
 * run in the last bits).  Needs W % 4 == 0; cp_conv3x3_mfma_wgrad_supported tells, else CP_EUNSUPPORTED. */
int cp_conv3x3_mfma_wgrad_supported(int32_t Cin, int32_t Cout, int32_t H, int32_t W);
int cp_conv3x3_mfma_wgrad(const float* x, const float* go, float* gw, int32_t B, int32_t Cin, int32_t H, int32_t W,
                          int32_t Cout, void* stream);
/* the same with taps = 9 (3x3 / pad 1) or 1 (1x1: gw [Cout][Cin][1][1]) */
int cp_conv_mfma_wgrad(const float* x, const float* go, float* gw, int32_t B, int32_t Cin, int32_t H, int32_t W,
                       int32_t Cout, int32_t taps, void* stream);

/* Weight gradient of the same three full-resolution layers (cuDNN backward-filter in the reference), exact fp32 MFMA:
 *   gw[co][ci][ky][kx] += sum_{b,y,x} go[b][co][y][x] * x[b][ci][y*stride - pad + ky][x*stride - pad + kx]
 * gw [Cout][Cin][k][k] is ACCUMULATED into (float atomics: zero it first).  Shapes: (k 7, 3->16, stride 1, pad 3),
 * (k 3, 16->16, stride 1, pad 1), (k 3, 16->32, stride 2, pad 1); cp_conv_direct_wgrad_supported tells. */
int cp_conv_direct_wgrad_supported(int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t pad);
int cp_conv_direct_wgrad(const float* x, const float* go, float* gw, int32_t B, int32_t Cin, int32_t H, int32_t W,
                         int32_t Cout, int32_t k, int32_t stride, int32_t pad, void* stream);

/* The detection heads at inference as ONE kernel (the `fc` Sequentials of DLASeg over their shared input,
 * src/lib/models/networks/pose_dla_dcn.py:445-462,479-481):
 *   out[h][b][o][p] = b2[h][o] + sum_c w2[h][o][c] * relu(b1[h * HC + c] + conv3x3(x, w1)[b][h * HC + c][p])
 * w1 = the heads' 3x3 weights concatenated along the output channels ([nheads * HC][Cin][3][3]) and prepared by
 * cp_conv_mfma_prepare(taps 9) into wperm1; w2[h] = the head's 1x1 weight [cout[h]][HC] prepared by
 * cp_heads_fused_prepare_w2.  The HC-channel intermediate stays in accumulator registers (split-bf16 x3 on both
 * stages).  nheads <= 4, cout[h] <= 128, HC % 64 == 0, Cin % 32 == 0; otherwise CP_EUNSUPPORTED.
 * A head of more than 64 outputs runs as two 64-column segments over the same 3x3 tiles: its w2perm[h] holds two
 * prepared blocks of cp_heads_fused_w2_bytes(HC) bytes back to back, the first from rows 0..63 of w2
 * (cp_heads_fused_prepare_w2(w2, 64, ...)), the second from the rest (cp_heads_fused_prepare_w2(w2 + 64 * HC,
 * cout - 64, ..., w2perm + cp_heads_fused_w2_bytes(HC), ...)).  cp_heads_fused_prepare_w2 itself takes cout <= 64. */
size_t cp_heads_fused_w2_bytes(int32_t head_conv);
int cp_heads_fused_prepare_w2(const float* w2, int32_t cout, int32_t head_conv, void* w2perm, void* stream);
int cp_heads_fused_forward(const float* x, const void* wperm1, const float* b1, const void* const* w2perm,
                           const float* const* b2, float* const* out, const int32_t* cout, int32_t nheads, int32_t B,
                           int32_t Cin, int32_t H, int32_t W, int32_t head_conv, void* stream);

/* Output stage of a detection head at inference (the `fc` Sequential of DLASeg,
 * src/lib/models/networks/pose_dla_dcn.py:445-462: Conv2d 3x3 + bias -> ReLU -> Conv2d 1x1 + bias),
 * everything after the 3x3 convolution's matrix product, one pass:
 *   out[b][o][p] = bias[o] + sum_c w_t[c][o] * act(y[b][c][p] + in_bias[c])
 * y: raw 3x3-conv output, channel slice of a larger tensor allowed (y_bstride = elements between
 * images); in_bias [Cin] or NULL; relu_in != 0 applies ReLU; w_t is the 1x1 weight TRANSPOSED to
 * [Cin][Cout]; bias [Cout] or NULL; out [B][Cout][HW].  Cout <= 32, HW % 4 == 0, 16-byte aligned
 * y / out (otherwise CP_EUNSUPPORTED). */
int cp_conv1x1_act_forward(const float* y, int64_t y_bstride, const float* in_bias, int32_t relu_in,
                           const float* w_t, const float* bias, float* out, int32_t B, int32_t Cin,
                           int32_t Cout, int64_t HW, void* stream);

/* ------------------------------------------------ evaluation result writer --
 * cp_instance_masks: the per-instance rasterisation of CITYSCAPES.format_and_write_to_cityscapes
 * (src/lib/datasets/dataset/cityscapes.py:240-272) for the instances of ONE image, already sorted by
 * ascending depth: polygon fill + outline, radius-2 dilation of the closed Bresenham contour, removal of
 * what nearer instances with score >= 0.5 hide.
 *   poly   DEVICE int32 [n][N][2]  integer (x, y) vertices      flags  DEVICE uint8 [n]: bit 0 = the label
 *   has masks (not pole / traffic sign / traffic light), bit 1 = score >= 0.5 (hides farther instances)
 *   masks  DEVICE uint8 [n][H][W] out, 0 / 255                  counts DEVICE int32 [n] out, non-zero pixels
 * n <= 128, N <= 64.  Equal to PIL 12.2's drawing mask for mask (tests/golden/writer_*.npz). */
int cp_instance_masks(const int32_t* poly, const uint8_t* flags, int32_t n, int32_t N, int32_t H, int32_t W,
                      uint8_t* masks, int32_t* counts, void* stream);

/* ------------------------------------------------ instance-level evaluation --
 * The pixel counting of the Cityscapes instance-level AP (evalInstanceLevelSemanticLabeling.assignGt2Preds and
 * instances2dict of the cityscapesscripts): every count the protocol needs of one image, from the masks
 * cp_instance_masks left on the device and the 16-bit `*_gtFine_instanceIds.png` image.  Integer counts, exact.
 *
 * cp_id_histogram: hist[v] = number of pixels of value v (np.unique + one (img == id).sum() per id, one pass).
 *   ids   DEVICE uint16 [H][W]                 hist  DEVICE int32 [65536] out (zeroed here)
 *
 * cp_instance_overlaps:
 *   masks     DEVICE uint8 [n][H][W], non-zero = inside      gt_ids   DEVICE uint16 [H][W]
 *   inst_ids  DEVICE int32 [G], distinct values of interest  void_ids DEVICE int32 [V] (values outside 16 bits
 *                                                                      match no pixel)
 *   inter       DEVICE int32 [n][G] out: pixels where mask i is set and gt_ids == inst_ids[j]
 *   void_inter  DEVICE int32 [n]    out: pixels where mask i is set and the RAW pixel value is one of void_ids
 *   pred_pixels DEVICE int32 [n]    out: non-zero pixels of mask i
 * n <= 128, G <= 1024, V <= 64, H * W < 2^31 (CP_EUNSUPPORTED otherwise); any H, W and any alignment (16-byte
 * aligned masks with H * W % 16 == 0 take the wide loads).  A fixed number of launches whatever n and G.
 * workspace: cp_instance_overlaps_workspace_bytes (the id -> column table); shorter: CP_EWORKSPACE.  All checks
 * come before any device work. */
int cp_id_histogram(const uint16_t* ids, int32_t H, int32_t W, int32_t* hist, void* stream);
size_t cp_instance_overlaps_workspace_bytes(int32_t n, int32_t G, int32_t H, int32_t W);
int cp_instance_overlaps(const uint8_t* masks, int32_t n, const uint16_t* gt_ids, int32_t H, int32_t W,
                         const int32_t* inst_ids, int32_t G, const int32_t* void_ids, int32_t V, int32_t* inter,
                         int32_t* void_inter, int32_t* pred_pixels, void* workspace, size_t workspace_bytes,
                         void* stream);

/* cp_segment_medians: per segment of an id image the exact median pair of a 16-bit value image (the disparity of a
 * ground-truth instance, for AP 100 m / AP 50 m; datasets/evaluation/distances.py turns it into metres).
 *   ids      DEVICE uint16 [H][W], an id image         values  DEVICE uint16 [H][W], 0 = no measurement
 *   seg_ids  DEVICE int32 [G], distinct (a value outside 16 bits matches no pixel)
 *   out      DEVICE int32 [G][4] out: pixels (ids == seg_ids[j]), valid (those with values != 0), v_lo, v_hi: the
 *            values of 0-based ascending rank (valid - 1) / 2 and valid / 2 among the valid pixels; 0, 0 when valid == 0
 * Exact integers.  G <= 1024, H * W < 2^31 (CP_EUNSUPPORTED otherwise); any H, W; ids and values at any element
 * alignment (16-byte aligned images take the wide loads).  G == 0 is a no-op.  workspace:
 * cp_segment_medians_workspace_bytes (the id -> column table, the high-byte histograms with the counts, the picked
 * buckets, the low-byte histograms; 16-byte aligned), shorter: CP_EWORKSPACE.  All checks come before any device
 * work.  Six launches whatever G and the content, nothing is read back in between. */
size_t cp_segment_medians_workspace_bytes(int32_t G, int32_t H, int32_t W);
int cp_segment_medians(const uint16_t* ids, const uint16_t* values, int32_t H, int32_t W, const int32_t* seg_ids,
                       int32_t G, int32_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* cp_writer_instances: the writer's selection for ONE image on the device -- image_instances plus the label, flag and
 * confidence bookkeeping of format_and_write_to_cityscapes (cityscapes.py:225-238, 266-281) -- from detection rows in
 * the layout cp_polydet_post_process writes to the instance list cp_instance_masks and the evaluator read.
 *   rows   DEVICE fp32 [R][2N + 7]: x1,y1,x2,y2,score,cls,poly(2N),depth (cls counts from 0)
 *   class_table  HOST int32 [C][2]: label id, "the label has masks" (non-zero) of class 0 .. C-1
 *   n_out  DEVICE int32 [1]: live instances        src    DEVICE int32 [R]: source row of every instance
 *   poly   DEVICE int32 [R][N][2]                  flags  DEVICE uint8 [R], the bits of cp_instance_masks
 *   label  DEVICE int32 [R]                        conf   DEVICE fp32 [R]: min(1, score * 1.2f) in fp32
 * A row is live when score > thresh (strict, fp32) and cls is an integer in [0, C).  Instances are in ascending
 * depth, ties by class and then by row (the stable sort of the host loop; a NaN depth sorts last).  A vertex is
 * int(float("%.2f" % v)) = sign(v) (floor|v| + (|v| - floor|v| > 0.995)) in fp64, saturated to int32.  Slots at n_out
 * and above are dead: flags 0 (cp_instance_masks draws nothing), src and label -1, conf 0, vertices 0.  More than
 * 128 live rows are reported through n_out; it is the caller's to refuse them before it reads the masks.
 * 1 <= R <= 1024, 3 <= N <= 64, 1 <= C <= 32: beyond the upper limits CP_EUNSUPPORTED, otherwise (and for null
 * pointers or a NaN threshold) CP_EINVAL, all before any device work.  One launch of one workgroup. */
int cp_writer_instances(const float* rows, int32_t R, int32_t N, float thresh, const int32_t* class_table, int32_t C,
                        int32_t* n_out, int32_t* src, int32_t* poly, uint8_t* flags, int32_t* label, float* conf,
                        void* stream);

/* ------------------------------------------------ KITTI / IDD result writers --
 * cp_class_instance_masks: the per-instance drawing of format_and_write_to_kitti / format_and_write_to_IDD
 * (src/lib/datasets/dataset/kitti_poly.py:126-136, IDD.py:160-170) for the instances of ONE image in drawing order
 * (ascending depth within a group): with F what ImageDraw.polygon(pts, fill=...) sets and O what
 * ImageDraw.polygon(pts, outline=...) sets in PIL 12.2 on an 'L' image,
 *   mask_i = (F_i \ O_i) \ union { F_j : j < i, group_j == group_i, flags_j bit 1 set }
 * (the writers clear to_remove_mask with polygon(outline=0, fill=0), and PIL draws no outline in the fill's ink).
 *   poly   DEVICE int32 [n][N][2]  integer (x, y) vertices      group  DEVICE int32 [n], compared for equality (the
 *   class); the instances of a group need not be adjacent       flags  DEVICE uint8 [n]: bit 0 = draw (0: the mask
 *   is empty and hides nothing), bit 1 = score >= 0.5 (hides farther instances of its group)
 *   masks  DEVICE uint8 [n][H][W] out, 0 / 255, any alignment   counts DEVICE int32 [n] out, non-zero pixels
 * n <= 128, 3 <= N <= 64, H * W < 2^31 (CP_EUNSUPPORTED beyond), any H and W; all checks come before any device
 * work.  F and O are PIL's scan-line fill and integer line restated (csrc/class_masks_core.h), exact for vertices
 * within +-2^24; farther out nothing is written outside the canvas but the drawing is not PIL's.  A fixed number of
 * launches whatever n is; integer results, the same bits on every run. */
int cp_class_instance_masks(const int32_t* poly, const int32_t* group, const uint8_t* flags, int32_t n, int32_t N,
                            int32_t H, int32_t W, uint8_t* masks, int32_t* counts, void* stream);

/* cp_class_writer_instances: the selection of those two writers for ONE image on the device, from detection rows in
 * the layout cp_polydet_post_process writes to the instance list cp_class_instance_masks and the evaluator read.
 *   rows   DEVICE fp32 [R][2N + 7]: x1,y1,x2,y2,score,cls,poly(2N),depth (cls counts from 0)
 *   at_threshold  0: a row is live when score > thresh (KITTI), 1: when score >= thresh (IDD); fp32
 *   class_label   HOST int32 [C]: label id of class 0 .. C-1
 *   n_out  DEVICE int32 [1]: live instances        src    DEVICE int32 [R]: source row of every instance
 *   poly   DEVICE int32 [R][N][2]                  group  DEVICE int32 [R]: the class
 *   flags  DEVICE uint8 [R]: 1 | (score >= 0.5 ? 2 : 0)         label  DEVICE int32 [R]
 *   conf   DEVICE fp32 [R]: the score as it is     text_index DEVICE int32 [R]: the writers' `count`, the line of
 *   the instance in the image's text file = its place in the order (class, row)
 * Instances are in DRAWING order: class, then ascending depth, ties by row (the stable sort of the host loop; a NaN
 * depth sorts last).  Vertices as cp_writer_instances has them.  Slots at n_out and above are dead: flags 0, src,
 * group, label and text_index -1, conf 0, vertices 0.  More than 128 live rows are reported through n_out.
 * 1 <= R <= 1024, 3 <= N <= 64, 1 <= C <= 32: beyond the upper limits CP_EUNSUPPORTED, otherwise (null pointers, a
 * NaN threshold, at_threshold not 0 or 1) CP_EINVAL, all before any device work.  One launch of one workgroup. */
int cp_class_writer_instances(const float* rows, int32_t R, int32_t N, float thresh, int32_t at_threshold,
                              const int32_t* class_label, int32_t C, int32_t* n_out, int32_t* src, int32_t* poly,
                              int32_t* group, uint8_t* flags, int32_t* label, float* conf, int32_t* text_index,
                              void* stream);

/* ------------------------------------------------ instance maps (detectors/instances.py) --
 * cp_instance_map: the masks of ONE image merged, depth resolved, into one map with its per-instance tables -- which
 * instance owns each pixel, the `*_instanceIds.png` / `*_labelIds.png` values, and what every instance shows.
 *   masks  DEVICE uint8 [n][H][W], non-zero = inside (what cp_instance_masks and cp_class_instance_masks leave)
 *   flags  DEVICE uint8 [n]                      counts DEVICE int32 [n] or NULL
 *   label  DEVICE int32 [n]                      prio   DEVICE fp32 [n] or NULL
 *   bounds DEVICE int32 [n][4] inclusive x0, y0, x1, y1, or NULL
 * With
 *   live(i)      (flags[i] & flag_mask) != 0 and (counts NULL or counts[i] > min_count)
 *   covers(i, p) live(i), p inside bounds[i] clipped to the canvas (NULL bounds: the whole canvas; x1 < x0 or y1 < y0:
 *                nothing) and masks[i][p] != 0.  Pixels of a mask outside its bounds are ignored, in every code path
 *                alike: bounds tighter than the mask give a defined result
 *   before(i, j) NULL prio: i < j; otherwise prio[i] < prio[j], or equal and i < j; a NaN sorts after every number,
 *                NaNs among themselves by index
 *   winner(p)    the covering instance that is `before` every other covering instance
 * the outputs are
 *   index   DEVICE uint8 [H][W]: winner(p), 255 where nothing covers
 *   value   DEVICE int32 [n]: label[i] * multiplier + k for a live instance, k the number of live j < i with
 *           label[j] == label[i]; -1 for a dead one
 *   ids     DEVICE int32 [H][W] or NULL (not written): value[winner(p)], `background` where nothing covers
 *   labels  DEVICE int32 [H][W] or NULL (not written): label[winner(p)], `background` where nothing covers
 *   visible DEVICE int32 [n]: pixels instance i wins
 *   box     DEVICE int32 [n][4]: inclusive min x, min y, max x, max y of the pixels it wins; {W, H, -1, -1} when it
 *           wins none or is dead
 * 0 <= n <= 128, H * W < 2^31 (CP_EUNSUPPORTED beyond); H, W >= 1, multiplier >= 1, the required pointers (index
 * always, masks, flags, label, value, visible and box when n > 0) otherwise CP_EINVAL; workspace:
 * cp_instance_map_workspace_bytes (the tables in rank order), shorter: CP_EWORKSPACE.  All checks come before any device
 * work.  n == 0 fills the maps and reads no mask.  Any H, W and any alignment of masks (a 16-pixel piece of a row
 * that lies on a 16-byte boundary takes the wide loads and stores: every full piece when the planes are 16-byte
 * aligned and W % 16 == 0).  A workgroup owns a tile of 16 x 256 pixels and reads a plane only where its clipped
 * bounds meet the tile and pixels are still undecided.  Two launches whatever n is; integer results, the same bits
 * on every run. */
size_t cp_instance_map_workspace_bytes(int32_t n, int32_t H, int32_t W);
int cp_instance_map(const uint8_t* masks, int32_t n, int32_t H, int32_t W, const uint8_t* flags, int32_t flag_mask,
                    const int32_t* counts, int32_t min_count, const int32_t* label, const float* prio,
                    const int32_t* bounds, int32_t multiplier, int32_t background, uint8_t* index, int32_t* ids,
                    int32_t* labels, int32_t* value, int32_t* visible, int32_t* box, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------ pixel-level evaluation --
 * cp_pixel_confusion: the pixel counting of evalPixelLevelSemanticLabeling (cityscapesscripts, kittiscripts) for ONE
 * image -- the confusion matrix (addToConfusionMatrix.cEvaluatePair) and the per-instance counts of the
 * instance-weighted iIoU -- from an 8-bit prediction and the 16-bit instance-id image.
 *   pred        DEVICE uint8 [H][W]                   pred_label  HOST uint8 [256]: label of a prediction byte
 *   gt_ids      DEVICE uint16 [H][W]                  label_group HOST int8 [L]: group of a label, -1 (negative) = none
 *   inst_ids    DEVICE int32 [G], distinct (values outside 16 bits match no pixel)
 *   conf        DEVICE int64 [L][L], ADDED to         inst        DEVICE int32 [G][3], written (zeroed by the call)
 *   bad         DEVICE int32 [2], ADDED to
 * Definitions:
 *   * For pixel x with v = gt_ids[x], the ground-truth label is g = v < id_direct_below ? v : v / id_divisor.
 *       Cityscapes: id_direct_below = 1000, id_divisor = 1000.    KITTI: id_direct_below = 0, id_divisor = 256.
 *   * The predicted label is p = pred_label[pred[x]].
 *   * g >= L: bad[0] += 1 and the pixel is counted nowhere else (in neither conf nor bad[1]).
 *   * Otherwise p >= L: bad[1] += 1 and the pixel is counted nowhere else.
 *   * Otherwise conf[g][p] += 1.
 *   * For column j with id = inst_ids[j] and gl its label by the rule above:
 *       inst[j][0] = pixels with v == id.
 *       inst[j][1] = of those, pixels with p == gl.
 *       inst[j][2] = of those, pixels with label_group[p] == label_group[gl] and label_group[gl] >= 0.
 *       Pixels with a bad p count in inst[j][0] only; so do all pixels of a column with gl >= L.
 *   * Ids not in inst_ids touch no instance column.
 *   * inst is zeroed by the call.  conf and bad are not, so a run keeps its matrix on the device and reads it once at
 *     the end.
 * Limits: 1 <= L <= 64, 0 <= G <= 1024 (with G == 0, inst and inst_ids may be NULL), H * W < 2^31; beyond the upper
 * limits CP_EUNSUPPORTED.  Null pointers, non-positive sizes, id_divisor < 1, id_direct_below < 0: CP_EINVAL.
 * workspace: cp_pixel_confusion_workspace_bytes (the id and prediction tables), shorter: CP_EWORKSPACE.  All checks
 * come before any device work.  Any H, any W, any alignment of pred and gt_ids (a 16-byte aligned image takes 16-byte
 * loads for its full pieces of 16 pixels, each image by itself).  Two launches whatever G is; the counters live in
 * LDS as 32-bit words, which H * W < 2^31 cannot overflow.  Integer results, the same bits on every run. */
size_t cp_pixel_confusion_workspace_bytes(int32_t G);
int cp_pixel_confusion(const uint8_t* pred, const uint8_t* pred_label, const uint16_t* gt_ids, int32_t H, int32_t W,
                       int32_t id_divisor, int32_t id_direct_below, int32_t L, const int8_t* label_group,
                       const int32_t* inst_ids, int32_t G, int64_t* conf, int32_t* inst, int32_t* bad,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------ panoptic quality --
 * The protocol of evalPanopticSemanticLabeling (pq_compute_single_core) for ONE image, with the ground-truth segments
 * that createPanopticImgs derives from the 16-bit instance-id image, counted and matched on the device: nothing comes
 * back to the host per image.
 *
 * cp_panoptic_pairs: the segments of the ground truth and the pixel count of every (segment, prediction) pair.
 *   index       DEVICE uint8 [H][W]: what cp_instance_map writes     n  number of slots, 0 .. 255
 *   gt_ids      DEVICE uint16 [H][W]                                  id_divisor, id_direct_below: as cp_pixel_confusion
 *   label_flags HOST uint8 [L]: bit 0 = evaluated (not ignoreInEval), bit 1 = has instances
 *   seg         DEVICE int32 [1025][4] out, 16-byte aligned      pairs  DEVICE int32 [1025][n + 1] out
 *   - the label of a value v is g = v < id_direct_below ? v : v / id_divisor; the pixel is VOID (row 0) when g >= L or
 *     label g is not evaluated, otherwise it belongs to the segment of value v.  The image's segments are its distinct
 *     non-void values, ascending: rows 1 .. G.  A segment is crowd when v < id_direct_below and its label has
 *     instances.  The column of a pixel is index[x] when that is < n, else n ("no prediction": 255 and anything >= n).
 *   - seg[0] = {G, void pixels, 0, 0}, seg[r] = {value, label, crowd, area}; pairs[r][c] = pixels in row r and column c.
 *     Both are fully written for rows 0 .. min(G, 1024) (pairs is zeroed whole).  With G > 1024, seg[0][0] holds the
 *     true G, the tables hold the first 1024 segments and the pixels of the others are counted nowhere.
 * Limits: 1 <= L <= 64, 0 <= n <= 255, H * W < 2^31; beyond the upper limits CP_EUNSUPPORTED.  Null pointers,
 * non-positive sizes, n < 0, id_divisor < 1, id_direct_below < 0, a misaligned table: CP_EINVAL.  workspace:
 * cp_panoptic_pairs_workspace_bytes (the presence bytes and the id -> row table, 16-byte aligned), shorter:
 * CP_EWORKSPACE.  All checks come before any device work.  Any H, any W, any alignment of index and gt_ids (a 16-byte
 * aligned image takes 16-byte loads for its full pieces of 16 pixels, each image by itself).  Five launches whatever
 * the content; the segments are found on the device (presence pass, then a compaction of the 65536 entries).  The
 * counting keeps a workgroup's table in LDS when (min(G, 1024) + 1) * (n + 1) <= 15360 cells and adds to the global
 * table directly otherwise.  Integer atomics only: the same bits on every run.
 *
 * cp_panoptic_match: the matching on those two tables, one launch of one workgroup.
 *   pred_label  HOST int32 [n]: label of a slot                      label_flags as above
 *   stat        DEVICE int64 [L][3] = tp, fp, fn, ADDED to           iou  DEVICE float64 [L], ADDED to
 *   bad         DEVICE int32 [2], ADDED to                           match DEVICE int32 [n] out, or NULL
 *   - area_p[i] = sum over r of pairs[r][i], area_g[r] = seg[r][3].  Slot i is a predicted segment when area_p[i] > 0
 *     and pred_label[i] is in [0, L) and evaluated; a slot with pixels but another label counts bad[1] += 1 and is
 *     absent (the evaluator raises a KeyError there).
 *   - (r, i) match when r >= 1, row r is not crowd, seg[r][1] == pred_label[i] and 2 * inter > union with
 *     inter = pairs[r][i], union = area_g[r] + area_p[i] - inter - pairs[0][i] (an integer comparison that decides as
 *     the evaluator's float64 inter / union > 0.5 for counts below 2^32).  A match counts tp[label] += 1 and
 *     iou[label] += (double)inter / (double)union; the additions of one image happen in ascending row order, each onto
 *     the running value, so the sum is the evaluator's sequence of operations and the same bits on every run.
 *   - every non-crowd row without a match: fn[label] += 1.  Every existing slot without a match: with
 *     x = pairs[0][i] + pairs[rc][i], rc the crowd row of the slot's label (the one of highest value if several),
 *     the slot is ignored if 2 * x > area_p[i], otherwise fp[label] += 1.
 *   - match[i] = the matched row, 0 for an existing unmatched slot, -1 for an absent one.
 *   - seg[0][0] > 1024: bad[0] += 1, match is all -1 and nothing else is added for the image.
 * Limits and codes as above; stat and iou 8-byte aligned. */
size_t cp_panoptic_pairs_workspace_bytes(void);
int cp_panoptic_pairs(const uint8_t* index, int32_t n, const uint16_t* gt_ids, int32_t H, int32_t W, int32_t id_divisor,
                      int32_t id_direct_below, int32_t L, const uint8_t* label_flags, int32_t* seg, int32_t* pairs,
                      void* workspace, size_t workspace_bytes, void* stream);
int cp_panoptic_match(const int32_t* seg, const int32_t* pairs, int32_t n, const int32_t* pred_label, int32_t L,
                      const uint8_t* label_flags, int64_t* stat, double* iou, int32_t* bad, int32_t* match, void* stream);

/* ------------------------------------------------ instance tracking (detectors/tracking.py) --
 * Links the instances of one frame (cp_instance_map's `index`) to the tracks of the frames before it by the IoU of the
 * pixels they own.  Not in the reference tree: a capability of this library, defined here and pinned by the host
 * statement tests/golden/tracking_host.py.
 *
 * A tracker belongs to one canvas (W, H) and keeps on the device
 *   mem     uint16 [H][W]: the track slot that last owned the pixel, 0xffff for none
 *   slots   int32 [CP_TRACK_SLOTS][5] = {track_id, label, first_frame, last_seen, hits}; track_id >= 1, 0 marks a free
 *           slot (the whole row is then 0)
 *   next_id int32 [1], starting at 1: track ids rise by one per new track and are never reused within a run; freed slots
 *           are reused, lowest index first
 * and the host keeps the frame counter t, starting at 0.  One step takes a frame's index (uint8 [H][W], 255 = none),
 * n <= 128 instances, a label and a live flag per instance:
 *   1. counts.  inter[s][k] = pixels with mem == s and index == k, area_mem[s] = pixels with mem == s, area_cur[k] =
 *      pixels with index == k.  Exact integers (cp_map_pairs with R = CP_TRACK_SLOTS and no lookup).
 *   2. association (cp_track_associate).  (s, k) is a candidate when slot s is occupied, k is live, the labels are
 *      equal, inter > 0 and (double)inter / (double)(area_mem[s] + area_cur[k] - inter) >= iou_thresh -- one correctly
 *      rounded float64 division of two integers against the float64 threshold.  Greedy: take the candidate of largest
 *      IoU, compared exactly as fractions (inter_a * union_b against inter_b * union_a in 64-bit integers), ties to
 *      the smaller track_id, then the smaller k; match it, drop its row and column, repeat until none is left.  A
 *      matched instance takes the slot's track id, last_seen = t, hits += 1.  Every unmatched live instance, in
 *      ascending k, takes the lowest free slot: {next_id++, label, t, t, 1}.  Then every slot with
 *      last_seen < t - max_age is freed (max_age 0: a track not seen in this frame ends here).  If an instance finds no
 *      free slot, status = 1 and nothing else is written: slots, next_id and (through cp_track_update) mem stay as
 *      they were.
 *   3. update (cp_track_update), one pass: mem[p] = the slot of the instance that owns p; else its old slot if that
 *      slot is still occupied and took no instance in this frame (a lost track keeps what is left of its last mask, a
 *      track seen in this frame remembers exactly its current mask); else 0xffff.  ids[p] = label * multiplier +
 *      track_id of the owner, 0 where there is none.
 * and then t += 1.
 *
 * cp_map_pairs: the pixel count of every (row, column) pair of a 16-bit map and a byte map.
 *   a       DEVICE uint16 [H][W]                              b  DEVICE uint8 [H][W]
 *   row_of  DEVICE uint16 [65536] or NULL (identity): the row of a value of a; a row >= R (0xffff) is "none", row R
 *   R       rows, 0 .. 1024      n  columns, 0 .. 255: the column of a pixel is b when that is < n, else n ("none")
 *   pairs   DEVICE int32 [R + 1][n + 1] out, zeroed by the call: row sums and column sums are the areas
 * R > 1024, n > 255, H * W >= 2^31: CP_EUNSUPPORTED; null a, b or pairs, non-positive H or W, negative R or n, a
 * misaligned table: CP_EINVAL.  No workspace.  Any H, any W, any alignment of a and b (a 16-byte aligned image takes
 * 16-byte loads for its full pieces of 16 pixels, each image by itself).  Two launches; a workgroup's table lives in
 * LDS when (R + 1) * (n + 1) <= 33153 cells (257 x 129, the tracker's whole range) and the counts go to the global
 * table directly otherwise.  Integer atomics only: the same bits on every run.
 *
 * cp_track_associate: stage 2 on the pair table [CP_TRACK_SLOTS + 1][n + 1], one launch of one workgroup.
 *   label    HOST int32 [n]      live  HOST uint8 [n], non-zero = live      slots, next_id  DEVICE, in and out
 *   inst     DEVICE int32 [n][5] out = {slot, track_id, matched inter, matched union, is_new}; {-1, 0, 0, 0, 0} for a
 *            dead instance, inter = union = 0 for a new track
 *   assigned DEVICE uint8 [CP_TRACK_SLOTS] out: 1 where the slot took an instance in this frame, matched or new
 *   status   DEVICE int32 [1] out: 0, or 1 = more than CP_TRACK_SLOTS tracks alive (nothing else was written)
 * n > 128: CP_EUNSUPPORTED; iou_thresh outside (0, 1] or NaN, max_age < 0, t < 0, null or misaligned tables: CP_EINVAL.
 *
 * cp_track_update: stage 3 from the tables cp_track_associate wrote; writes nothing when status[0] != 0.
 *   mem  DEVICE uint16 [H][W] in and out      ids  DEVICE int32 [H][W] out      label  HOST int32 [n]
 * Limits and codes as above, multiplier >= 1; any H, W and alignment of index, mem and ids. */
#define CP_TRACK_SLOTS 256
int cp_map_pairs(const uint16_t* a, const uint16_t* row_of, int32_t R, const uint8_t* b, int32_t n, int32_t H, int32_t W,
                 int32_t* pairs, void* stream);
int cp_track_associate(const int32_t* pairs, int32_t n, const int32_t* label, const uint8_t* live, int32_t* slots,
                       int32_t* next_id, double iou_thresh, int32_t max_age, int32_t t, int32_t* inst, uint8_t* assigned,
                       int32_t* status, void* stream);
int cp_track_update(const uint8_t* index, int32_t n, const int32_t* label, int32_t H, int32_t W, const int32_t* slots,
                    const int32_t* inst, const uint8_t* assigned, const int32_t* status, int32_t multiplier,
                    uint16_t* mem, int32_t* ids, void* stream);

/* ------------------------------------------------ instance tracking with motion (detectors/tracking.py, motion=True) --
 * The same tracker with every track's remembered pixels moved to where the track should be now, at constant velocity
 * (as SORT does for boxes), before they are compared with the frame.  Not in the reference tree: this project's rule,
 * pinned by the host statement tests/golden/tracking_motion_host.py.  All quantities are integers; positions and
 * velocities are in 1/16 pixel; every product and quotient below is computed in 64 bits.
 *
 * Beside mem, slots and next_id the tracker keeps
 *   kin     int32 [CP_TRACK_SLOTS][6] = {cx, cy, vx, vy, seen, valid}, all zero for a new tracker
 * and a step at frame t is
 *   1. predict (cp_track_predict).  For a slot with track_id != 0 and valid: g = t - seen,
 *      dx = clamp(floor((vx * g + 8) / 16), -W, W), dy = clamp(floor((vy * g + 8) / 16), -H, H) (floor division: round
 *      half up); (0, 0) for every other slot.
 *   2. shifted counts (cp_map_pairs_shifted with R = CP_TRACK_SLOTS).  For every pixel (x, y) with s = mem[y][x] < R:
 *      q = (x + dx[s], y + dy[s]); if q lies on the canvas pairs[s][c] += 1 with c = index[q] when that is < n, else n;
 *      a pixel whose q is off the canvas is counted nowhere (the predicted footprint is clipped).  Row R, column k =
 *      area_cur[k] - the sum of pairs[s][k] over s < R, with area_cur[k] the pixels with index == k (k = n: index >= n).
 *      Row R may be negative: two predictions may land on the same pixels.  The row sum of s is its clipped predicted
 *      area and every column sum is the instance's true area, which is all cp_track_associate reads beside the cells:
 *      IoU = inter / (predicted area + area_cur - inter).  With all shifts zero the table is cp_map_pairs' bit for bit.
 *   3. cp_track_associate, unchanged.
 *   4. kinematics (cp_track_kinematics).  With A, Sx, Sy the pixel count and the sums of x and y over index == k:
 *      cx = floor((32 * Sx + A) / (2 * A)), cy likewise.  For every instance k with inst[k].slot = s >= 0:
 *        A == 0 and is_new               kin[s] = 0
 *        A == 0 and not new              kin[s] stays (a match needs inter > 0, so this does not happen)
 *        is_new, or kin[s].valid == 0    kin[s] = {cx, cy, 0, 0, t, 1}
 *        otherwise                       g = t - kin[s].seen, v = (c - c_old) / g rounded toward zero per axis,
 *                                        kin[s] = {cx, cy, vx, vy, t, 1}
 *      The velocity is the one between the last two sightings, without smoothing.  Afterwards every slot with
 *      track_id == 0 has kin[s] = 0.  With status[0] != 0 nothing in kin changes.
 *   5. cp_track_update, unchanged.  A lost track's remembered pixels stay where they were at frame kin.seen, which is
 *      why the shift of step 1 grows with g.
 *
 * cp_map_pairs_shifted: cp_map_pairs without the lookup and with a shift per row.
 *   shift   DEVICE int32 [R][2] = {dx, dy}, any values (NULL only with R == 0)
 * Limits and codes are cp_map_pairs': R > 1024, n > 255, H * W >= 2^31: CP_EUNSUPPORTED; null a, b, pairs or shift,
 * non-positive H or W, negative R or n, a misaligned table: CP_EINVAL; all checks come before any device work.  Any H,
 * any W, any alignment of a and b.  Two launches: the clear, then one pass that streams a and b (which gives area_cur)
 * and gathers b at the shifted positions -- 16 contiguous bytes at whatever byte offset for a piece of 16 pixels of one
 * image row that all belong to one slot and land on the canvas, a byte per pixel for every other piece that holds a
 * track.  The workgroup's table lives in LDS up to 33153 cells and in the global table beyond.  Integer atomics only.
 *
 * cp_track_predict: step 1 for the CP_TRACK_SLOTS rows, one launch.  shift DEVICE int32 [CP_TRACK_SLOTS][2] out.  Null or
 * misaligned tables, non-positive H or W, t < 0: CP_EINVAL.
 *
 * cp_track_kinematics: step 4 from the tables cp_track_associate wrote.  One memset, one streaming pass over index
 * ({A, Sx, Sy} per instance in 64-bit integers) and one launch of one workgroup for the table.
 *   workspace  DEVICE, 8-byte aligned, cp_track_kinematics_workspace_bytes(n) (24 bytes an instance; none for n == 0)
 * n > 128, H * W >= 2^31, H or W > 2^26 (16 * x must fit 32 bits): CP_EUNSUPPORTED; null or misaligned tables,
 * non-positive H or W, negative n or t: CP_EINVAL; a null or shorter workspace: CP_EWORKSPACE. */
int cp_map_pairs_shifted(const uint16_t* a, const int32_t* shift, int32_t R, const uint8_t* b, int32_t n, int32_t H,
                         int32_t W, int32_t* pairs, void* stream);
int cp_track_predict(const int32_t* slots, const int32_t* kin, int32_t t, int32_t H, int32_t W, int32_t* shift,
                     void* stream);
size_t cp_track_kinematics_workspace_bytes(int32_t n);
int cp_track_kinematics(const uint8_t* index, int32_t n, int32_t H, int32_t W, const int32_t* inst, const int32_t* slots,
                        const int32_t* status, int32_t t, int32_t* kin, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ------------------------------------------------ run-length masks (utils/rle.py) --
 * COCO's run-length encoding of binary masks, {"size": [H, W], "counts": "<string>"}, encoded from and decoded to device
 * masks.  Not in the reference tree, and no COCO library is part of this project: the format is restated here from the
 * published algorithm and pinned by the literal host statement tests/golden/rle_host.py.
 *
 * Counts.  A pixel of M[H][W] is set when its byte is non-zero.  Read the pixels in column-major order, j = x * H + y,
 * starting from an imagined value 0 before j = 0.  cnts[0] is the number of leading zeros (0 when pixel (0, 0) is set),
 * cnts[1] the length of the following run of ones, and so on alternating; the last run ends at H * W.  So
 * sum(cnts) == H * W, the odd entries sum to the area, and m = changes + 1.
 * String.  For i = 0 .. m - 1: x = cnts[i], and for i > 2, x -= cnts[i - 2] (signed).  Then repeat: c = x & 0x1f;
 * x >>= 5 (arithmetic); more = (c & 0x10) ? (x != -1) : (x != 0); if more, c |= 0x20; emit chr(c + 48); until more is
 * false.  With H * W < 2^31 a number takes 1 .. 7 characters.
 * Parsing a number.  x = 0, k = 0; per character: c = ord(ch) - 48; x |= (c & 0x1f) << 5k; more = c & 0x20; k += 1.
 * When more is 0 the number ends; if c & 0x10 then, x |= -1 << 5k.  After number i > 2, add cnts[i - 2].
 *
 * cp_rle_encode: counts and strings of n masks in one call, six launches whatever n is.
 *   planes   DEVICE uint8 [n][H][W], non-zero = set, n <= 128      -- exactly one of the two is non-NULL --
 *   index    DEVICE uint8 [H][W]: mask k is index == k, 1 <= n <= 255 (cp_instance_map's index; 255 = nobody)
 *   bounds   DEVICE int32 [n][4] inclusive x0, y0, x1, y1, or NULL: the caller promises that mask k is zero outside its
 *            box (x1 < x0 or y1 < y0, as W, H, -1, -1: empty).  Only the box is read, clipped to the image; column
 *            x1 + 1, where a mask on the bottom row of column x1 ends, belongs to the work
 *   counts   DEVICE uint32 [cap_counts] out or NULL: all masks back to back in slot order, mask k at the sum of the m
 *            before it
 *   chars    DEVICE bytes [cap_bytes] out: the strings back to back, no terminators (NULL only with cap_bytes == 0)
 *   table    DEVICE int32 [n][4] out = m, area, byte offset into chars, byte length
 *   head     DEVICE int32 [4] out = total counts, total bytes, overflow flag, 0
 * When the total counts (with counts given) or the total bytes exceed their capacity the flag is 1 and nothing is
 * written at or beyond either capacity; table and head are complete all the same (the lengths are computed from the
 * masks, not from stored counts), so a second call can be sized from them.  Values beyond int32 saturate.
 * H * W >= 2^31, n > 128 with planes, n > 255 with index: CP_EUNSUPPORTED; both or neither of planes and index, n < 1,
 * non-positive H or W, a negative capacity, null table, head or (with cap_bytes > 0) chars, misaligned tables:
 * CP_EINVAL; workspace NULL or shorter than cp_rle_encode_workspace_bytes: CP_EWORKSPACE (24 bytes per mask, column and
 * row segment, 8 segments: n * W * 192 bytes and the per-mask records, of which only the columns of a mask's box are
 * touched; it does not depend on cap_counts, which the query takes for the caller's convenience; 16-byte aligned).  All checks come before any device work.  Any H, W and
 * alignment of the masks.  No atomics: the same bits on every run.
 *
 * cp_rle_decode: n planes from counts.
 *   counts   DEVICE uint32: the counts of all masks      table  HOST int32 [n][2] = offset into counts and m per mask
 *   value    0 .. 255, the byte of a set pixel             planes DEVICE uint8 [n][H][W] out, every byte written
 *   status   DEVICE int32 [n] out: 0, or 1 with an all-zero plane when sum(cnts) != H * W (so also when a running sum
 *            passes H * W, or m == 0).  Counts of zero are legal anywhere.
 * 1 <= n <= 255, H * W < 2^31 (CP_EUNSUPPORTED beyond); null table, planes, status or (with any m > 0) counts, a
 * negative offset or m, value outside 0 .. 255: CP_EINVAL; workspace NULL or shorter than
 * cp_rle_decode_workspace_bytes(n, max(offset + m)) (the run ends, 4 bytes a count): CP_EWORKSPACE.  Two launches. */
size_t cp_rle_encode_workspace_bytes(int32_t n, int32_t H, int32_t W, int64_t cap_counts);
int cp_rle_encode(const uint8_t* planes, const uint8_t* index, int32_t n, int32_t H, int32_t W, const int32_t* bounds,
                  uint32_t* counts, int64_t cap_counts, uint8_t* chars, int64_t cap_bytes, int32_t* table, int32_t* head,
                  void* workspace, size_t workspace_bytes, void* stream);
size_t cp_rle_decode_workspace_bytes(int32_t n, int64_t total_counts);
int cp_rle_decode(const uint32_t* counts, const int32_t* table, int32_t n, int32_t H, int32_t W, int32_t value,
                  uint8_t* planes, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------ device PNG stream (utils/png.py) --
 * The zlib stream of a grey PNG image, 8 or 16 bit, compressed on the device so that only compressed bytes go to the
 * host, which frames them (signature, IHDR, one IDAT, IEND, CRC-32s).  Not in the reference tree: the format is zlib's
 * (RFC 1950, RFC 1951) with every choice fixed below, pinned by the literal host statement tests/golden/png_host.py;
 * zlib and PIL decode it.
 *
 * Filtered stream.  D = bits / 8 bytes per pixel, 16-bit pixels big-endian.  S is H rows of one filter byte 0 (filter
 * "None") followed by W * D pixel bytes; its length is L = H * (1 + W * D).
 * Tokens, chosen greedily from i = 0: r = the number of consecutive positions j = i, i + 1, ... with j >= D and
 * S[j] == S[j - D], capped at 258 and at L - i.  r >= 3: a match (length r, distance D), advance by r; otherwise the
 * literal S[i], advance by 1.  (Equivalently, in a maximal interval [a, b) of positions equal to their D-predecessor
 * the chunks of 258 from a are matches, the remainder (b - a) mod 258 is one match if >= 3 and else 1 or 2 literals,
 * and every other position is a literal.  Runs cross row ends; the filter byte is an ordinary byte of S.)
 * zlib stream, bits packed LSB first, Huffman codes MSB first: bytes 0x78 0x01; BFINAL = 1, BTYPE = 01 (one
 * fixed-Huffman block); the tokens; end-of-block (symbol 256); zero bits to a byte; Adler-32 of S, big-endian.
 * Literal/length codes: symbols 0-143 8 bits from 0x30, 144-255 9 bits from 0x190, 256-279 7 bits from 0, 280-287 8
 * bits from 0xC0.  Length symbol 257 + k: k 0-7 bases 3..10, no extra bits; 8-11 bases 11, 13, 15, 17, 1 bit; 12-15
 * bases 19, 23, 27, 31, 2 bits; 16-19 bases 35, 43, 51, 59, 3 bits; 20-23 bases 67, 83, 99, 115, 4 bits; 24-27 bases
 * 131, 163, 195, 227, 5 bits; k = 28 is 258, no extra bits.  The extra bits follow the length code, LSB first; the
 * distance is the 5-bit code D - 1 with no extra bits.
 *
 * cp_png_deflate: the zlib streams of n images in one call, seven launches and a fill whatever n is.
 *   planes_u8   DEVICE uint8 [n][H][W], bits = 8: the bytes as they are         -- exactly one of the two is non-NULL --
 *   images_i32  DEVICE int32 [n][H][W], bits 8 or 16: the low `bits` bits of every value (the caller refuses an image
 *               whose range in `table` does not fit)
 *   bounds      DEVICE int32 [n][4] inclusive x0, y0, x1, y1, or NULL, as in cp_rle_encode: the caller promises that
 *               image k is zero outside its box (W, H, -1, -1: empty); nothing outside it is read
 *   out         DEVICE bytes [cap_bytes] out, 4-byte aligned: the streams back to back (NULL only with cap_bytes == 0)
 *   table       DEVICE int32 [n][4] out = byte offset, byte length of the stream, minimum, maximum of the values
 *   head        DEVICE int32 [4] out = bytes needed in total, overflow flag, 0, 0
 * When the total exceeds cap_bytes the flag is 1 and no stream is written (out is zero); table and head are complete
 * all the same, so a second call at head[0] succeeds.  Nothing is ever written at or beyond out + cap_bytes.  Sizes
 * beyond int32 saturate.  n > 128, H or W > 16384, n * L >= 2^31: CP_EUNSUPPORTED; both or neither input, planes_u8
 * with bits 16, bits not 8 or 16, n < 1, non-positive H or W, a negative capacity, null table, head or (with cap_bytes
 * > 0) out, misaligned pointers: CP_EINVAL; workspace NULL or shorter than cp_png_deflate_workspace_bytes (40 bytes
 * per tile of 4096 stream bytes and the per-image records; 16-byte aligned): CP_EWORKSPACE.  All checks come before
 * any device work.  Whole words leave as vector stores; a word shared by two tiles or two streams is merged with an
 * integer atomic OR into the zeroed output, which commutes: the same bytes on every run. */
size_t cp_png_deflate_workspace_bytes(int32_t n, int32_t H, int32_t W, int32_t bits);
int cp_png_deflate(const uint8_t* planes_u8, const int32_t* images_i32, int32_t n, int32_t H, int32_t W, int32_t bits,
                   const int32_t* bounds, uint8_t* out, int64_t cap_bytes, int32_t* table, int32_t* head,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------ boundary evaluation (evaluation/boundary.py) --
 * cp_boundary_overlaps: the pixel counting of Boundary IoU / Boundary AP (Cheng et al., CVPR 2021) for ONE image --
 * the boundary band of every predicted mask and of every ground-truth value, and their pair counts.  Not in the
 * reference tree: a capability of this library, defined here and pinned by the host statement
 * tests/golden/boundary_host.py.
 * For a set M of pixels of the H x W image and an integer d >= 1,
 *   band(M, d) = { p in M : some q with max(|qx - px|, |qy - py|) <= d lies outside the image or not in M }
 * -- what the published implementation computes with one ring of zeros around the mask, d erosions by the 3 x 3
 * square and `mask - eroded`; a pixel closer than d to the image edge is always in the band.  Integer and exact.
 *   masks     DEVICE uint8 [n][H][W], non-zero = inside      gt_ids   DEVICE uint16 [H][W]
 *   bounds    DEVICE int32 [n][4] inclusive x0, y0, x1, y1, or NULL: as cp_instance_map takes them -- mask i is its
 *             non-zero pixels inside bounds[i] clipped to the image (NULL: the whole image; x1 < x0 or y1 < y0:
 *             nothing); pixels outside are ignored in every code path alike
 *   inst_ids  DEVICE int32 [G], distinct values of interest (values outside 16 bits match no pixel)
 *   d         the band's width in pixels; the caller computes max(1, round(ratio * sqrt(H * H + W * W)))
 * The ground-truth set of value v is { p : gt_ids[p] == v }, for EVERY value of the image, of interest or not (stuff
 * and void regions delimit their neighbours), so one band image holds all ground-truth bands: p is in it iff its
 * (2d + 1)^2 window leaves the image or holds another value.  Outputs (zeroed by the call):
 *   b_pred   DEVICE int32 [n]:    |band(mask_i, d)|
 *   b_gt     DEVICE int32 [G]:    band pixels of value inst_ids[j]
 *   b_inter  DEVICE int32 [n][G]: pixels of band(mask_i, d) that are in the ground-truth band and have
 *            gt_ids == inst_ids[j]
 *   pred_bands DEVICE uint8 [n][H][W] or NULL (not written), gt_band DEVICE uint8 [H][W] or NULL (not written): the
 *            bands as 255 / 0, as cp_instance_masks writes masks; for tests and debug pictures
 * 0 <= n <= 128, 0 <= G <= 1024, 1 <= d <= 64, H * W < 2^31: beyond the upper limits CP_EUNSUPPORTED; H, W < 1, d < 1,
 * negative n or G and a null required pointer (gt_ids always; masks and b_pred when n > 0; inst_ids and b_gt when
 * G > 0; b_inter when both) CP_EINVAL; workspace: cp_boundary_overlaps_workspace_bytes (the id -> column table and the
 * bit images of the separable erosion: 128 KiB + (4 + 2n) * H * ceil(W / 32) * 4 bytes), shorter or NULL:
 * CP_EWORKSPACE.  All checks come before any device work.  Any H, W and any alignment of masks.  With n == 0 the
 * ground-truth side is still computed.  Five launches (three when n == 0; one more fill when pred_bands and bounds are
 * both given), whatever n, G and d are; integer results, the same bits on every run. */
size_t cp_boundary_overlaps_workspace_bytes(int32_t n, int32_t G, int32_t H, int32_t W, int32_t d);
int cp_boundary_overlaps(const uint8_t* masks, int32_t n, const int32_t* bounds, const uint16_t* gt_ids, int32_t H,
                         int32_t W, int32_t d, const int32_t* inst_ids, int32_t G, int32_t* b_inter, int32_t* b_pred,
                         int32_t* b_gt, uint8_t* pred_bands, uint8_t* gt_band, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------ training annotations (make_annotations.py) --
 * The "regular interval" recipe of the reference's offline annotation tools (KITTIPolyStuff/Tools/
 * create_annotations.py:107-166, cityscapesStuff/Tools/create_bouding_box_annotations.py:135-215, IDDStuff/Tools/
 * create_annotations.py:100-166) for the objects of ONE image.  With k = N / 4, qx = (x1 - x0) / k and qy = (y1 - y0) / k
 * in fp64, vertex j of an object with box (x0, y0, x1, y1) starts at
 *   j = i:       (round(x0 + i qx), y0)      j = k + i:   (x1, round(y0 + i qy))
 *   j = 2k + i:  (round(x1 - i qx), y1)      j = 3k + i:  (x0, round(y1 - i qy))          i = 0 .. k-1
 * (round = half-to-even on the fp64 value fl(x0 + fl(i q)), no FMA; both coordinates then truncated towards zero),
 * walks the `bresenham` package's line to the centre (int(x0 + (x1 - x0) / 2), int(y0 + (y1 - y0) / 2)), both ends
 * included, every pixel clipped to the canvas, and is the first clipped pixel whose mask is set -- the clipped centre
 * when there is none.  Integer results, the same bits on every run.  All checks come before any device work.
 *
 * cp_annot_id_instances: the objects of a 16-bit instance image v = label * divisor + k (the KITTI tool: divisor 256).
 *   ids   DEVICE uint16 [H][W]        class_label  HOST int32 [C]: label of class 0 .. C-1
 *   n_out DEVICE int32 [1]: the distinct non-zero values whose v / divisor is one of class_label
 *   inst_id DEVICE int32 [max_inst]: those values, ascending (the place in this order is the tool's pseudo-depth)
 *   cls   DEVICE int32 [max_inst]: the class       box  DEVICE int32 [max_inst][4]: min x, min y, max x, max y of its pixels
 * Slots at n_out and above: inst_id 0, cls -1, box 0.  More than max_inst objects are reported through n_out; the
 * caller refuses them.  1 <= C <= 32, 1 <= max_inst <= 1024, H * W < 2^31 (CP_EUNSUPPORTED beyond); any H, W and
 * alignment.  workspace: cp_annot_id_instances_workspace_bytes (the box table of 65536 values); shorter: CP_EWORKSPACE.
 *
 * cp_polygon_masks: ImageDraw.polygon(pts, outline=0, fill=255) on a fresh 'L' image for each of n polygons on its
 * own canvas -- F \ O in the words of cp_class_instance_masks, no occlusion -- for polygons of any length.
 *   xy     DEVICE int32 [T][2]: the vertices of all polygons, one after the other
 *   first  HOST int32 [n + 1]: polygon i is xy[first[i] .. first[i + 1]), first[0] = 0, T = first[n]
 *   masks  DEVICE uint8 [n][H][W] out, 0 / 255, any alignment      counts DEVICE int32 [n] out, non-zero pixels
 * n <= 128, 3 <= vertices of a polygon <= 4096, H * W < 2^31 (CP_EUNSUPPORTED beyond; fewer than 3 vertices or a
 * first[] that does not start at 0: CP_EINVAL).  The arithmetic is csrc/class_masks_core.h, exact for vertices within
 * +-2^24.  workspace: cp_polygon_masks_workspace_bytes(n, T) (the edge table); shorter: CP_EWORKSPACE.  A fixed number
 * of launches whatever n and T.
 *
 * cp_annot_rays_ids / cp_annot_rays_masks: the N vertices of n objects; the mask of object i is ids == inst_id[i],
 * or masks[i] > 0.
 *   box   DEVICE fp64 [n][4]: x0, y0, x1, y1 as the tool holds them (integers for an id image, the untruncated
 *         numbers of a polygon file)            inst_id DEVICE int32 [n]
 *   poly  DEVICE int32 [n][N][2] out
 * 4 <= N <= 64 and N % 4 == 0 (otherwise CP_EINVAL, beyond 64 CP_EUNSUPPORTED), n <= 1024, H * W < 2^31.  Every mask
 * read is clipped to the canvas and every walk ends with its line, whatever the box holds (coordinates are kept
 * within +-2^29, a NaN at 0; the recipe is the tools' for boxes within +-2^24). */
size_t cp_annot_id_instances_workspace_bytes(void);
int cp_annot_id_instances(const uint16_t* ids, int32_t H, int32_t W, const int32_t* class_label, int32_t C,
                          int32_t divisor, int32_t max_inst, int32_t* n_out, int32_t* inst_id, int32_t* cls,
                          int32_t* box, void* workspace, size_t workspace_bytes, void* stream);
size_t cp_polygon_masks_workspace_bytes(int32_t n, int32_t total_vertices);
int cp_polygon_masks(const int32_t* xy, const int32_t* first, int32_t n, int32_t H, int32_t W, uint8_t* masks,
                     int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int cp_annot_rays_ids(const uint16_t* ids, int32_t H, int32_t W, const int32_t* inst_id, const double* box, int32_t n,
                      int32_t N, int32_t* poly, void* stream);
int cp_annot_rays_masks(const uint8_t* masks, int32_t H, int32_t W, const double* box, int32_t n, int32_t N,
                        int32_t* poly, void* stream);

/* ------------------------------------------------ ground-truth id images (make_ground_truth.py) --
 * cp_polygon_paint: the painter of the evaluators' preparation scripts (IDDscripts/preperation/json2instanceImg.py:
 * 132-206 and json2labelImg.py:85-146, cityscapesscripts/preparation/json2instanceImg.py:111-166 and json2labelImg.py:
 * 78-122) for ONE image: a canvas of `background`, then ImageDraw.polygon(pts, fill=value[i]) for i = 0 .. n-1 in this
 * order, each overwriting what lies under it.  image[y][x] = value[i] of the LARGEST i whose fill F_i holds (x, y),
 * `background` where there is none; F is the fill of cp_class_instance_masks (no outline), the arithmetic
 * csrc/class_masks_core.h, exact for vertices within +-2^24.  A polygon of two vertices (a, b) is drawn as F of
 * (a, b, a): PIL's edge list for it.
 *   xy     DEVICE int32 [T][2]: the vertices of all polygons, one after the other
 *   first  HOST int32 [n + 1]: polygon i is xy[first[i] .. first[i + 1]), first[0] = 0, T = first[n]; ordinary
 *          (pageable) host memory has been read when the call returns, pinned memory only when the stream reaches
 *          the copy: keep a pinned array unchanged until then
 *   value  DEVICE int32 [n]           image  DEVICE int32 [H][W] out
 * 0 <= n <= 4096 (n = 0: the background image; xy, first, value and workspace may then be null), 2 <= vertices of a
 * polygon <= 4096, T <= 2^20, H * W < 2^31, W <= 16384 (the row is held in LDS): beyond the upper limits
 * CP_EUNSUPPORTED; null pointers, first[0] != 0, a polygon of fewer than 2 vertices, non-positive H or W: CP_EINVAL.
 * workspace: cp_polygon_paint_workspace_bytes(n, T) (the edge table, `first` and the y-ranges); shorter: CP_EWORKSPACE.
 * All checks come before any device work.  Nothing is written outside the canvas, whatever the vertices hold.  One
 * workgroup per row walks the polygons in order: no atomics on memory, no read-modify-write of the image, one copy and
 * two launches whatever n is, the same bits on every run. */
size_t cp_polygon_paint_workspace_bytes(int32_t n, int32_t total_vertices);
int cp_polygon_paint(const int32_t* xy, const int32_t* first, const int32_t* value, int32_t n, int32_t background,
                     int32_t H, int32_t W, int32_t* image, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------ detection overlays (demo.py, --debug) --
 * cp_render_overlay: the picture of ONE image's detections, composed on the device from the instance list
 * cp_writer_instances left there (run with thresh = vis_thresh and a class table in which every class has masks).
 *   image  DEVICE uint8 [H][W][3], the channel order is the caller's          out  DEVICE uint8 [H][W][3], may be image
 *   rows   DEVICE fp32 [R][2N + 7], the rows the list was made from           n    DEVICE int32 [1], cp_writer_instances' n_out
 *   src    DEVICE int32 [R]      poly  DEVICE int32 [R][N][2]                 palette  DEVICE uint8 [C][3]
 *   label_codes  DEVICE int32 [R][L]: per SOURCE row the glyph codes of its label, ended by a negative code
 *   atlas  DEVICE uint8 [G][11][6]: non-zero = set pixel of glyph g in its 6 x 11 cell (a code >= G is a blank cell)
 * The list is nearest first; instance i has paint index p = n - 1 - i (farthest painted first) and contributes, in
 * this order, with (x1, y1, x2, y2) the row's box truncated toward zero to int32 and colour = palette[class]
 * (255 - palette[class] under white_theme):
 *   1 fill      the pixels ImageDraw.polygon(pts, fill=...) of PIL 12.2 sets: (orig * (256 - alpha) + colour * alpha
 *               + 128) >> 8 per channel, orig being the INPUT image;
 *   2 outline   the pixels ImageDraw.polygon(pts, outline=...) sets, dilated by the (2 r + 1)^2 square, clipped:
 *               outline_colour;
 *   3 box       the pixels x1 <= x <= x2, y1 <= y <= y2 with min(x - x1, x2 - x, y - y1, y2 - y) < box_thickness: colour;
 *   4 label background   x1 <= x < x1 + 6 len, y1 - 12 <= y <= y1 - 2 (len = the label's length): colour;
 *   5 label glyphs       the set pixels of glyph j in the cell at (x1 + 6 j, y1 - 12): (0, 0, 0).
 * A pixel shows the last operation covering it in the order (p, operation); untouched pixels keep the input.  show_txt
 * == 0 (or L == 0) drops 4 and 5 (label_codes and atlas may then be null), show_polygons == 0 drops 1 and 2.  An
 * instance whose polygon has a coordinate beyond +-2^29 contributes 3, 4 and 5 only (no defined drawing that far out).  With n > 128 nothing is drawn (out =
 * image): n is on the device, the caller refuses it when it reads n.  Integer arithmetic, the same bits on every run.
 * R <= 1024, 3 <= N <= 64, C <= 32, L <= 16, G <= 128, H * W < 2^31, outline_radius <= 16: beyond, CP_EUNSUPPORTED;
 * null pointers, alpha outside 0..256, a negative radius or thickness: CP_EINVAL; workspace shorter than
 * cp_render_overlay_workspace_bytes (the per-pixel operation map, 4 bytes a pixel): CP_EWORKSPACE.  All checks come
 * before any device work.  One memset and two launches whatever n is.
 *
 * cp_render_heatmap: the reference's gen_colormap + add_blend_img (utils/debugger.py) in one launch:
 *   cm[k] = max over c of uint8(hm[c][y / ratio][x / ratio] * palette[c % P][k]) (an fp32 product, truncated),
 *   255 - cm under `white`; back[k] = uint8((input[k][y][x] * std[k] + mean[k]) * 255), every step rounded to fp32,
 *   kept in 0..255; out[y][x][k] = (back * 77 + cm * 179 + 128) >> 8.
 *   hm  DEVICE fp32 [C][h][w], activated      input  DEVICE fp32 [3][h * ratio][w * ratio]      mean, std  HOST fp32 [3]
 *   palette  DEVICE uint8 [P][3], P <= 32     out    DEVICE uint8 [h * ratio][w * ratio][3]
 * C == 0 (hm may be null) writes out = back, the de-normalised network input alone. */
typedef struct cp_overlay_params {
  int32_t alpha;              /* 0 .. 256, weight of the class colour in the fill */
  int32_t outline_radius;     /* r */
  int32_t box_thickness;      /* t */
  int32_t white_theme;
  int32_t show_txt;           /* 0 drops operations 4 and 5 */
  int32_t show_polygons;      /* 0 drops operations 1 and 2 (boxes and labels alone) */
  uint8_t outline_colour[3];  /* in the image's channel order */
  uint8_t reserved;
} cp_overlay_params;
size_t cp_render_overlay_workspace_bytes(int32_t H, int32_t W);
int cp_render_overlay(const uint8_t* image, int32_t H, int32_t W, const float* rows, int32_t R, int32_t N,
                      const int32_t* n, const int32_t* src, const int32_t* poly, const uint8_t* palette, int32_t C,
                      const int32_t* label_codes, int32_t L, const uint8_t* atlas, int32_t G,
                      const cp_overlay_params* params, uint8_t* out, void* workspace, size_t workspace_bytes,
                      void* stream);
int cp_render_heatmap(const float* hm, int32_t C, int32_t h, int32_t w, int32_t ratio, const float* input,
                      const float* mean, const float* stdv, const uint8_t* palette, int32_t P, int32_t white,
                      uint8_t* out, void* stream);

/* ------------------------------------------------ ground-truth head maps (--eval_oracle_*) --
 * cp_oracle_map: the reference's gen_oracle_map (src/lib/utils/oracle_utils.py), a 4-neighbour breadth-first flood
 * fill from the objects' centres over the whole map, in its closed form and in one launch:
 *   feat  DEVICE fp32 [B][M][D]       ind  DEVICE int64 [B][M], flat index y * w + x of object j's centre
 *   out   DEVICE fp32 [B][D][h][w], every element written (no need to clear it)
 * Per image, object j is a seed when ind[j] > 0 -- not reg_mask: padding rows are skipped, and so is a real object
 * whose centre is flat index 0, as in the reference.  Then
 *   out[b][:][y][x] = feat[b][j*][:], j* = the LOWEST j among the seeds at minimal |x - x_j| + |y - y_j|
 * (the BFS level of a pixel is its L1 distance to the nearest seed, and the queue keeps each level in seed order),
 * with one exception: at a seed's own pixel the HIGHEST j with that ind wins (later duplicates overwrite the pixel,
 * the earlier one expands first).  An image without a seed is all zeros.  The values are copies: bit-exact.
 * ind[j] >= h * w: the reference indexes out of bounds there and defines nothing; here such an object is skipped like
 * ind <= 0.  This is the one place where the reference leaves the result open.
 * M <= 1024, B <= 65535, h * w < 2^31 (CP_EUNSUPPORTED beyond); any D (a loop over channels), any h and w, any
 * alignment (16-byte stores where w % 4 == 0 and out is 16-byte aligned).  Null pointers or non-positive sizes:
 * CP_EINVAL.  All checks come before any device work. */
int cp_oracle_map(const float* feat, const int64_t* ind, int32_t B, int32_t M, int32_t D, int32_t h, int32_t w,
                  float* out, void* stream);

/* ------------------------------------------------ detector pre/post-processing --
 * cp_preprocess_warp_normalize: the cv2 stage of BaseDetector.pre_process
 * (src/lib/detectors/base_detector.py:66-87): cv2.warpAffine(image, trans_input, (dst_w, dst_h),
 * flags=INTER_LINEAR) on the 8-bit image followed by ((x / 255. - mean) / std) and the HWC -> CHW
 * transpose; OpenCV's fixed-point arithmetic, bit-identical to oracle/pre.py.
 *   src   DEVICE uint8 [src_h][src_w][3]      trans  HOST float64[6], forward map src -> dst
 *   mean, std  HOST float32[3]                out    DEVICE fp32 [1 + flip_copy][3][dst_h][dst_w]
 * flip_copy != 0 also writes the horizontally flipped image behind it (--flip_test, :84-85).
 *
 * cp_polydet_post_process: transform_preds of polydet_post_process
 * (src/lib/utils/post_process.py:105-122, src/lib/utils/image.py:19-24) + the `/ scale` of
 * PolydetDetector.post_process (src/lib/detectors/polydet.py:52-57) on the decoded rows
 *   dets [B][K][ncols] (ncols = 2N + 7: x1,y1,x2,y2,score,class, N vertices, depth), DEVICE
 *   trans_dev  DEVICE float64 [B][6]: inverse affine (output map -> image) per image
 * Box corners and vertices are mapped in float64, cast to fp32, divided by `scale`; the other
 * columns are copied.  out has the layout of dets (out == dets is NOT allowed). */
int cp_preprocess_warp_normalize(const uint8_t* src, int32_t src_h, int32_t src_w,
                                 const double* trans, const float* mean, const float* stdv,
                                 int32_t dst_h, int32_t dst_w, int32_t flip_copy, float* out,
                                 void* stream);

/* cp_preprocess_warp_normalize_batch: cp_preprocess_warp_normalize for B source images of different sizes in one
 * launch per 16 images (BaseDetector.run_batch; added without an ABI version change).
 *   images        DEVICE uint8: the B sources back to back, each [H_b][W_b][3]
 *   image_offset  HOST int64 [B]: byte offset of image b in `images`      image_hw  HOST int32 [B][2]: (H_b, W_b)
 *   trans         HOST float64 [B][6]: forward map source -> dst per image       mean, stdv  HOST float32[3]
 *   out           DEVICE fp32 [(1 + flip_copy) * B][3][dst_h][dst_w], every element written
 * Image b is at index b of `out`, its horizontally flipped copy (flip_copy != 0) at index B + b: all originals, then
 * all flips.  Both equal, bit for bit, the two images cp_preprocess_warp_normalize writes for that source and map.
 * The per-image parameters travel in the kernel arguments (no copy inside the call); `images` must hold every
 * [offset_b, offset_b + 3 H_b W_b) -- the library cannot see its length.
 * H_b or W_b > 32767 or dst_h > 65535: CP_EUNSUPPORTED.  Null pointers, batch <= 0, a non-positive size or a negative
 * offset: CP_EINVAL.  All checks come before any device work. */
int cp_preprocess_warp_normalize_batch(const uint8_t* images, const int64_t* image_offset, const int32_t* image_hw,
                                       const double* trans, const float* mean, const float* stdv, int32_t batch,
                                       int32_t dst_h, int32_t dst_w, int32_t flip_copy, float* out, void* stream);

/* cp_color_aug_normalize: the colour augmentation + normalisation of the TRAINING sampler
 * (src/lib/datasets/sample/polydet.py:128-136: `inp / 255.` -> color_aug -> `(inp - mean) / std`;
 * src/lib/utils/image.py:231-264) in place on the warped input, BGR planes [3][HW] holding x / 255
 * (cp_preprocess_warp_normalize with mean 0 / std 1).  The random draws stay with the caller
 * (reference: data_rng + random.shuffle in the loader worker): order[3] = the three ops in
 * application order (0 brightness, 1 contrast, 2 saturation), alpha[3] their blend factors,
 * light[3] = eig_vec . (eig_val * alpha_pca) per BGR channel (float64).  color_on == 0 only
 * normalises.  All HOST pointers except img / workspace (cp_color_aug_workspace_bytes). */
size_t cp_color_aug_workspace_bytes(void);
int cp_color_aug_normalize(float* img, int64_t HW, int32_t color_on, const int32_t* order,
                           const float* alpha, const double* light, const float* mean, const float* stdv,
                           void* workspace, size_t workspace_bytes, void* stream);
int cp_polydet_post_process(const float* dets, const double* trans_dev, float scale, int32_t B,
                            int32_t K, int32_t ncols, float* out, void* stream);

/* cp_sample_inputs_batch: the image path of the TRAINING sampler for a whole batch whose source images differ in
 * size (src/lib/datasets/sample/polydet.py:106-136: cv2.warpAffine to input_w x input_h -> `inp / 255.` -> color_aug
 * -> `(inp - mean) / std` -> CHW; src/lib/utils/image.py:231-264).  The reference warps on the host so that its
 * collate sees equal shapes; here the 8-bit sources arrive back to back and the dense batch is formed on the device.
 *   images        DEVICE uint8: the B source images back to back, each [H_b][W_b][3] BGR (already mirrored where flipped)
 *   image_offset  HOST int64 [B]: byte offset of image b in `images` (64-bit addressing throughout)
 *   image_hw      HOST int32 [B][2]: (H_b, W_b)
 *   trans_input   HOST float64 [B][6]: forward affine source -> network input, inverted in float64 as cv::warpAffine does
 *   color         HOST float64 [B][10]: [on, order x3, alpha x3, light x3], the sampler's row: order = the three ops in
 *                 application order (0 brightness, 1 contrast, 2 saturation), alpha their blend factors (rounded to
 *                 float32), light = eig_vec . (eig_val * alpha_pca) per BGR channel.  on == 0: the row is not read
 *                 further and the image is only normalised
 *   mean, stdv    HOST float32[3]              out  DEVICE fp32 [B][3][dst_h][dst_w], every element written
 * Image b of `out` equals, operation for operation, cp_preprocess_warp_normalize(mean 0, std 1) followed by
 * cp_color_aug_normalize on that image alone: OpenCV's fixed-point 8-bit warp (border 0), x / 255 in float64 cast to
 * fp32, the grey-level mean over the image's own dst_h x dst_w pixels in float64, the float32 colour chain, the
 * lighting add in float64, (x - mean) / std in float32.  Only the summation order of the grey mean differs; it is
 * fixed (no floating-point atomics), so a call repeats its bits and an image's result does not depend on its batch.
 * Two launches per 16 images; the per-image parameters travel in the kernel arguments (no copy inside the call).
 * H_b or W_b > 32767 or dst_h > 65535: CP_EUNSUPPORTED.  Null pointers, batch <= 0, a non-positive size, a negative
 * offset, an order entry outside {0, 1, 2} on a colour-on row, or workspace_bytes below
 * cp_sample_inputs_workspace_bytes(batch, dst_h, dst_w): CP_EINVAL.  All checks come before any device work. */
size_t cp_sample_inputs_workspace_bytes(int32_t batch, int32_t dst_h, int32_t dst_w);
int cp_sample_inputs_batch(const uint8_t* images, const int64_t* image_offset, const int32_t* image_hw,
                           const double* trans_input, const double* color, const float* mean, const float* stdv,
                           int32_t batch, int32_t dst_h, int32_t dst_w, float* out, void* workspace,
                           size_t workspace_bytes, void* stream);

/* soft_nms of external/nms.pyx:77-170 (Cython in the reference) on HOST float32 rows
 * [n][row_stride] (x1,y1,x2,y2,score,...), in place, as merge_outputs uses it
 * (src/lib/detectors/polydet.py:66-67: Nt=0.5, method=2).  method 0 hard / 1 linear /
 * 2 gaussian.  Only columns 0-4 move; returns the live row count N (>= 0) or CP_EINVAL. */
int cp_soft_nms(float* boxes_host, int32_t n, int32_t row_stride, float sigma, float Nt,
                float threshold, int32_t method);

/* cp_soft_nms_device: cp_soft_nms on DEVICE rows, n_seg independent problems in one call (csrc/merge_nms.hip).
 *   rows       DEVICE fp32, rows of row_stride floats (x1,y1,x2,y2,score,...); only columns 0-4 are read and written
 *   seg_start, seg_len   DEVICE int32 [n_seg]: segment s is rows [seg_start[s], seg_start[s] + seg_len[s])
 *   live_out   DEVICE int32 [n_seg]: what cp_soft_nms returns for the segment
 * Every segment equals, bit for bit, cp_soft_nms on a host copy of it -- the slots at and above the live count
 * included: a row that fills a hole decays at its new position, so the stale copy it leaves at the end of the live
 * range keeps its UNDECAYED score (only a row discarded in the last live slot keeps the decayed one).  The double exp
 * of method 2 is the device library's; its result is rounded to float.  A segment of length 0 (or below) leaves nothing
 * written but live_out[s] = 0; the segments must not overlap.  One launch, one 64-lane wave per segment.
 * row_stride >= 5 and n_seg <= 64, otherwise CP_EUNSUPPORTED; null pointers, a negative n_seg or row_stride, a method
 * outside 0..2: CP_EINVAL; all checks come before any device work.  seg_len <= 4096: the lengths lie on the device, so
 * the call cannot refuse a longer one -- such a segment is left untouched and reported as live_out[s] = -1.
 *
 * cp_merge_detections: PolydetDetector.merge_outputs (src/lib/detectors/polydet.py:62-76) with its soft_nms
 * (external/nms.pyx:77-170) on the DEVICE rows of the S test scales, literal behaviour.
 *   rows    DEVICE fp32 [S][K][ncols]: what cp_polydet_post_process wrote for each scale (class in column 5)
 *   out     DEVICE fp32 [S * K][ncols]       counts  DEVICE int32 [1 + num_classes]: the total, then per class
 * out[0 : counts[0]] holds class 0's rows, then class 1's, ...; each row x1,y1,x2,y2,score,cls,poly...,depth -- the
 * reference's `results` with the class column put back.  Rows beyond counts[0] are not specified.  Per class the rows
 * of every scale in scale order, in row order; with nms != 0 soft_nms(sigma, Nt, threshold, method) in place on the
 * class block, of which only columns 0-4 move (polygon and depth stay in their slots), the live count is ignored and
 * the stale slots above it stay part of the block (see cp_soft_nms_device); when the blocks hold more than
 * max_per_image rows, each class keeps, in order, its rows with score >= the (total - max_per_image)-th smallest score
 * (np.partition; ties are kept, so counts[0] may exceed max_per_image).  A class value that equals no integer of
 * [0, num_classes) drops its row.  Scores are assumed finite: with a NaN score the call terminates and stays inside
 * its buffers, but its result is unspecified.
 * Three launches (two with nms == 0): partition by class, soft-NMS with one wave per class, cut.  No atomics: a call
 * repeats its bits.  S * K <= 4096, num_classes <= 64, ncols >= 7, otherwise CP_EUNSUPPORTED; null pointers,
 * non-positive sizes, max_per_image < 1, a method outside 0..2, out == rows, or workspace_bytes below
 * cp_merge_detections_workspace_bytes(S, K, ncols, num_classes) (the class-sorted rows and the segment table; 0 for an
 * unsupported shape): CP_EINVAL.  All checks come before any device work. */
int cp_soft_nms_device(float* rows, int32_t row_stride, const int32_t* seg_start, const int32_t* seg_len,
                       int32_t n_seg, float sigma, float Nt, float threshold, int32_t method, int32_t* live_out,
                       void* stream);
size_t cp_merge_detections_workspace_bytes(int32_t S, int32_t K, int32_t ncols, int32_t num_classes);
int cp_merge_detections(const float* rows, int32_t S, int32_t K, int32_t ncols, int32_t num_classes,
                        int32_t max_per_image, int32_t nms, float sigma, float Nt, float threshold, int32_t method,
                        float* out, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------ mask NMS (--mask_nms) --
 * The merge above is the reference's, literally: after it a box and its score sit in a row whose polygon and depth
 * belong to another detection, and the overlap that drives the decay is the box IoU.  The two entry points below
 * (csrc/mask_nms.hip) are the merge whose output can be used.  The definition is this project's own, not the
 * reference's:
 *   candidates  the rows [S][K][ncols] of all scales, scale by scale and row by row, ncols = 2 N + 7
 *               (x1,y1,x2,y2,score,cls,poly(2N),depth); a row takes part when its class equals an integer of
 *               [0, num_classes), the rule of cp_merge_detections.  A row's POSITION is its index in that order within
 *               its class.
 *   mask        F of a row: the pixels ImageDraw.polygon(pts, fill=1) sets on an H x W 'L' image (PIL's scan-line
 *               fill: csrc/class_masks_core.h, fitted against PIL 12.2), the vertices int(float("%.2f" % v)) as the
 *               result writers use, clipped to the canvas; no outline pass, no dilation, no occlusion, the same for
 *               every data set.
 *   overlap     of two candidates of one class: inter = |F_i & F_j|, uni = |F_i| + |F_j| - inter,
 *               ov = (double)inter / (double)uni, 0 when uni == 0.
 *   selection   per class: take the live candidate with the largest score, the lowest position on a tie; if its score
 *               is below `threshold` the class stops and all its remaining rows are dropped; otherwise it moves to the
 *               output and every remaining live candidate p decays once, score_p = (float)(w * (double)score_p) with w
 *               in double: method 0 (hard) w = ov > Nt ? 0 : 1; 1 (linear) w = ov > Nt ? 1 - ov : 1; 2 (gaussian)
 *               w = exp(-(ov * ov) / sigma) (the device library's double exp).  A pair with inter == 0 is left
 *               untouched.
 *   cut         merge_outputs' rule on the kept rows of all classes: with more than max_per_image of them, those with
 *               score >= the (total - max_per_image)-th smallest stay (ties are kept).
 *   output      the layout of cp_merge_detections: out[0 : counts[0]] class by class, counts [1 + num_classes]; within
 *               a class the rows in selection order.  Every column of a row is copied from its ONE source row, except
 *               that column 4 holds the final score.  There are no stale slots; rows beyond counts[0] are not
 *               specified.  Scores are assumed finite: with a NaN score the call terminates inside its buffers and its
 *               result is unspecified.
 *
 * cp_polygon_overlaps: the masks' pixel counts of R DEVICE rows [R][ncols] on an H x W canvas.
 *   area   DEVICE int32 [R]: |F_i| (0 for a row without a class)
 *   inter  DEVICE int32 [R][R]: |F_i & F_j|; inter[i][i] == area[i], the matrix is symmetric, and it holds 0 for pairs
 *          of different class and for rows without a class.  Integers: a call repeats its bits.
 * Two memsets and three launches: the classes and the clipped boxes (one workgroup), the raster (one wave per row and
 * image row, the spans ORed into a bit plane per candidate of ceil(W / 32) words a row, only the words of the
 * candidate's own box written), the pairs (one wave per pair of one class whose boxes intersect: popcount(A & B) over
 * the intersection of the boxes).  Workspace: R bit planes plus tables, cp_polygon_overlaps_workspace_bytes(R, ncols,
 * H, W) (0 for a refused shape); 16-byte aligned.
 *
 * cp_merge_detections_mask: the signature of cp_merge_detections plus the canvas H, W.  The class split, the overlaps,
 * the selection (one wave per class) and the cut: one memset and five launches whatever S * K is, nothing allocated.
 * With nms == 0 no mask is drawn and no row decays or is dropped: each class by descending score, then the cut.
 * Workspace: the planes, the matrix and tables, cp_merge_detections_mask_workspace_bytes(S, K, ncols, num_classes, H,
 * W) -- 64 MiB at S * K = 256 on 2048 x 1024, 256 MiB at 1024 rows; only box-sized parts of the planes are touched.
 *
 * Both: R = S * K <= 1024, N = (ncols - 7) / 2 <= 64, num_classes <= 64, H * W < 2^31, otherwise CP_EUNSUPPORTED; null
 * pointers, non-positive sizes, ncols even or below 13 (N < 3), max_per_image < 1, a method outside 0..2, out == rows,
 * a workspace that is not 16-byte aligned: CP_EINVAL; a short workspace: CP_EWORKSPACE.  All checks come before any
 * device work. */
size_t cp_polygon_overlaps_workspace_bytes(int32_t R, int32_t ncols, int32_t H, int32_t W);
int cp_polygon_overlaps(const float* rows, int32_t R, int32_t ncols, int32_t num_classes, int32_t H, int32_t W,
                        int32_t* area, int32_t* inter, void* workspace, size_t workspace_bytes, void* stream);
size_t cp_merge_detections_mask_workspace_bytes(int32_t S, int32_t K, int32_t ncols, int32_t num_classes, int32_t H,
                                                int32_t W);
int cp_merge_detections_mask(const float* rows, int32_t S, int32_t K, int32_t ncols, int32_t num_classes,
                             int32_t max_per_image, int32_t nms, float sigma, float Nt, float threshold, int32_t method,
                             int32_t H, int32_t W, float* out, int32_t* counts, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ------------------------------------------------- training-target construction --
 * The per-object loop of PolydetDataset.__getitem__ (src/lib/datasets/sample/polydet.py:160-405)
 * with affine_transform / gaussian_radius / draw_umich_gaussian (src/lib/utils/image.py:62-65,
 * 95-141): raw annotations of a batch -> the tensors of the batch dict (:425-449).
 * Inputs (all DEVICE): bbox_xywh f64 [B][M][4] COCO boxes, poly_xy f64 [B][M][2N] vertices in
 * image coordinates, cls_id i32 [B][M], pseudo_depth_in f32 [B][M], class_freq f32 [B][M] (the
 * object's class frequency), num_objs i32 [B] (slots >= num_objs stay zero), flipped u8 [B],
 * img_width i32 [B] (mirror axis), trans_output f64 [B][6] (get_affine_transform(c, s, 0,
 * [out_w, out_h])).  Outputs (DEVICE, fully written): hm f32 [B][C][h][w], border_hm f32
 * [B][1][h][w] or NULL, reg_mask u8 [B][M], ind i64 [B][M], poly f32 [B][M][2N], pseudo_depth
 * f32 [B][M][1], peak / reg / wh f32 [B][M][2], freq_mask f32 [B] (mean over the image's
 * objects, 1 when none).  rep: CP_REP_* (polar targets are (r, theta) pairs). */
typedef struct cp_target_shape {
  int32_t B, max_objs, nbr_points, num_classes, out_h, out_w, rep, no_reorder_flip;
} cp_target_shape;
size_t cp_polydet_targets_workspace_bytes(const cp_target_shape* s);
int cp_polydet_targets(const cp_target_shape* s, const double* bbox_xywh, const double* poly_xy,
                       const int32_t* cls_id, const float* pseudo_depth_in, const float* class_freq,
                       const int32_t* num_objs, const uint8_t* flipped, const int32_t* img_width,
                       const double* trans_output, float* hm, float* border_hm, uint8_t* reg_mask,
                       int64_t* ind, float* poly, float* pseudo_depth, float* peak, float* reg,
                       float* wh, float* freq_mask, void* workspace, size_t workspace_bytes,
                       void* stream);

/* Centre heat map of cp_polydet_targets_ex (`--elliptical_gt`, src/lib/datasets/sample/polydet.py:156-159,223-228,
 * src/lib/utils/image.py:144-173).
 *   CP_HEATMAP_UMICH    draw_umich_gaussian: the (2r+1)^2 Gaussian, sigma = (2r+1)/6, values below DBL_EPSILON cut
 *                       to 0.  What cp_polydet_targets draws (it is this mode of the same implementation).
 *   CP_HEATMAP_ELLIPSE  draw_ellipse_gaussian into hm[class] with radius_x = r if h > w else int(r * (w / h)),
 *                       radius_y = r if w >= h else int(r * (h / w)) (h, w: the float32 box sides after the affine
 *                       and the clip; ratio and product in float32, then truncated).  Window (2ry+1) x (2rx+1) around
 *                       the centre, clipped like the UMich one; at row offset dy, column offset dx the value is
 *                       exp(-((dy*mr)^2 + (dx*mc)^2) / (2 sigma^2)) in float64 with mr = (2rx+1) / m,
 *                       mc = (2ry+1) / m, m = max(2rx+1, 2ry+1), sigma = (2 min(rx, ry) + 1) / 6, no epsilon cut,
 *                       max-composited into the float32 map.  border_hm keeps the UMich splats of radius r, and the
 *                       ownership test of cp_polydet_dense_targets keeps the UMich Gaussian and window of radius r
 *                       (draw_dense_reg), against the class maximum of the elliptical map.  Every other output is
 *                       the UMich call's, bit for bit.
 * The mode is recorded in the workspace, so cp_polydet_dense_targets follows it without an argument of its own. */
enum { CP_HEATMAP_UMICH = 0, CP_HEATMAP_ELLIPSE = 1 };
/* cp_polydet_targets with a centre heat map of `heatmap` (CP_HEATMAP_*; any other value: CP_EINVAL before any device
 * work).  Same arguments, outputs and workspace as cp_polydet_targets. */
int cp_polydet_targets_ex(const cp_target_shape* s, int32_t heatmap, const double* bbox_xywh, const double* poly_xy,
                          const int32_t* cls_id, const float* pseudo_depth_in, const float* class_freq,
                          const int32_t* num_objs, const uint8_t* flipped, const int32_t* img_width,
                          const double* trans_output, float* hm, float* border_hm, uint8_t* reg_mask,
                          int64_t* ind, float* poly, float* pseudo_depth, float* peak, float* reg,
                          float* wh, float* freq_mask, void* workspace, size_t workspace_bytes,
                          void* stream);

/* `--dense_poly` targets (src/lib/datasets/sample/polydet.py:401-403,429-441 with draw_dense_reg,
 * src/lib/utils/image.py:176-204): after cp_polydet_targets on the SAME shape and workspace (its per-object
 * descriptors are read from it), dense_poly [B][2N][h][w] holds, per pixel, the polygon row of the LAST object k (in
 * annotation order) whose Gaussian there is >= the class-maximum heat map as it stood after drawing objects 0..k
 * (the comparison the reference makes: float64 Gaussian against the float32 map), 0 where no object qualifies;
 * dense_mask [B][2N][h][w] = (dense_poly != 0) as 0 / 1 floats.  poly = cp_polydet_targets' poly output. */
int cp_polydet_dense_targets(const cp_target_shape* s, const float* poly, const void* workspace,
                             size_t workspace_bytes, float* dense_poly, float* dense_mask, void* stream);

/* --------------------------- fused training BatchNorm2d (+residual) (+ReLU) --
 * y = act(bn(x) + residual) with batch statistics (torch.nn.BatchNorm2d training semantics:
 * biased variance for normalisation, running stats updated with `momentum`, unbiased variance).
 * Replaces the BN -> add -> ReLU chains of DeformConv / BasicBlock / Root / conv levels
 * (src/lib/models/networks/pose_dla_dcn.py:32-60,148-166,266-277,347-359) in training.
 * x, y, residual and their gradients: fp32 [B,C,H,W], HW = H x W; weight, bias, running and
 * saved statistics: [C].  backward: grad_weight / grad_bias are OVERWRITTEN; grad_residual (may be NULL) receives
 * the post-activation gradient; workspace from cp_bn_workspace_bytes.  `bias` is the forward's bias (NULL if it had none);
 * with relu and NO residual in the forward, pass y = NULL: the ReLU mask [y > 0] is then recomputed from x (the forward's
 * own expression, bit-identical) and y is not read -- a third less traffic (y = NULL with grad_residual: CP_EINVAL). */
size_t cp_bn_workspace_bytes(int32_t B, int32_t C, int64_t HW);
int cp_bn_act_forward_train(const float* x, const float* weight, const float* bias,
                            const float* residual, float* y, float* save_mean, float* save_invstd,
                            float* running_mean, float* running_var, float momentum, float eps,
                            int32_t relu, int32_t B, int32_t C, int64_t HW, void* workspace,
                            size_t workspace_bytes, void* stream);
int cp_bn_act_backward(const float* x, const float* y, const float* grad_y, const float* weight, const float* bias,
                       const float* save_mean, const float* save_invstd, int32_t relu, float* grad_x,
                       float* grad_residual, float* grad_weight, float* grad_bias, int32_t B,
                       int32_t C, int64_t HW, void* workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------- decode --
 * heat [B,C,H,W] (already activated), polys [B,2N,H,W], depth [B,1,H,W],
 * reg [B,2,H,W] or NULL (then +0.5).  K <= 256 and N2 = 2N <= 128 (64 vertices, the
 * limit of the writers, mask kernels and renderer), in any combination: the winners'
 * polygon rows [K][N2] are staged in up to 128 KB of the CU's 160 KB of LDS.  Beyond
 * either limit, for cp_polydet_decode and cp_polydet_decode_ex alike: CP_EUNSUPPORTED.
 * Outputs: dets [B,K,2N+7] = [x1,y1,x2,y2,score,cls,poly(2N),depth],
 * inds [B,K] int64 (flat y*W+x), clses [B,K] int32 (both may be NULL).
 * Selection order: score descending, ties by (class, flat index) ascending --
 * the order a stable sort of the reference's two-level top-k yields.
 */
size_t cp_polydet_decode_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t K);
int cp_polydet_decode(const float* heat, const float* polys, const float* depth, const float* reg,
                      int32_t B, int32_t C, int32_t H, int32_t W, int32_t N2, int32_t K,
                      int32_t rep, float* dets, int64_t* inds, int32_t* clses, void* workspace,
                      size_t workspace_bytes, void* stream);
/* `--cat_spec_poly` (src/lib/models/decode.py:534-537): polys is [B, C * N2, H, W], one polygon of N2 numbers per
 * class, and a detection of class c takes channels c * N2 .. c * N2 + N2 - 1 (`polys.view(batch, K, cat,
 * nbr_points).gather(2, clses)`).  cat_spec_poly = 0 is cp_polydet_decode.  (The reference takes `nbr_points` from
 * `polys.shape[-1]` of the MAP, i.e. its width: its view only succeeds when C * W equals the channel count -- the
 * Python mirror keeps that precondition, the kernel does not need it.) */
int cp_polydet_decode_ex(const float* heat, const float* polys, const float* depth, const float* reg,
                         int32_t B, int32_t C, int32_t H, int32_t W, int32_t N2, int32_t K,
                         int32_t rep, int32_t cat_spec_poly, float* dets, int64_t* inds, int32_t* clses,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------- focal loss --
 * forward: hm[n] <- clamp(sigmoid(hm[n]), 1e-4, 1-1e-4) IN PLACE (the reference
 * mutates output['hm'] the same way) and loss_out[0] <- CornerNet focal loss;
 * stats_out[0..2] <- {sum pos term, sum neg term, num_pos} (device floats).
 * backward: grad_logits[n] <- grad_loss[0] * dLoss/dlogit from the ACTIVATED hm.
 */
size_t cp_sigmoid_focal_workspace_bytes(int64_t n);
int cp_sigmoid_focal_forward(float* hm_inout, const float* gt, int64_t n, float* loss_out,
                             float* stats_out, void* workspace, size_t workspace_bytes,
                             void* stream);
int cp_sigmoid_focal_backward(const float* hm_act, const float* gt, int64_t n,
                              const float* stats, const float* grad_loss, float* grad_logits,
                              void* stream);

/* ----------------------------------------------------- gathered L1 losses --
 * feat [B,D,H,W]; ind [B,M] int64; mask [B,M] uint8; target [B,M,D].
 * pred[b,m,d] = feat[b,d,ind[b,m]] (no NHWC copy).
 * loss_out[0] = S / (sum(mask)*D + eps), S by `mode` (CP_L1_*).
 * pred_add [B,M,D] or NULL: constant added to pred before the loss (the order
 * term's in-place `angles += 2*3.14`, src/lib/models/losses.py:892-899).
 * backward scatter-ADDS grad_loss[0] * dS/dfeat / denom into grad_feat (caller zero-fills).
 */
int cp_gather_l1_forward(const float* feat, const int64_t* ind, const uint8_t* mask,
                         const float* target, const float* pred_add, int32_t B, int32_t D,
                         int32_t H, int32_t W, int32_t M, int32_t mode, float eps,
                         float* loss_out, void* stream);
int cp_gather_l1_backward(const float* feat, const int64_t* ind, const uint8_t* mask,
                          const float* target, const float* pred_add, int32_t B, int32_t D,
                          int32_t H, int32_t W, int32_t M, int32_t mode, float eps,
                          const float* grad_loss, float* grad_feat, void* stream);

/* `--mse_loss` (src/lib/trains/polydet.py:23,44-46,84): torch.nn.MSELoss() between the RAW heat-map head (no
 * sigmoid) and the target, loss = mean((x - gt)^2); backward grad_x = 2 (x - gt) / n * grad_loss[0]. */
size_t cp_mse_workspace_bytes(void);
int cp_mse_forward(const float* x, const float* gt, int64_t n, float* loss_out, void* workspace,
                   size_t workspace_bytes, void* stream);
int cp_mse_backward(const float* x, const float* gt, int64_t n, const float* grad_loss, float* grad_x,
                    void* stream);

/* `--dense_poly` loss (src/lib/trains/polydet.py:107-110): torch.nn.L1Loss(reduction='sum')(pred * mask, target * mask)
 * / (mask.sum() + eps) over whole maps of n elements.  forward: out2[0] = loss, out2[1] = mask.sum() + eps (the
 * denominator the backward needs); backward: grad_pred = sign(pred * mask - target * mask) * mask * grad_loss[0] / den[0]. */
size_t cp_dense_l1_workspace_bytes(void);
int cp_dense_l1_forward(const float* pred, const float* target, const float* mask, int64_t n, float eps, float* out2,
                        void* workspace, size_t workspace_bytes, void* stream);
int cp_dense_l1_backward(const float* pred, const float* target, const float* mask, int64_t n, const float* den,
                         const float* grad_loss, float* grad_pred, void* stream);

/* ----------------------------------- polygon IoU (Weiler-Atherton) + order --
 * feat = polygon head [B,2N,H,W]; per masked object the literal reference
 * computation (every point read as (r, theta), doubled first shoelace term,
 * early-terminating traversal).  flags: bit0 = IoU term, bit1 = order term.
 *   iou_loss_out[0]   = 1 - sum(iou) / (sum(mask) + 1e-6)          (bit0)
 *   order_loss_out[0] = sum(hinge) / (10*sum(mask) + 1e-4)         (bit1)
 *   pred_add_out [B,M,2N] (bit1): the +2*3.14 edits, to feed cp_gather_l1_*.  Only the angle slots (odd) of the
 *   masked objects are written -- the caller zero-fills it; the two losses are overwritten.
 * backward scatter-ADDS into grad_feat (caller zero-fills).  The forward takes a workspace of arbitrary contents and
 * leaves the object count in it; the backward READS that count, so it is handed the forward's workspace, unchanged.
 */
size_t cp_poly_iou_order_workspace_bytes(int32_t B, int32_t M, int32_t N);
int cp_poly_iou_order_forward(const float* feat, const int64_t* ind, const uint8_t* mask,
                              const float* target, int32_t B, int32_t N, int32_t H, int32_t W,
                              int32_t M, int32_t flags, float* iou_loss_out,
                              float* order_loss_out, float* pred_add_out, void* workspace,
                              size_t workspace_bytes, void* stream);
int cp_poly_iou_order_backward(const float* feat, const int64_t* ind, const uint8_t* mask,
                               const float* target, int32_t B, int32_t N, int32_t H, int32_t W,
                               int32_t M, int32_t flags, const float* grad_iou_loss,
                               const float* grad_order_loss, float* grad_feat, void* workspace,
                               size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CENTERPOLY_HIP_H */
