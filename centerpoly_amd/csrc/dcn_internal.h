// Internal interface between the DCNv2 translation units (not part of the C ABI).
#pragma once
#include "cp_common.h"

// output extent of the 3x3 kernel along one axis
static inline int out_extent(int in, int pad, int dil, int stride) {
  return (in + 2 * pad - (dil * 2 + 1)) / stride + 1;
}

// N elements of one channel of a K-split DCN output from its slices: per element the slices' raw sums added to 0 in slice
// order, then the epilogue act(v * sc + sh).  p[k] = element k in slice 0, stride = elements between two slices.
// dcn_splitk_reduce_kernel (dcn_fwd.hip) and the up-sample kernels that read the slices themselves (upsample.hip) both
// go through this one expression, so a map is the same bits whichever of them forms it.  Eight (then four) slices' loads are issued
// before their adds (a load-wait-add loop costs a full memory latency per slice); the order of the adds is untouched.
// U slices' loads of N elements issued before their adds, which stay in slice order
template <int N, int U>
__device__ __forceinline__ void cp_dcn_slices_block(const float* (&p)[N], long long stride, int sidx, float (&v)[N]) {
  float t[U][N];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int k = 0; k < N; ++k) t[u][k] = p[k][(long long)(sidx + u) * stride];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] += t[u][k];
}

template <int N>
__device__ inline void cp_dcn_slices_values(const float* (&p)[N], long long stride, int nslices, float sc, float sh,
                                            int relu, float (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = 0.f;
  int sidx = 0;
  for (; sidx + 8 <= nslices; sidx += 8) cp_dcn_slices_block<N, 8>(p, stride, sidx, v);
  if (sidx + 4 <= nslices) {
    cp_dcn_slices_block<N, 4>(p, stride, sidx, v);
    sidx += 4;
  }
  for (; sidx < nslices; ++sidx) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] += p[k][(long long)sidx * stride];
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    v[k] = v[k] * sc + sh;
    if (relu) v[k] = cp_relu(v[k]);
  }
}

// region-sampling split-bf16 kernel (dcn_fwd_region.hip): 3x3, stride 1, pad 1, dilation 1, Cin % 16 == 0
bool cp_dcn_region_supported(const cp_dcn_shape* s);
size_t cp_dcn_region_wperm_bytes(const cp_dcn_shape* s);
int cp_dcn_region_prepare(const cp_dcn_shape* s, const float* weight, void* wp, hipStream_t st);
size_t cp_dcn_region_om_wperm_bytes(const cp_dcn_shape* s);
int cp_dcn_region_prepare_om(const cp_dcn_shape* s, const float* om_weight, void* wp, hipStream_t st);
// om_wp != null: conv_offset_mask fused into the kernel (offset / mask unused, om_out optional [B][27][H][W]).
// ksplit > 1 (never with om_wp): the input channels are split over grid z, the slices' RAW sums go to
// partial[ksplit'][B][Cout][H][W] (ksplit' = the slice count the launch really uses, cp_dcn_region_ksplit(s) when that
// was passed) and the caller reduces them and applies the epilogue.
int cp_dcn_region_ksplit(const cp_dcn_shape* s);
int cp_dcn_region_forward(const cp_dcn_shape* s, const float* x, const float* offset, int64_t offset_bstride,
                          const float* mask, int64_t mask_bstride, int32_t mask_is_logit, const void* wp,
                          const float* bias, const float* ep_scale, const float* ep_shift, int32_t relu, float* out,
                          const void* om_wp, const float* om_bias, float* om_out, float* partial, int ksplit,
                          hipStream_t st);

// dcn_bwd_data.hip: the register-resident grad-column kernel for the data gradients
bool cp_dcn_bwd_data2_supported(const cp_dcn_shape* s);
size_t cp_dcn_bwd_data2_workspace_bytes(const cp_dcn_shape* s);
int cp_dcn_bwd_data2(const cp_dcn_shape* s, const float* x, const float* offset, int64_t offset_bstride,
                     const float* mask, int64_t mask_bstride, int32_t mask_is_logit, const float* weight,
                     const float* grad_out, float* grad_x, float* grad_offset, int64_t grad_offset_bstride,
                     float* grad_mask, int64_t grad_mask_bstride, int32_t flags, void* workspace, size_t workspace_bytes,
                     hipStream_t st);

// dcn_bwd_weight.hip: the weight gradient with columns sampled straight into the MFMA operand
bool cp_dcn_bwd_weight2_supported(const cp_dcn_shape* s);
int cp_dcn_bwd_weight2(const cp_dcn_shape* s, const float* x, const float* offset, int64_t offset_bstride,
                       const float* mask, int64_t mask_bstride, int32_t mask_is_logit, const float* grad_out,
                       float* grad_weight, float* grad_bias, int32_t flags, hipStream_t st);
