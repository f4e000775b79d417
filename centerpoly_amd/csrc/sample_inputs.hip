// The image path of the training sampler for a whole batch of sources of DIFFERENT sizes.
//
// Replaces the host stage of PolydetDataset.__getitem__ (reference: src/lib/datasets/sample/polydet.py:106-136):
//     inp = cv2.warpAffine(img, trans_input, (input_w, input_h), flags=cv2.INTER_LINEAR)
//     inp = inp.astype(np.float32) / 255.
//     color_aug(self._data_rng, inp, self._eig_val, self._eig_vec)          (src/lib/utils/image.py:231-264)
//     inp = ((inp - self.mean) / self.std).transpose(2, 0, 1)
// which the reference runs per image so that default_collate sees equal shapes.  Here the 8-bit sources reach the
// device back to back in one ragged buffer and two launches build the dense [B][3][h][w] input:
//   (a) sample_warp_kernel    cv2's 8-bit warp (the arithmetic of preprocess_kernel, detector_io.hip) -> x / 255 into
//                             `out`, plus one float64 grey-level partial per workgroup for the colour-on images
//   (b) sample_color_kernel   sums the image's partials in a fixed order (no atomics: the same bits every call),
//                             then color_apply_kernel's float32 chain and the normalisation, in place
// The image index is blockIdx.z; the per-image parameters (inverse matrix, offset, size, colour row) travel by value
// in the kernel-argument struct, SI_CHUNK images per launch pair, so nothing is copied to the device inside the call.
//
// HBM-bound streaming.  Per OUTPUT pixel (a) writes 12 B and (b) reads and writes 12 B: 36 B, all plane accesses
// coalesced (lane = x); the per-image loop it replaces moves 72 B in 3 launches and one copy per image.  On top, in
// both paths, come the source bytes: 3 r B per output pixel inside the source, r = source pixels per output pixel
// (1 / scale^2: the 2x2 taps of neighbouring lanes share lines through L1, and below scale 1 their stride of 1 / scale
// still touches every line of the window).
#include "cp_common.h"

namespace {

constexpr int SI_CHUNK = 16;      // images per launch: 16 x (72 + 56) B of parameters stay far below the 4 KB of kernel arguments
constexpr int SI_ROWS = 4;        // output rows per workgroup of (a): one grey partial per 256 x 4 pixels
constexpr int SI_PIX = 4;         // pixels per thread of (b)

struct WarpImage {
  double m[6];                    // inverse map dst -> src
  long long offset;               // bytes from `images` to this source
  int sh, sw, color_on, pad;
};

struct WarpArgs {
  const uint8_t* images;
  float* out;                     // image 0 of the chunk
  double* part;                   // partials of image 0 of the chunk, nparts per image
  int dh, dw, nparts, nxb;
  WarpImage im[SI_CHUNK];
};

struct ColorImage {
  double light[3];
  float alpha[3];
  int order[3];
  int color_on, pad;
};

struct ColorArgs {
  float* out;
  const double* part;
  long long HW;
  int nparts;
  float mean[3], stdv[3];
  ColorImage im[SI_CHUNK];
};

__device__ __forceinline__ float grey_of(float b, float g, float r) {
  return __fadd_rn(__fadd_rn(__fmul_rn(b, 0.114f), __fmul_rn(g, 0.587f)), __fmul_rn(r, 0.299f));
}

__global__ __launch_bounds__(256) void sample_warp_kernel(WarpArgs a) {
  const int b = blockIdx.z;
  const WarpImage& p = a.im[b];
  const int x = blockIdx.x * 256 + threadIdx.x;
  const bool live = x < a.dw;                                  // dead lanes skip the rows and add 0 to the grey sum
  const uint8_t* src = a.images + p.offset;
  const long long plane = (long long)a.dh * a.dw;
  float* out = a.out + (long long)b * 3 * plane;
  const long long ax = cp_round_fix(__dmul_rn(p.m[0], (double)x));
  const long long bx = cp_round_fix(__dmul_rn(p.m[3], (double)x));
  double gsum = 0.0;
  const int y_end = min((int)(blockIdx.y + 1) * SI_ROWS, a.dh);
  for (int y = blockIdx.y * SI_ROWS; y < y_end && live; ++y) {
    // explicit rn ops: the compiler must not contract M1*y + M2 into an fma
    const long long X0 = cp_round_fix(__dadd_rn(__dmul_rn(p.m[1], (double)y), p.m[2])) + 16;
    const long long Y0 = cp_round_fix(__dadd_rn(__dmul_rn(p.m[4], (double)y), p.m[5])) + 16;
    const long long X = (X0 + ax) >> 5;
    const long long Y = (Y0 + bx) >> 5;
    const int sx = (int)min(max(X >> 5, -32768ll), 32767ll);   // saturate_cast<short>
    const int sy = (int)min(max(Y >> 5, -32768ll), 32767ll);
    const int fx = (int)(X & 31), fy = (int)(Y & 31);
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32;
    const int w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    const bool y0 = sy >= 0 && sy < p.sh, y1 = sy + 1 >= 0 && sy + 1 < p.sh;
    const bool x0 = sx >= 0 && sx < p.sw, x1 = sx + 1 >= 0 && sx + 1 < p.sw;
    const uint8_t* r0 = src + ((long long)(y0 ? sy : 0) * p.sw) * 3;
    const uint8_t* r1 = src + ((long long)(y1 ? sy + 1 : 0) * p.sw) * 3;
    const int c0 = (x0 ? sx : 0) * 3, c1 = (x1 ? sx + 1 : 0) * 3;
    float* o = out + (long long)y * a.dw + x;
    float f[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int p00 = (y0 && x0) ? r0[c0 + c] : 0, p01 = (y0 && x1) ? r0[c1 + c] : 0;
      const int p10 = (y1 && x0) ? r1[c0 + c] : 0, p11 = (y1 && x1) ? r1[c1 + c] : 0;
      const int v = (w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + (1 << 14)) >> 15;   // <= 255
      f[c] = (float)__ddiv_rn((double)v, 255.0);
      o[c * plane] = f[c];
    }
    gsum += (double)grey_of(f[0], f[1], f[2]);
  }
  if (!p.color_on) return;                                      // uniform over the workgroup
  gsum = cp_wave_sum_d(gsum);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = gsum;
  __syncthreads();
  if (threadIdx.x == 0)
    a.part[(long long)b * a.nparts + (long long)blockIdx.y * a.nxb + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void sample_color_kernel(ColorArgs a) {
  const int b = blockIdx.z;
  const ColorImage& p = a.im[b];
  __shared__ float s_mean;
  if (p.color_on) {
    const double* part = a.part + (long long)b * a.nparts;
    double s = 0.0;
    for (int i = threadIdx.x; i < a.nparts; i += 256) s += part[i];
    s = cp_wave_sum_d(s);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) s_mean = (float)((red[0] + red[1] + red[2] + red[3]) / (double)a.HW);
    __syncthreads();
  }
  float* img = a.out + (long long)b * 3 * a.HW;
  const long long base = (long long)blockIdx.x * (256 * SI_PIX) + threadIdx.x;
#pragma unroll
  for (int j = 0; j < SI_PIX; ++j) {
    const long long i = base + j * 256;
    if (i >= a.HW) break;
    float v[3] = {img[i], img[a.HW + i], img[2 * a.HW + i]};
    if (p.color_on) {
      const float gs = grey_of(v[0], v[1], v[2]);
      const float gmean = s_mean;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float al = p.alpha[k];
        const float other = p.order[k] == 1 ? __fmul_rn(gmean, 1.f - al) : __fmul_rn(gs, 1.f - al);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v[c] = __fmul_rn(v[c], al);
          if (p.order[k] != 0) v[c] = __fadd_rn(v[c], other);
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = (float)__dadd_rn((double)v[c], p.light[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) img[c * a.HW + i] = __fdiv_rn(__fsub_rn(v[c], a.mean[c]), a.stdv[c]);
  }
}

inline int si_nxb(int dst_w) { return (dst_w + 255) / 256; }
inline int si_nyb(int dst_h) { return (dst_h + SI_ROWS - 1) / SI_ROWS; }

}  // namespace

extern "C" size_t cp_sample_inputs_workspace_bytes(int32_t batch, int32_t dst_h, int32_t dst_w) {
  if (batch <= 0 || dst_h <= 0 || dst_w <= 0) return 0;
  return (size_t)batch * (size_t)si_nyb(dst_h) * (size_t)si_nxb(dst_w) * sizeof(double);
}

extern "C" int cp_sample_inputs_batch(const uint8_t* images, const int64_t* image_offset, const int32_t* image_hw,
                                      const double* trans_input, const double* color, const float* mean,
                                      const float* stdv, int32_t batch, int32_t dst_h, int32_t dst_w, float* out,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  // the host tables first, so that a refusal never depends on what the device pointers are
  CP_CHECK_ARG(image_offset && image_hw && trans_input && color && mean && stdv);
  CP_CHECK_ARG(batch > 0 && dst_h > 0 && dst_w > 0);
  for (int b = 0; b < batch; ++b) {
    CP_CHECK_ARG(image_hw[2 * b] > 0 && image_hw[2 * b + 1] > 0 && image_offset[b] >= 0);
    if (color[10 * b] != 0)
      for (int k = 1; k <= 3; ++k) CP_CHECK_ARG(color[10 * b + k] == 0 || color[10 * b + k] == 1 || color[10 * b + k] == 2);
  }
  if (dst_h > 65535) return CP_EUNSUPPORTED;
  for (int b = 0; b < batch; ++b)
    if (image_hw[2 * b] > 32767 || image_hw[2 * b + 1] > 32767) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(images && out && workspace);
  CP_CHECK_ARG(workspace_bytes >= cp_sample_inputs_workspace_bytes(batch, dst_h, dst_w));

  const long long HW = (long long)dst_h * dst_w;
  const int nxb = si_nxb(dst_w), nyb = si_nyb(dst_h);
  hipStream_t st = (hipStream_t)stream;
  for (int first = 0; first < batch; first += SI_CHUNK) {
    const int n = batch - first < SI_CHUNK ? batch - first : SI_CHUNK;
    WarpArgs w;
    ColorArgs c;
    w.images = images;
    w.out = c.out = out + (long long)first * 3 * HW;
    w.part = (double*)workspace + (long long)first * nxb * nyb;
    c.part = w.part;
    w.dh = dst_h; w.dw = dst_w; w.nxb = nxb; w.nparts = c.nparts = nxb * nyb;
    c.HW = HW;
    for (int k = 0; k < 3; ++k) { c.mean[k] = mean[k]; c.stdv[k] = stdv[k]; }
    for (int i = 0; i < SI_CHUNK; ++i) {
      const int b = first + (i < n ? i : 0);                  // unused slots repeat the chunk's first image
      const double* col = color + 10 * b;
      WarpImage& wi = w.im[i];
      ColorImage& ci = c.im[i];
      cp_invert_affine(trans_input + 6 * b, wi.m);
      wi.offset = image_offset[b];
      wi.sh = image_hw[2 * b]; wi.sw = image_hw[2 * b + 1];
      wi.color_on = ci.color_on = col[0] != 0 ? 1 : 0;
      wi.pad = ci.pad = 0;
      for (int k = 0; k < 3; ++k) {
        ci.order[k] = ci.color_on ? (int)col[1 + k] : 0;
        ci.alpha[k] = ci.color_on ? (float)col[4 + k] : 1.f;
        ci.light[k] = ci.color_on ? col[7 + k] : 0.0;
      }
    }
    hipLaunchKernelGGL(sample_warp_kernel, dim3(nxb, nyb, n), dim3(256), 0, st, w);
    hipLaunchKernelGGL(sample_color_kernel, dim3((unsigned)((HW + 256 * SI_PIX - 1) / (256 * SI_PIX)), 1, n), dim3(256), 0,
                       st, c);
  }
  return cp_launch_status();
}
