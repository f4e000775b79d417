// Detection overlays and the heat-map debug view for gfx950 (demo.py, --debug).
//
// cp_render_overlay composes, over an 8-bit image, the detections cp_writer_instances selected from the device rows:
// per instance a translucent polygon fill, its outline, the box, a label background and the label's glyphs.  Every
// operation's result depends on the input image and the operation alone, and a pixel shows the LAST operation that
// covers it in the order (paint index, operation number), the farthest instance painted first.  So the picture is one
// max-reduction per pixel and one compose pass: integer arithmetic, order independent, the same bits on every run.
//   memset           the operation map (4 bytes per pixel: 8 * paint index + operation, 0 = untouched);
//   raster kernel    one workgroup per (instance, band of 16 rows); a workgroup whose band meets nothing of its
//                    instance returns at once.  Fill: one wave per row, PIL's scan line in the wave form of scanline.h
//                    (lane k owns edge k, the crossings sorted through wave shuffles), the spans
//                    painted with atomicMax.  Outline: PIL's integer line, edge by edge, the on-canvas steps of an edge that
//                    can reach the band spread over the workgroup, each pixel dilated by the (2r+1)^2 square.  Box frame,
//                    label background and glyph cells: rectangles spread over the workgroup;
//   compose kernel   16 pixels per thread (48 image bytes, 64 map bytes, 16-byte accesses where the pointers allow),
//                    the per-instance colours in LDS.
// n (the live count) is read on the device: nothing comes back to the host between the selection and the picture.
//
// cp_render_heatmap is the reference's gen_colormap + add_blend_img on the device in one launch.
#include "cp_common.h"
#include "scanline.h"

namespace {

constexpr int kMaxInst = 128;
constexpr int kMaxVerts = 64;
constexpr int kMaxRows = 1024;
constexpr int kMaxClasses = 32;
constexpr int kMaxLabel = 16;
constexpr int kMaxGlyphs = 128;
constexpr int kMaxRadius = 16;
constexpr int kMaxCoord = 1 << 29;                                        // vertices beyond: the polygon is not drawn
constexpr int kWaves = 4;                                                 // waves of the raster workgroup
constexpr int kBand = 16;                                                 // rows of a band (a multiple of kWaves)
constexpr int kCellW = 6, kCellH = 11;                                    // a glyph cell

enum { OP_FILL = 1, OP_OUTLINE = 2, OP_BOX = 3, OP_LABEL_BG = 4, OP_GLYPH = 5 };

struct OverlayArgs {
  const unsigned char* image;   // [H][W][3]
  unsigned char* out;           // [H][W][3]
  const float* rows;            // [R][2N + 7]
  const int* n;                 // [1]
  const int* src;               // [R]
  const int* poly;              // [R][N][2]
  const unsigned char* palette; // [C][3]
  const int* label_codes;       // [R][L]
  const unsigned char* atlas;   // [G][11][6]
  unsigned* map;                // [H][W]
  int H, W, R, N, C, L, G;
  int alpha, radius, thick, white, show_txt, show_poly;
  unsigned char outline[3];
};

// a box coordinate: the float truncated toward zero, kept inside int32 (a NaN is 0)
__device__ __forceinline__ int box_int(float f) {
  if (f != f) return 0;
  return (int)fminf(fmaxf(f, -2147483648.f), 2147483520.f);
}

__device__ __forceinline__ long long ceil_div(long long a, long long b) {  // b > 0
  const long long q = a / b;
  return q * b < a ? q + 1 : q;
}

// the rectangle [xlo, xhi] x [ylo, yhi] cut to the canvas and to the rows [yb, ye] of this workgroup's band
__device__ __forceinline__ void paint_rect(const OverlayArgs& a, long long xlo, long long xhi, long long ylo,
                                           long long yhi, int yb, int ye, unsigned code) {
  xlo = xlo < 0 ? 0 : xlo;
  xhi = xhi > a.W - 1 ? a.W - 1 : xhi;
  ylo = ylo < yb ? yb : ylo;
  yhi = yhi > ye ? ye : yhi;
  if (xlo > xhi || ylo > yhi) return;
  const long long w = xhi - xlo + 1, area = w * (yhi - ylo + 1);           // at most W * kBand
  for (long long k = threadIdx.x; k < area; k += 64 * kWaves) {
    const long long dy = k / w, dx = k - dy * w;
    atomicMax(a.map + (ylo + dy) * a.W + xlo + dx, code);
  }
}

__global__ __launch_bounds__(64 * kWaves) void overlay_raster_kernel(OverlayArgs a) {
  __shared__ CmEdge s_edge[kMaxVerts];
  __shared__ float s_x[kWaves][2 * kMaxVerts];
  __shared__ SlSpan s_span[kWaves][2 * kMaxVerts];
  const int n = a.n[0], i = blockIdx.y;
  if (n > kMaxInst || n > a.R || i >= n) return;                          // (uniform in the workgroup, as all below)
  const int s = a.src[i];
  if (s < 0 || s >= a.R) return;
  const int yb = blockIdx.x * kBand, ye = min(yb + kBand, a.H) - 1;
  const unsigned base = (unsigned)(n - 1 - i) * 8u;                       // farthest first: paint index n - 1 - i
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int* p = a.poly + (long long)i * a.N * 2;
  const float* row = a.rows + (long long)s * (2 * a.N + 7);
  const int x1 = box_int(row[0]), y1 = box_int(row[1]), x2 = box_int(row[2]), y2 = box_int(row[3]);

  // the polygon's rows: [lo, hi]; its last scan line is max(0, hi) cut at H
  int hi = lane < a.N ? p[2 * lane + 1] : INT32_MIN, lo = lane < a.N ? p[2 * lane + 1] : INT32_MAX;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hi = max(hi, __shfl_xor(hi, o, 64));
    lo = min(lo, __shfl_xor(lo, o, 64));
  }
  const int last_row = min(max(hi, 0), a.H);
  // A polygon with a coordinate beyond +-2^29 is not drawn (its box and label are): the products of the line's closed
  // form stay inside 64 bits, and PIL has no defined drawing that far out either.
  int far = 0;
  if (lane < a.N) {
    const int vx = p[2 * lane], vy = p[2 * lane + 1];
    far = vx > kMaxCoord || vx < -kMaxCoord || vy > kMaxCoord || vy < -kMaxCoord;
  }
  const bool poly_ok = a.show_poly && __ballot(far) == 0ull;

  int len = 0;                                                            // the label's length: leading codes >= 0
  if (a.show_txt) {
    const int* codes = a.label_codes + (long long)s * a.L;
    while (len < a.L && codes[len] >= 0) ++len;
  }
  const long long ly0 = (long long)y1 - 2 - (kCellH - 1), ly1 = (long long)y1 - 2;   // the label's rows

  const bool fill_here = poly_ok && max(lo, 0) <= ye && min(last_row, a.H - 1) >= yb && max(lo, 0) <= min(last_row, a.H - 1);
  const bool line_here = poly_ok && (long long)lo - a.radius <= ye && (long long)hi + a.radius >= yb;
  const bool box_here = a.thick > 0 && x1 <= x2 && y1 <= y2 && y1 <= ye && y2 >= yb;
  const bool label_here = len > 0 && ly0 <= ye && ly1 >= yb;
  if (!(fill_here || line_here || box_here || label_here)) return;

  // ---- 1: fill, PIL's scan line (sl_wave_spans), the spans painted ----
  if (fill_here) {
    if (tid < kMaxVerts) {
      CmEdge e;
      e.kind = CM_ABSENT;
      if (tid < a.N) e = cm_make_edge(p, tid, a.N);
      s_edge[tid] = e;
    }
    __syncthreads();
    for (int it = 0; it < kBand / kWaves; ++it) {
      const int y = yb + it * kWaves + w;
      const int nsp = sl_wave_spans(s_edge, s_x[w], s_span[w], lane, y, last_row, a.W);
      if (y <= ye) {
        unsigned* mrow = a.map + (long long)y * a.W;
        for (int q = 0; q < nsp; ++q) {
          const SlSpan v = s_span[w][q];                                  // inside [0, W - 1] by construction
          for (int x = v.lo + lane; x <= v.hi; x += 64) atomicMax(mrow + x, base | OP_FILL);
        }
      }
    }
  }

  // ---- 2: outline, PIL's integer line dilated by the (2r + 1)^2 square ----
  if (line_here) {
    const int r = a.radius;
    for (int k = 0; k < a.N; ++k) {
      const int j = k + 1 == a.N ? 0 : k + 1;
      const int ex0 = p[2 * k], ey0 = p[2 * k + 1], ex1 = p[2 * j], ey1 = p[2 * j + 1];
      const long long steps = cm_line_steps(ex0, ey0, ex1, ey1);
      if (steps < 0) continue;
      const long long dx = (long long)ex1 - ex0, dy = (long long)ey1 - ey0;
      const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
      const bool xmajor = ax > ay;
      // the steps t whose pixel lies on the canvas and can reach this band: the coordinate along the longer axis is c0 +- t, the other one
      // o0 +- m(t) with m(t) = floor((2 dmin t + dmaj) / (2 dmaj)), so m >= M exactly from t = ceil((2 dmaj M - dmaj) / (2 dmin))
      const long long dmaj = xmajor ? ax : ay, dmin = xmajor ? ay : ax;
      const long long c0 = xmajor ? ex0 : ey0, o0 = xmajor ? ey0 : ex0;
      const bool fwd = (xmajor ? dx : dy) >= 0, ofwd = (xmajor ? dy : dx) >= 0;
      const long long ylo = max(yb - r, 0), yhi = min(ye + r, a.H - 1);    // rows of the canvas that reach the band
      const long long clo = xmajor ? 0 : ylo, chi = xmajor ? (long long)a.W - 1 : yhi;
      const long long olo = xmajor ? ylo : 0, ohi = xmajor ? yhi : (long long)a.W - 1;
      long long t0 = fwd ? clo - c0 : c0 - chi, t1 = fwd ? chi - c0 : c0 - clo;
      long long m0 = ofwd ? olo - o0 : o0 - ohi, m1 = ofwd ? ohi - o0 : o0 - olo;
      m0 = m0 < 0 ? 0 : m0;
      m1 = m1 > dmin ? dmin : m1;
      if (m0 > m1) continue;
      if (dmin > 0) {
        const long long u0 = ceil_div(2 * dmaj * m0 - dmaj, 2 * dmin), u1 = ceil_div(2 * dmaj * (m1 + 1) - dmaj, 2 * dmin) - 1;
        t0 = t0 > u0 ? t0 : u0;
        t1 = t1 < u1 ? t1 : u1;
      }
      t0 = t0 < 0 ? 0 : t0;
      t1 = t1 > steps ? steps : t1;
      for (long long t = t0 + tid; t <= t1; t += 64 * kWaves) {
        int px, py;
        cm_line_pixel(ex0, ey0, ex1, ey1, t, &px, &py);
        if (px < 0 || px >= a.W || py < 0 || py >= a.H) continue;         // (only pixels PIL sets are dilated)
        for (int oy = -r; oy <= r; ++oy) {
          const long long yy = (long long)py + oy;
          if (yy < yb || yy > ye) continue;
          for (int ox = -r; ox <= r; ++ox) {
            const long long xx = (long long)px + ox;
            if (xx >= 0 && xx < a.W) atomicMax(a.map + yy * a.W + xx, base | OP_OUTLINE);
          }
        }
      }
    }
  }

  // ---- 3: the box's frame, the pixels of the box within `thick` of one of its sides ----
  if (box_here) {
    const long long t = a.thick;
    const long long yt = min((long long)y2, y1 + t - 1), yu = max((long long)y1, y2 - t + 1);
    const long long xt = min((long long)x2, x1 + t - 1), xu = max((long long)x1, x2 - t + 1);
    paint_rect(a, x1, x2, y1, yt, yb, ye, base | OP_BOX);
    paint_rect(a, x1, x2, yu, y2, yb, ye, base | OP_BOX);
    paint_rect(a, x1, xt, y1, y2, yb, ye, base | OP_BOX);
    paint_rect(a, xu, x2, y1, y2, yb, ye, base | OP_BOX);
  }

  // ---- 4, 5: the label's background and its glyphs, cell j at (x1 + 6 j, y1 - 12) ----
  if (label_here) {
    paint_rect(a, x1, (long long)x1 + kCellW * len - 1, ly0, ly1, yb, ye, base | OP_LABEL_BG);
    const int* codes = a.label_codes + (long long)s * a.L;
    for (int k = tid; k < len * kCellW * kCellH; k += 64 * kWaves) {
      const int cell = k / (kCellW * kCellH), q = k - cell * (kCellW * kCellH);
      const int cy = q / kCellW, cx = q - cy * kCellW;
      const int g = codes[cell];
      if (g >= a.G || !a.atlas[(g * kCellH + cy) * kCellW + cx]) continue;
      const long long xx = (long long)x1 + kCellW * cell + cx, yy = ly0 + cy;
      if (xx >= 0 && xx < a.W && yy >= yb && yy <= ye) atomicMax(a.map + yy * a.W + xx, base | OP_GLYPH);
    }
  }
}

__global__ __launch_bounds__(256) void overlay_compose_kernel(OverlayArgs a) {
  __shared__ unsigned s_col[kMaxInst];                                    // by paint index: the class colour, themed
  const int tid = threadIdx.x;
  int n = a.n[0];
  if (n > kMaxInst || n > a.R || n < 0) n = 0;
  if (tid < kMaxInst) {
    unsigned col = 0;
    if (tid < n) {
      const int s = a.src[n - 1 - tid];
      if (s >= 0 && s < a.R) {
        const int cls = min(max((int)a.rows[(long long)s * (2 * a.N + 7) + 5], 0), a.C - 1);
        for (int k = 0; k < 3; ++k) {
          const unsigned v = a.palette[3 * cls + k];
          col |= (a.white ? 255u - v : v) << (8 * k);
        }
      }
    }
    s_col[tid] = col;
  }
  __syncthreads();
  const long long HW = (long long)a.H * a.W;
  const long long p0 = ((long long)blockIdx.x * 256 + tid) * 16;
  if (p0 >= HW) return;
  const int cnt = p0 + 16 <= HW ? 16 : (int)(HW - p0);
  const unsigned char* in = a.image + p0 * 3;
  unsigned char* out = a.out + p0 * 3;
  const unsigned* mp = a.map + p0;
  const bool wide = cnt == 16 && (((uintptr_t)a.image | (uintptr_t)a.out | (uintptr_t)a.map) & 15) == 0;
  unsigned code[16], pix[12];
  if (wide) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 v = reinterpret_cast<const uint4*>(mp)[q];
      code[4 * q] = v.x; code[4 * q + 1] = v.y; code[4 * q + 2] = v.z; code[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const uint4 v = reinterpret_cast<const uint4*>(in)[q];
      pix[4 * q] = v.x; pix[4 * q + 1] = v.y; pix[4 * q + 2] = v.z; pix[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) code[k] = k < cnt ? mp[k] : 0u;
#pragma unroll
    for (int k = 0; k < 12; ++k) pix[k] = 0u;
#pragma unroll
    for (int k = 0; k < 48; ++k)
      if (k < 3 * cnt) pix[k >> 2] |= (unsigned)in[k] << (8 * (k & 3));
  }
  unsigned any = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) any |= code[k];
  if (any == 0u && a.out == a.image) return;                              // nothing drawn here, drawn in place
  if (any != 0u) {
    const unsigned line = a.outline[0] | (a.outline[1] << 8) | (a.outline[2] << 16);
    const unsigned al = (unsigned)a.alpha;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const unsigned c = code[k];
      if (c == 0u) continue;
      const unsigned op = c & 7u, col = s_col[(c >> 3) & (kMaxInst - 1)];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int b = 3 * k + ch, sh = 8 * (b & 3);
        const unsigned orig = (pix[b >> 2] >> sh) & 255u, cc = (col >> (8 * ch)) & 255u;
        unsigned v;
        if (op == OP_FILL) v = (orig * (256u - al) + cc * al + 128u) >> 8;
        else if (op == OP_OUTLINE) v = (line >> (8 * ch)) & 255u;
        else if (op == OP_GLYPH) v = 0u;
        else v = cc;
        pix[b >> 2] = (pix[b >> 2] & ~(255u << sh)) | (v << sh);
      }
    }
  }
  if (wide) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      reinterpret_cast<uint4*>(out)[q] = make_uint4(pix[4 * q], pix[4 * q + 1], pix[4 * q + 2], pix[4 * q + 3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 48; ++k)
      if (k < 3 * cnt) out[k] = (unsigned char)(pix[k >> 2] >> (8 * (k & 3)));
  }
}

struct HeatmapArgs {
  const float* hm;              // [C][h][w], activated (C == 0: no heat map, the de-normalised input alone)
  const float* input;           // [3][h * ratio][w * ratio], normalised
  const unsigned char* palette; // [P][3]
  unsigned char* out;           // [h * ratio][w * ratio][3]
  int C, h, w, ratio, P, white;
  float mean[3], stdv[3];
};

// uint8(v) of a float32 already meant to lie in 0..255: kept there (a NaN is 0), truncated
__device__ __forceinline__ unsigned to_u8(float v) { return (unsigned)(int)fminf(fmaxf(v, 0.f), 255.f); }

__global__ __launch_bounds__(256) void heatmap_kernel(HeatmapArgs a) {
  const int W = a.w * a.ratio, H = a.h * a.ratio;
  const long long HW = (long long)H * W;
  const long long pixel = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pixel >= HW) return;
  const int Y = (int)(pixel / W), X = (int)(pixel - (long long)Y * W);
  const int y = Y / a.ratio, x = X / a.ratio;
  unsigned cm[3] = {0u, 0u, 0u};
  for (int c = 0; c < a.C; ++c) {
    const float v = a.hm[((long long)c * a.h + y) * a.w + x];
    const unsigned char* col = a.palette + 3 * (c % a.P);
#pragma unroll
    for (int k = 0; k < 3; ++k) cm[k] = max(cm[k], to_u8(__fmul_rn(v, (float)col[k])));
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned m = a.white ? 255u - cm[k] : cm[k];
    const float xin = a.input[(long long)k * HW + pixel];
    const unsigned back = to_u8(__fmul_rn(__fadd_rn(__fmul_rn(xin, a.stdv[k]), a.mean[k]), 255.f));
    a.out[pixel * 3 + k] = (unsigned char)(a.C == 0 ? back : (back * 77u + m * 179u + 128u) >> 8);
  }
}

}  // namespace

extern "C" size_t cp_render_overlay_workspace_bytes(int32_t H, int32_t W) {
  if (H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31)) return 0;
  return (size_t)H * (size_t)W * sizeof(unsigned);
}

extern "C" int cp_render_overlay(const uint8_t* image, int32_t H, int32_t W, const float* rows, int32_t R, int32_t N,
                                 const int32_t* n, const int32_t* src, const int32_t* poly, const uint8_t* palette,
                                 int32_t C, const int32_t* label_codes, int32_t L, const uint8_t* atlas, int32_t G,
                                 const cp_overlay_params* params, uint8_t* out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(H > 0 && W > 0 && R >= 1 && N >= 3 && C >= 1 && L >= 0 && G >= 0);
  CP_CHECK_ARG(image && rows && n && src && poly && palette && params && out && workspace);
  CP_CHECK_ARG(params->alpha >= 0 && params->alpha <= 256 && params->outline_radius >= 0 &&
               params->box_thickness >= 0);
  const bool text = params->show_txt != 0 && L > 0;
  CP_CHECK_ARG(!text || (label_codes && atlas));
  if (R > kMaxRows || N > kMaxVerts || C > kMaxClasses || L > kMaxLabel || G > kMaxGlyphs ||
      (long long)H * W >= (1ll << 31) || params->outline_radius > kMaxRadius)
    return CP_EUNSUPPORTED;
  if (workspace_bytes < cp_render_overlay_workspace_bytes(H, W)) return CP_EWORKSPACE;
  OverlayArgs a;
  a.image = image; a.out = out; a.rows = rows; a.n = n; a.src = src; a.poly = poly; a.palette = palette;
  a.label_codes = label_codes; a.atlas = atlas; a.map = (unsigned*)workspace;
  a.H = H; a.W = W; a.R = R; a.N = N; a.C = C; a.L = L; a.G = G;
  a.alpha = params->alpha; a.radius = params->outline_radius; a.thick = params->box_thickness;
  a.white = params->white_theme != 0; a.show_txt = text; a.show_poly = params->show_polygons != 0;
  for (int k = 0; k < 3; ++k) a.outline[k] = params->outline_colour[k];
  hipStream_t st = (hipStream_t)stream;
  const long long HW = (long long)H * W;
  if (hipMemsetAsync(workspace, 0, (size_t)HW * sizeof(unsigned), st) != hipSuccess) return CP_EHIP;
  hipLaunchKernelGGL(overlay_raster_kernel, dim3((H + kBand - 1) / kBand, kMaxInst), dim3(64 * kWaves), 0, st, a);
  hipLaunchKernelGGL(overlay_compose_kernel, dim3((unsigned)((HW + 4095) / 4096)), dim3(256), 0, st, a);
  return cp_launch_status();
}

extern "C" int cp_render_heatmap(const float* hm, int32_t C, int32_t h, int32_t w, int32_t ratio, const float* input,
                                 const float* mean, const float* stdv, const uint8_t* palette, int32_t P,
                                 int32_t white, uint8_t* out, void* stream) {
  CP_CHECK_ARG(C >= 0 && h > 0 && w > 0 && ratio >= 1 && P >= 1);
  CP_CHECK_ARG((hm || C == 0) && input && mean && stdv && palette && out);
  const long long HW = (long long)h * ratio * (long long)w * ratio;
  if (P > kMaxClasses || (long long)h * ratio >= (1ll << 31) || (long long)w * ratio >= (1ll << 31) ||
      HW >= (1ll << 31))
    return CP_EUNSUPPORTED;
  HeatmapArgs a;
  a.hm = hm; a.input = input; a.palette = palette; a.out = out;
  a.C = C; a.h = h; a.w = w; a.ratio = ratio; a.P = P; a.white = white != 0;
  for (int k = 0; k < 3; ++k) { a.mean[k] = mean[k]; a.stdv[k] = stdv[k]; }
  hipLaunchKernelGGL(heatmap_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return cp_launch_status();
}
