// Whole-row soft-NMS by the IoU of the polygons' masks, on DEVICE rows, for gfx950 (--mask_nms).
//
// The literal merge (merge_nms.hip) moves columns 0-4 only and decays by the box IoU: after it a box and its score sit
// in a row whose polygon belongs to another detection.  This file is the usable merge.  Its definition is this
// project's own (include/centerpoly_hip.h): the mask of a row is what ImageDraw.polygon(pts, fill=1) sets on the
// image's H x W canvas with the writers' vertices int(float("%.2f" % v)), the overlap of two rows of one class is the
// IoU of their masks, selection is per class by the largest live score (the lowest position on a tie), every live row
// decays once per selected row, and whole rows move: every column of an output row comes from ONE input row, column 4
// holds the final score.
//
// Kernels (cp_merge_detections_mask: a memset and five launches whatever R is; cp_polygon_overlaps: two memsets and
// the first three):
//   prep    one workgroup: the class of every row (the rule of cp_merge_detections), the clipped bounding box of its
//           integer vertices in rows and 32-pixel words, and the stable partition by class (ballot prefix counts);
//   raster  one wave per (candidate, image row), four to a workgroup: PIL's scan line (sl_wave_spans), the spans ORed
//           into the 32-bit words of the candidate's bit plane (row pitch ceil(W / 32) words).  Only the words of the
//           candidate's own box are written -- every one of them, so the planes need no memset -- and their popcounts
//           go to area[] (one integer atomic per wave);
//   pairs   one wave per pair i <= j of one class whose boxes intersect: popcount(A & B) over the words of the
//           intersection of the two boxes, a wave reduction, one lane stores both cells; the diagonal takes area[i].
//           Every other pair exits at once;
//   select  one wave per class, scores, areas and candidate indices in LDS: the arg-max is the 64-bit-key DPP idiom of
//           row_merge.h, the chosen candidate's line of `inter` is read once per iteration, the decay pass leaves
//           the next iteration's keys behind;
//   cut     one workgroup: merge_outputs' rule on the kept rows (rank counting in LDS), a prefix sum, the whole-row
//           copy.
// The class rule, the partition, the arg-max's order and the cut are row_merge.h's, shared with merge_nms.hip.
// Integer atomics and vector stores only: a call repeats its bits.
#include <math.h>

#include "cp_common.h"
#include "row_merge.h"
#include "scanline.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxRows = 1024;
constexpr int kMaxClasses = 64;
constexpr int kMaxVerts = 64;
constexpr int kThreads = row_merge::kThreads;                            // prep and cut: one row per thread
constexpr int kRowsPerBlock = 4;                                          // waves of the raster kernel's workgroup
constexpr int kPairsPerBlock = 4;                                         // waves of the pair kernel's workgroup
static_assert(kMaxRows == kThreads, "mask_prep_kernel and mask_cut_kernel hold one row per thread");

using row_merge::score_key;
using row_merge::wave_max_key;
using row_merge::wave_sync;

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct Box { int w0, w1, y0, y1; };                                       // words and rows, both ends included

struct MaskArgs {
  const float* rows;          // [R][ncols]
  unsigned* planes;           // workspace: [R][H][pitch]; only the words of a row's box are ever written or read
  Box* box;                   // workspace: [R]; empty (w0 > w1) for a row without a class or off the canvas
  int* cls;                   // workspace: [R]
  int* area;                  // [R], zeroed
  int* inter;                 // [R][R], zeroed
  int* order;                 // workspace: [R] candidates class by class, in position order (or null: no partition)
  int* seg_start;             // workspace: [C]
  int* seg_len;               // workspace: [C]
  int* sel_idx;               // workspace: [R] per class block the selected candidates in selection order, then -1
  float* sel_score;           // workspace: [R] their final scores
  float* out;                 // [R][ncols]
  int* counts;                // [1 + C]
  int R, ncols, N, C, H, W, pitch, max_per_image, method;
  float sigma, Nt, threshold;
};

__global__ __launch_bounds__(kThreads) void mask_prep_kernel(MaskArgs a) {
  __shared__ signed char s_cls[kMaxRows];
  __shared__ unsigned short s_rank[kMaxRows];                             // position of a row within its class
  __shared__ int s_cnt[kMaxClasses];
  __shared__ int s_start[kMaxClasses];
  const int t = threadIdx.x;
  int ci = -1;
  if (t < a.R) {
    const float* row = a.rows + (long long)t * a.ncols;
    ci = row_merge::class_of(row[5], a.C);
    Box b = {1, 0, 1, 0};
    if (ci >= 0) {
      int x0 = INT32_MAX, x1 = INT32_MIN, y0 = INT32_MAX, y1 = INT32_MIN;
      for (int k = 0; k < a.N; ++k) {
        const int x = cp_vertex_int(row[6 + 2 * k]), y = cp_vertex_int(row[7 + 2 * k]);
        x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
      }
      x0 = max(x0, 0); x1 = min(x1, a.W - 1); y0 = max(y0, 0); y1 = min(y1, a.H - 1);
      if (x0 <= x1 && y0 <= y1) { b.w0 = x0 >> 5; b.w1 = x1 >> 5; b.y0 = y0; b.y1 = y1; }
    }
    a.box[t] = b;
    a.cls[t] = ci;
  }
  if (!a.order) return;                                                   // uniform: cp_polygon_overlaps stops here
  if (t < kMaxRows) s_cls[t] = (signed char)ci;
  if (t < a.R) a.sel_idx[t] = -1;
  row_merge::class_partition(s_cls, s_rank, s_cnt, s_start, a.R, a.C, a.seg_start, a.seg_len);
  if (t < a.R && ci >= 0) a.order[s_start[ci] + s_rank[t]] = t;
}

__global__ __launch_bounds__(64 * kRowsPerBlock) void mask_raster_kernel(MaskArgs a) {
  __shared__ int s_p[2 * kMaxVerts];
  __shared__ CmEdge s_edge[kMaxVerts];
  __shared__ float s_x[kRowsPerBlock][2 * kMaxVerts];
  __shared__ SlSpan s_span[kRowsPerBlock][2 * kMaxVerts];
  const int i = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const Box b = a.box[i];
  const int yb = blockIdx.x * kRowsPerBlock;
  if (b.w0 > b.w1 || yb > b.y1 || yb + kRowsPerBlock - 1 < b.y0) return;  // uniform in the workgroup
  const float* row = a.rows + (long long)i * a.ncols;
  if (threadIdx.x < 2 * a.N) s_p[threadIdx.x] = cp_vertex_int(row[6 + threadIdx.x]);
  __syncthreads();
  if (threadIdx.x < kMaxVerts) {
    CmEdge e;
    e.kind = CM_ABSENT;
    if (threadIdx.x < a.N) e = cm_make_edge(s_p, threadIdx.x, a.N);
    s_edge[threadIdx.x] = e;
  }
  // the polygon's last scan line: max(0, largest y) cut at H
  int hi = lane < a.N ? s_p[2 * lane + 1] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hi = max(hi, __shfl_xor(hi, o, 64));
  const int last_row = min(max(hi, 0), a.H);
  __syncthreads();

  const int y = yb + w;
  const int nsp = sl_wave_spans(s_edge, s_x[w], s_span[w], lane, y, last_row, a.W);
  if (y < b.y0 || y > b.y1) return;                                       // (b.y1 <= H - 1)
  unsigned* line = a.planes + ((size_t)i * a.H + y) * a.pitch;
  int cnt = 0;
  for (int wx = b.w0 + lane; wx <= b.w1; wx += 64) {
    const int x0 = wx * 32;
    unsigned bits = 0;
    for (int s = 0; s < nsp; ++s) {
      const SlSpan q = s_span[w][s];
      const int lo = max(q.lo, x0) - x0, hi2 = min(q.hi, x0 + 31) - x0;
      if (lo <= hi2) bits |= ((2u << hi2) - 1u) & ~((1u << lo) - 1u);
    }
    line[wx] = bits;
    cnt += __popc(bits);
  }
  cnt = wave_sum_i(cnt);
  if (lane == 0 && cnt) atomicAdd(&a.area[i], cnt);
}

__global__ __launch_bounds__(64 * kPairsPerBlock) void mask_pairs_kernel(MaskArgs a) {
  const int i = blockIdx.y, lane = threadIdx.x & 63;
  const int j = blockIdx.x * kPairsPerBlock + (threadIdx.x >> 6);
  if (j >= a.R || j < i) return;
  const int ci = a.cls[i];
  if (ci < 0 || a.cls[j] != ci) return;
  if (j == i) {
    if (lane == 0) a.inter[(size_t)i * a.R + i] = a.area[i];
    return;
  }
  const Box p = a.box[i], q = a.box[j];
  const int w0 = max(p.w0, q.w0), w1 = min(p.w1, q.w1), y0 = max(p.y0, q.y0), y1 = min(p.y1, q.y1);
  if (p.w0 > p.w1 || q.w0 > q.w1 || w0 > w1 || y0 > y1) return;
  const int nw = w1 - w0 + 1, total = (y1 - y0 + 1) * nw;                  // <= H * pitch < 2^31
  const unsigned* A = a.planes + ((size_t)i * a.H + y0) * a.pitch + w0;
  const unsigned* B = a.planes + ((size_t)j * a.H + y0) * a.pitch + w0;
  int cnt = 0;
  for (int k = lane; k < total; k += 64) {
    const int yy = k / nw, ww = k - yy * nw;
    const size_t at = (size_t)yy * a.pitch + ww;
    cnt += __popc(A[at] & B[at]);
  }
  cnt = wave_sum_i(cnt);
  if (lane == 0 && cnt) {
    a.inter[(size_t)i * a.R + j] = cnt;
    a.inter[(size_t)j * a.R + i] = cnt;
  }
}

constexpr int kSelectBatch = 4;                                           // positions of a lane in flight in the decay pass

__global__ __launch_bounds__(CP_WAVE) void mask_select_kernel(MaskArgs a) {
  __shared__ float s_sc[kMaxRows];
  __shared__ int s_idx[kMaxRows];                                         // the candidate at a position, -1 once selected
  __shared__ int s_area[kMaxRows];
  __shared__ int s_sel[kMaxRows];                                         // the selected candidates, in selection order
  __shared__ float s_final[kMaxRows];                                     // ... and their final scores
  const int lane = threadIdx.x, c = blockIdx.x;
  const int start = a.seg_start[c];
  const int n = a.seg_len[c];
  if (n <= 0 || start < 0 || start + n > a.R) return;
  unsigned long long best = 0ull;
  for (int p = lane; p < n; p += CP_WAVE) {
    const int r = a.order[start + p];
    const float s = a.rows[(long long)r * a.ncols + 4];
    s_idx[p] = r;
    s_sc[p] = s;
    s_area[p] = a.area[r];
    const unsigned long long k = score_key(s, p);
    best = k > best ? k : best;
  }
  wave_sync();
  const double sigma = (double)a.sigma, Nt = (double)a.Nt;
  int kept = 0;
  // one iteration per selected row: a chain of the arg-max, one line of `inter` from memory and the decay, which
  // leaves the next iteration's keys in `best`; the selection list stays in LDS until the end
  for (int it = 0; it < n; ++it) {
    const unsigned long long top_key = wave_max_key(best);
    if (top_key == 0ull) break;                                           // nothing is live
    const unsigned pos = 0xffffffffu - (unsigned)top_key;
    if (pos >= (unsigned)n) break;                                        // (a NaN score: stay inside the segment)
    const float s = s_sc[pos];
    if (!(s >= a.threshold)) break;                                       // the rest of the class is dropped
    const int top = s_idx[pos], atop = s_area[pos];
    if (top < 0) break;
    wave_sync();                                                          // every lane has read position pos
    if (lane == 0) {
      s_sel[kept] = top;
      s_final[kept] = s;
      s_idx[pos] = -1;
    }
    ++kept;
    wave_sync();
    const int* line = a.inter + (size_t)top * a.R;
    best = 0ull;
    for (int base = 0; base < n; base += kSelectBatch * CP_WAVE) {        // loads first: their latencies overlap
      int r[kSelectBatch], in[kSelectBatch];
#pragma unroll
      for (int q = 0; q < kSelectBatch; ++q) {
        const int p = base + q * CP_WAVE + lane;
        r[q] = p < n ? s_idx[p] : -1;
      }
#pragma unroll
      for (int q = 0; q < kSelectBatch; ++q) in[q] = r[q] >= 0 ? line[r[q]] : 0;
#pragma unroll
      for (int q = 0; q < kSelectBatch; ++q) {
        if (r[q] < 0) continue;
        const int p = base + q * CP_WAVE + lane;
        float sc = s_sc[p];
        if (in[q] > 0) {
          const int uni = atop + s_area[p] - in[q];
          const double ov = (double)in[q] / (double)uni;
          double wgt;
          if (a.method == 1) wgt = ov > Nt ? 1.0 - ov : 1.0;
          else if (a.method == 2) wgt = exp(-(ov * ov) / sigma);
          else wgt = ov > Nt ? 0.0 : 1.0;
          sc = (float)(wgt * (double)sc);
          s_sc[p] = sc;
        }
        const unsigned long long k = score_key(sc, p);
        best = k > best ? k : best;
      }
    }
    wave_sync();
  }
  for (int k = lane; k < kept; k += CP_WAVE) {
    a.sel_idx[start + k] = s_sel[k];
    a.sel_score[start + k] = s_final[k];
  }
}

__global__ __launch_bounds__(kThreads) void mask_cut_kernel(MaskArgs a) {
  __shared__ row_merge::CutLds<1> s_cut;
  __shared__ int s_src[kMaxRows];                                         // the source row of slot r, -1: the slot is empty
  const int t = threadIdx.x;
  if (t < a.R) {
    const int src = a.sel_idx[t];
    s_src[t] = src >= 0 && src < a.R ? src : -1;
  }
  __syncthreads();
  row_merge::cut_rows(
      s_cut, a.R, [&](int r) { return s_src[r] >= 0; }, [&](int r) { return a.sel_score[r]; },
      [&](int r) { return a.rows + (long long)s_src[r] * a.ncols; }, a.seg_start, a.seg_len, a.C, a.max_per_image,
      a.ncols, a.out, a.counts);
}

// ---- the workspace: the bit planes, then the tables ----

struct Layout {
  size_t planes, box, cls, area, inter, order, seg, sel_idx, sel_score, bytes;
};

// `merge`: with the matrix, the areas and the selection tables (cp_merge_detections_mask); without, cp_polygon_overlaps
Layout layout(int R, int C, int H, int W, bool merge) {
  Layout l;
  size_t at = 0;
  const size_t pitch = ((size_t)W + 31) / 32;
  l.planes = at; at += cp_align_up((size_t)R * H * pitch * sizeof(unsigned), 16);
  l.box = at; at += cp_align_up((size_t)R * sizeof(Box), 16);
  l.cls = at; at += cp_align_up((size_t)R * sizeof(int), 16);
  l.area = l.inter = l.order = l.seg = l.sel_idx = l.sel_score = 0;
  if (merge) {
    l.inter = at; at += cp_align_up((size_t)R * R * sizeof(int), 16);     // the matrix and the areas: one memset
    l.area = at; at += cp_align_up((size_t)R * sizeof(int), 16);
    l.order = at; at += cp_align_up((size_t)R * sizeof(int), 16);
    l.seg = at; at += cp_align_up((size_t)2 * C * sizeof(int), 16);
    l.sel_idx = at; at += cp_align_up((size_t)R * sizeof(int), 16);
    l.sel_score = at; at += cp_align_up((size_t)R * sizeof(float), 16);
  }
  l.bytes = at;
  return l;
}

// CP_OK, or why (rows, ncols, classes, canvas) cannot be rasterised; ncols = 2 N + 7
int shape_status(long long R, int ncols, int C, int H, int W) {
  if (R < 1 || ncols < 1 || C < 1 || H < 1 || W < 1) return CP_EINVAL;
  if (ncols < 2 * 3 + 7 || (ncols & 1) == 0) return CP_EINVAL;            // fewer than three vertices, or no (x, y) pairs
  if (R > kMaxRows || C > kMaxClasses || (ncols - 7) / 2 > kMaxVerts || (long long)H * W >= (1ll << 31))
    return CP_EUNSUPPORTED;
  return CP_OK;
}

// prep, raster, pairs; the matrix and the areas are zero.  Without `masks` prep alone: every overlap stays 0.
int launch_overlaps(const MaskArgs& m, bool masks, hipStream_t st) {
  hipLaunchKernelGGL(mask_prep_kernel, dim3(1), dim3(kThreads), 0, st, m);
  int rc = cp_launch_status();
  if (rc != CP_OK || !masks) return rc;
  hipLaunchKernelGGL(mask_raster_kernel, dim3((m.H + kRowsPerBlock - 1) / kRowsPerBlock, m.R),
                     dim3(64 * kRowsPerBlock), 0, st, m);
  rc = cp_launch_status();
  if (rc != CP_OK) return rc;
  hipLaunchKernelGGL(mask_pairs_kernel, dim3((m.R + kPairsPerBlock - 1) / kPairsPerBlock, m.R),
                     dim3(64 * kPairsPerBlock), 0, st, m);
  return cp_launch_status();
}

}  // namespace

extern "C" size_t cp_polygon_overlaps_workspace_bytes(int32_t R, int32_t ncols, int32_t H, int32_t W) {
  if (shape_status(R, ncols, 1, H, W) != CP_OK) return 0;
  return layout(R, 1, H, W, false).bytes;
}

extern "C" int cp_polygon_overlaps(const float* rows, int32_t R, int32_t ncols, int32_t num_classes, int32_t H,
                                   int32_t W, int32_t* area, int32_t* inter, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const int rc = shape_status(R, ncols, num_classes, H, W);
  if (rc != CP_OK) return rc;
  CP_CHECK_ARG(rows && area && inter && workspace);
  CP_CHECK_ARG((((uintptr_t)workspace) & 15) == 0);
  const Layout l = layout(R, 1, H, W, false);
  if (workspace_bytes < l.bytes) return CP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  MaskArgs m = {};
  m.rows = rows; m.area = area; m.inter = inter;
  m.planes = reinterpret_cast<unsigned*>(ws + l.planes);
  m.box = reinterpret_cast<Box*>(ws + l.box);
  m.cls = reinterpret_cast<int*>(ws + l.cls);
  m.R = R; m.ncols = ncols; m.N = (ncols - 7) / 2; m.C = num_classes; m.H = H; m.W = W; m.pitch = (W + 31) / 32;
  if (hipMemsetAsync(area, 0, (size_t)R * sizeof(int), st) != hipSuccess) return CP_EHIP;
  if (hipMemsetAsync(inter, 0, (size_t)R * R * sizeof(int), st) != hipSuccess) return CP_EHIP;
  return launch_overlaps(m, true, st);
}

extern "C" size_t cp_merge_detections_mask_workspace_bytes(int32_t S, int32_t K, int32_t ncols, int32_t num_classes,
                                                           int32_t H, int32_t W) {
  if (S < 1 || K < 1 || shape_status((long long)S * K, ncols, num_classes, H, W) != CP_OK) return 0;
  return layout(S * K, num_classes, H, W, true).bytes;
}

extern "C" int cp_merge_detections_mask(const float* rows, int32_t S, int32_t K, int32_t ncols, int32_t num_classes,
                                        int32_t max_per_image, int32_t nms, float sigma, float Nt, float threshold,
                                        int32_t method, int32_t H, int32_t W, float* out, int32_t* counts,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(S >= 1 && K >= 1 && max_per_image >= 1);
  CP_CHECK_ARG(method >= 0 && method <= 2);
  const int rc0 = shape_status((long long)S * K, ncols, num_classes, H, W);
  if (rc0 != CP_OK) return rc0;
  CP_CHECK_ARG(rows && out && counts && workspace && rows != out);
  CP_CHECK_ARG((((uintptr_t)workspace) & 15) == 0);
  const int R = S * K;
  const Layout l = layout(R, num_classes, H, W, true);
  if (workspace_bytes < l.bytes) return CP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  MaskArgs m = {};
  m.rows = rows; m.out = out; m.counts = counts;
  m.planes = reinterpret_cast<unsigned*>(ws + l.planes);
  m.box = reinterpret_cast<Box*>(ws + l.box);
  m.cls = reinterpret_cast<int*>(ws + l.cls);
  m.inter = reinterpret_cast<int*>(ws + l.inter);
  m.area = reinterpret_cast<int*>(ws + l.area);
  m.order = reinterpret_cast<int*>(ws + l.order);
  m.seg_start = reinterpret_cast<int*>(ws + l.seg);
  m.seg_len = m.seg_start + num_classes;
  m.sel_idx = reinterpret_cast<int*>(ws + l.sel_idx);
  m.sel_score = reinterpret_cast<float*>(ws + l.sel_score);
  m.R = R; m.ncols = ncols; m.N = (ncols - 7) / 2; m.C = num_classes; m.H = H; m.W = W; m.pitch = (W + 31) / 32;
  m.max_per_image = max_per_image; m.method = method;
  m.sigma = sigma; m.Nt = Nt;
  // nms == 0: no masks are drawn, so no row decays, and none is dropped: the class split (each class by descending
  // score) and the cut alone
  m.threshold = nms ? threshold : -__builtin_inff();
  if (hipMemsetAsync(ws + l.inter, 0, l.order - l.inter, st) != hipSuccess) return CP_EHIP;
  int rc = launch_overlaps(m, nms != 0, st);
  if (rc != CP_OK) return rc;
  hipLaunchKernelGGL(mask_select_kernel, dim3(num_classes), dim3(CP_WAVE), 0, st, m);
  rc = cp_launch_status();
  if (rc != CP_OK) return rc;
  hipLaunchKernelGGL(mask_cut_kernel, dim3(1), dim3(kThreads), 0, st, m);
  return cp_launch_status();
}
