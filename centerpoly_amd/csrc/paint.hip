// Ground-truth id images from polygon files for gfx950: the painter of the evaluators' preparation scripts
// (IDDscripts/preperation/json2instanceImg.py and json2labelImg.py, cityscapesscripts/preparation/json2instanceImg.py
// and json2labelImg.py) on the device.
//
// The scripts open one canvas with a background value and call ImageDraw.polygon(pts, fill=v) for every kept object
// of the file, in file order: a later polygon overwrites what lies under it.  With F_i the fill of polygon i (the F of
// class_masks.hip: no outline) a pixel therefore holds value[i] of the LARGEST i whose F_i has it, and the background
// where there is none.  A polygon of two vertices (a, b) has the edges a -> b and b -> a, as PIL builds them: F of
// (a, b, a).
//
//   paint_edges_kernel   one workgroup per polygon: the edge table and the polygon's smallest and largest y, once
//                        (sl_group_edges of scanline.h).
//   paint_rows_kernel    the drawing order is a dependency, so a row belongs to exactly one workgroup.  It holds the
//                        row (W int32, at most 64 KB) in LDS, walks the polygons in order, skips those whose y-range
//                        misses the row, and for each of the others runs the workgroup form's row pass (sl_group_row:
//                        crossings collected and sorted in LDS), which overwrites the spans and the flat edges of the
//                        row in the LDS image.  The row goes to memory once, coalesced.
// No atomics on memory, no read-modify-write of the image, two launches and one copy of `first` whatever n is.
// Integers and float32 with no contraction: the same bits on every run.
#include "cp_common.h"
#include "scanline.h"

namespace {

constexpr int kMaxPaintPolys = 4096;
constexpr int kMaxPaintVerts = kSlMaxGroupVerts;                          // of one polygon
constexpr int kMaxPaintTotal = 1 << 20;                                   // of all polygons
constexpr int kMaxPaintWidth = 16384;                                     // the row image: 64 KB of LDS

struct PaintArgs {
  const int* xy;              // [T][2]
  const int* value;           // [n]
  const int* first;           // [n + 1] (workspace, copied from the host)
  CmEdge* edges;              // [T] (workspace)
  int* yrange;                // [n][2]: smallest and largest y of the polygon (workspace)
  int* image;                 // [H][W]
  int n, H, W, background;
};

__global__ __launch_bounds__(256) void paint_edges_kernel(PaintArgs a) {
  // N == 2: a -> b, then the closing edge b -> a (absent only when a == b, where a -> b is the one flat pixel)
  const int i = blockIdx.x, base = a.first[i];
  sl_group_edges(a.xy + 2ll * base, a.first[i + 1] - base, a.edges + base, a.yrange + 2 * i);
}

// s_x, s_n: sl_group_row's list and counter for the current polygon.  s_row: the row as painted so far, W <= kWidth
// int32.  Every index into s_row is cut to 0 .. W-1.
template <int kWidth>
__global__ __launch_bounds__(256) void paint_rows_kernel(PaintArgs a) {
  __shared__ int s_row[kWidth];
  __shared__ float s_x[2 * kMaxPaintVerts];
  __shared__ int s_n;
  const int y = blockIdx.x, t = threadIdx.x;
  for (int x = t; x < a.W; x += 256) s_row[x] = a.background;
  for (int i = 0; i < a.n; ++i) {
    const int ylo = a.yrange[2 * i], yhi = a.yrange[2 * i + 1];
    if (y < ylo || y > yhi) continue;                                     // uniform in the workgroup
    const int base = a.first[i], N = a.first[i + 1] - base;
    const CmEdge* edges = a.edges + base;
    const int last_row = min(max(yhi, 0), a.H);
    const int v = a.value[i];
    __syncthreads();                                                      // the previous polygon is done with s_x
    sl_group_row(edges, N, y, last_row, a.W, s_x, &s_n, [&](int x) { s_row[x] = v; });
  }
  __syncthreads();
  int* row = a.image + (long long)y * a.W;
  for (int x = t; x < a.W; x += 256) row[x] = s_row[x];
}

size_t paint_edges_bytes(int T) { return cp_align_up((size_t)T * sizeof(CmEdge), 16); }
size_t paint_first_bytes(int n) { return cp_align_up((size_t)(n + 1) * sizeof(int), 16); }

}  // namespace

extern "C" size_t cp_polygon_paint_workspace_bytes(int32_t n, int32_t total_vertices) {
  if (n < 0 || total_vertices < 0) return 0;
  return paint_edges_bytes(total_vertices) + paint_first_bytes(n) + (size_t)n * 2 * sizeof(int);
}

extern "C" int cp_polygon_paint(const int32_t* xy, const int32_t* first, const int32_t* value, int32_t n,
                                int32_t background, int32_t H, int32_t W, int32_t* image, void* workspace,
                                size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(n >= 0 && H > 0 && W > 0);
  if (n > kMaxPaintPolys || W > kMaxPaintWidth || (long long)H * W >= (1ll << 31)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(image);
  int T = 0;
  if (n > 0) {
    CP_CHECK_ARG(xy && first && value && workspace);
    CP_CHECK_ARG(first[0] == 0);
    for (int i = 0; i < n; ++i) {
      const long long len = (long long)first[i + 1] - first[i];
      CP_CHECK_ARG(len >= 2);
      if (len > kMaxPaintVerts || first[i + 1] > kMaxPaintTotal) return CP_EUNSUPPORTED;
    }
    T = first[n];
    if (workspace_bytes < cp_polygon_paint_workspace_bytes(n, T)) return CP_EWORKSPACE;
  }
  PaintArgs a;
  a.xy = xy; a.value = value; a.image = image;
  a.edges = (CmEdge*)workspace;
  a.first = n > 0 ? (const int*)((char*)workspace + paint_edges_bytes(T)) : nullptr;
  a.yrange = n > 0 ? (int*)((char*)workspace + paint_edges_bytes(T) + paint_first_bytes(n)) : nullptr;
  a.n = n; a.H = H; a.W = W; a.background = background;
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    // pageable host memory has been read when the copy call returns; a pinned array must stay unchanged until the
    // stream reaches the copy (the header says so)
    if (hipMemcpyAsync((void*)a.first, first, (size_t)(n + 1) * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess)
      return CP_EHIP;
    hipLaunchKernelGGL(paint_edges_kernel, dim3(n), dim3(256), 0, st, a);
  }
  // the row image is static LDS in three sizes: 40 KB, 48 KB or 96 KB a workgroup with the crossing list
  if (W <= 2048) hipLaunchKernelGGL(paint_rows_kernel<2048>, dim3(H), dim3(256), 0, st, a);
  else if (W <= 4096) hipLaunchKernelGGL(paint_rows_kernel<4096>, dim3(H), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(paint_rows_kernel<kMaxPaintWidth>, dim3(H), dim3(256), 0, st, a);
  return cp_launch_status();
}
