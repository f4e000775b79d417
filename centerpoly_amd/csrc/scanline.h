// PIL's scan line on the device, once: what stands between the arithmetic of class_masks_core.h and the stores of
// the four rasterisers that restate ImageDraw.polygon (class_masks.hip, render.hip, annotate.hip, paint.hip).
//   wave form       a polygon of at most 64 vertices, lane k owns edge k: the row's crossings, sorted through wave
//                   shuffles (wave_sort.h), become a compacted list of clipped spans in LDS (sl_wave_spans);
//   workgroup form  a polygon of at most kSlMaxGroupVerts vertices and 256 threads: the edge table and the y-range
//                   once (sl_group_edges), then per row the crossings collected through an LDS counter, sorted by a
//                   bitonic network in LDS and painted one span per wave, the flat edges after them (sl_group_row);
//   clipped line    the on-canvas steps of PIL's integer line, the error term carried step by step (sl_line_clipped).
// What a caller does with a span or a pixel is its own: the stores are callables, inlined.  Device code only; the
// arithmetic itself stays in class_masks_core.h, which also compiles for the host.
#pragma once
#include "class_masks_core.h"
#include "wave_sort.h"

struct SlSpan { int lo, hi; };

constexpr float kSlNone = __builtin_inff();                               // "no crossing": sorts behind every value
constexpr int kSlMaxGroupVerts = 4096;                                    // workgroup form: s_x holds 2 * this floats

// ------------------------------------------------------------------------------------------------- wave form ----

// Row y of the polygon whose edge table (64 entries, absent ones CM_ABSENT) is s_edge, for one wave; every wave of
// the workgroup calls it (two barriers).  s_x and s_span are this wave's 128 entries.  Returns the number of spans in
// s_span: pair s of the sorted crossings, then the flat edges of the row; cut to 0 .. W - 1, empty ones dropped.
__device__ __forceinline__ int sl_wave_spans(const CmEdge* s_edge, float* s_x, SlSpan* s_span, int lane, int y,
                                             int last_row, int W) {
  float out[2] = {kSlNone, kSlNone};
  const int c = cm_crossings([&](int j) { return s_edge[j]; }, lane, y, last_row, out);
  float xa = c >= 1 ? out[0] : kSlNone, xb = c == 2 ? out[1] : kSlNone;
  const int cnt = __popcll(__ballot(c >= 1)) + __popcll(__ballot(c == 2));
  wave_sort128(xa, xb, lane);
  s_x[lane] = xa;
  s_x[lane + 64] = xb;
  __syncthreads();

  const unsigned long long below = (1ull << lane) - 1ull;
  SlSpan sp;
  sp.lo = 1; sp.hi = 0;
  if (2 * lane + 1 < cnt) {
    sp.lo = max(cm_round_up(s_x[2 * lane]), 0);
    sp.hi = min(cm_round_down(s_x[2 * lane + 1]), W - 1);
  }
  const unsigned long long m1 = __ballot(sp.lo <= sp.hi);
  if (sp.lo <= sp.hi) s_span[__popcll(m1 & below)] = sp;
  const CmEdge e = s_edge[lane];
  SlSpan fl;
  fl.lo = 1; fl.hi = 0;
  if (e.kind == CM_FLAT && e.ymin == y) { fl.lo = max(e.xmin, 0); fl.hi = min(e.xmax, W - 1); }
  const unsigned long long m2 = __ballot(fl.lo <= fl.hi);
  const int n1 = __popcll(m1);
  if (fl.lo <= fl.hi) s_span[n1 + __popcll(m2 & below)] = fl;
  __syncthreads();
  return n1 + __popcll(m2);
}

// -------------------------------------------------------------------------------------------- workgroup form ----

// The edge table of the polygon p[0 .. N) and its smallest and largest y (yrange[0], yrange[1]); 256 threads.
__device__ __forceinline__ void sl_group_edges(const int* p, int N, CmEdge* edges, int* yrange) {
  __shared__ int s_lo[4], s_hi[4];
  const int t = threadIdx.x;
  int lo = INT32_MAX, hi = INT32_MIN;
  for (int k = t; k < N; k += 256) {
    edges[k] = cm_make_edge(p, k, N);
    const int y = p[2 * k + 1];
    lo = min(lo, y); hi = max(hi, y);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o, 64));
    hi = max(hi, __shfl_xor(hi, o, 64));
  }
  if ((t & 63) == 0) { s_lo[t >> 6] = lo; s_hi[t >> 6] = hi; }
  __syncthreads();
  if (t == 0) {
    yrange[0] = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
    yrange[1] = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
  }
}

// Row y of the polygon whose N edges are `edges`; 256 threads, all of them call it.  paint(x) sets one pixel, x in
// 0 .. W - 1; a pixel may be painted more than once.  s_x (2 * kSlMaxGroupVerts floats of LDS) holds the row's
// crossing list, an edge gives at most two, and after it the row's flat edges, one span of two integers each;
// *counter (LDS) counts both, the flat edges on from the number of crossings, so it is set once.  The caller has
// made sure that no thread still uses s_x or *counter from an earlier call.
template <typename Paint>
__device__ __forceinline__ void sl_group_row(const CmEdge* edges, int N, int y, int last_row, int W, float* s_x,
                                             int* counter, Paint paint) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t == 0) *counter = 0;
  __syncthreads();
  for (int k = t; k < N; k += 256) {
    float out[2];
    const int c = cm_crossings([&](int j) { return edges[j]; }, k, y, last_row, out);
    if (c) {
      const int at = atomicAdd(counter, c);                               // LDS; the list is sorted below
      s_x[at] = out[0];
      if (c == 2) s_x[at + 1] = out[1];
    }
  }
  __syncthreads();
  const int cnt = *counter;
  int P = 2;
  while (P < cnt) P <<= 1;
  for (int k = cnt + t; k < P; k += 256) s_x[k] = kSlNone;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)                                        // bitonic sort, ascending
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = t; q < P; q += 256) {
        const int o = q ^ j;
        if (o > q) {
          const float u = s_x[q], v = s_x[o];
          if ((u > v) == ((q & k) == 0)) { s_x[q] = v; s_x[o] = u; }
        }
      }
      __syncthreads();
    }
  for (int s = w; 2 * s + 1 < cnt; s += 4) {                              // one wave per span
    const int lo = max(cm_round_up(s_x[2 * s]), 0), hi = min(cm_round_down(s_x[2 * s + 1]), W - 1);
    for (int x = lo + lane; x <= hi; x += 64) paint(x);
  }
  __syncthreads();
  int* s_flat = reinterpret_cast<int*>(s_x);
  for (int k = t; k < N; k += 256) {
    const CmEdge e = edges[k];
    if (e.kind == CM_FLAT && e.ymin == y) {
      const int lo = max(e.xmin, 0), hi = min(e.xmax, W - 1);
      if (lo <= hi) {
        const int at = atomicAdd(counter, 1) - cnt;                       // the same value everywhere: any order
        s_flat[2 * at] = lo; s_flat[2 * at + 1] = hi;
      }
    }
  }
  __syncthreads();
  const int nflat = *counter - cnt;
  for (int s = w; s < nflat; s += 4) {
    const int lo = s_flat[2 * s], hi = s_flat[2 * s + 1];
    for (int x = lo + lane; x <= hi; x += 64) paint(x);
  }
}

// ---------------------------------------------------------------------------------------------- clipped line ----

// PIL's integer line from (x0, y0) to (x1, y1) on a W x H canvas: put(y * W + x) for every pixel of it that is on the
// canvas.  Only the steps whose coordinate along the longer axis is on the canvas are walked (a vertex far away costs
// nothing); the other coordinate starts from the closed form and its error term is carried step by step
// (cm_line_pixel).  An edge between two equal vertices draws nothing.
template <typename Put>
__device__ __forceinline__ void sl_line_clipped(int x0, int y0, int x1, int y1, int W, int H, Put put) {
  const long long steps = cm_line_steps(x0, y0, x1, y1);
  if (steps < 0) return;
  const long long dx = (long long)x1 - x0, dy = (long long)y1 - y0;
  const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  const bool xmajor = ax > ay;
  const long long c0 = xmajor ? x0 : y0, size = xmajor ? W : H;
  const bool fwd = (xmajor ? dx : dy) >= 0;
  long long t0 = fwd ? -c0 : c0 - (size - 1), t1 = fwd ? size - 1 - c0 : c0;
  t0 = t0 < 0 ? 0 : t0;
  t1 = t1 > steps ? steps : t1;
  if (t0 > t1) return;
  const long long dmaj = xmajor ? ax : ay, dmin = xmajor ? ay : ax;
  long long m = (2 * dmin * t0 + dmaj) / (2 * dmaj);
  long long r = (2 * dmin * t0 + dmaj) - m * (2 * dmaj);
  const int smaj = fwd ? 1 : -1, smin = (xmajor ? dy : dx) < 0 ? -1 : 1;
  const long long o0 = xmajor ? y0 : x0, osize = xmajor ? H : W;
  for (long long s = t0; s <= t1; ++s) {
    const long long cmaj = c0 + smaj * s, cmin = o0 + smin * m;
    if (cmin >= 0 && cmin < osize) put(xmajor ? cmin * W + cmaj : cmaj * W + cmin);
    r += 2 * dmin;
    if (r >= 2 * dmaj) { r -= 2 * dmaj; m += 1; }
  }
}
