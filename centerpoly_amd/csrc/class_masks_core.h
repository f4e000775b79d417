// The arithmetic of PIL's two polygon primitives, restated for class_masks.hip: what one edge contributes to one
// scan line of ImageDraw.polygon(fill=...), and where ImageDraw.polygon(outline=...) puts the pixels of one edge.
// Fitted against PIL 12.2.0 on an 'L' image (tests/test_class_masks.py compares a host transcription of exactly
// these rules with the installed PIL, pixel for pixel).  Plain functions of integers and float32 with no contraction
// into FMA: the same text compiles for the device and, for checking, for the host.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CM_FN __host__ __device__ __forceinline__
#else
#define CM_FN static inline
#endif

// kind of an edge of the closed polygon v[k] -> v[k + 1 mod N]
enum { CM_ABSENT = 0, CM_FLAT = 1, CM_SLOPED = 2 };

struct CmEdge {
  int x0, y0;       // first vertex
  int ymin, ymax;   // rows it spans (CM_SLOPED), its row (CM_FLAT: ymin == ymax)
  int xmin, xmax;   // CM_FLAT: the span PIL draws for it
  float dx;         // (x1 - x0) / (y1 - y0) in float32
  int kind;
};

// PIL's ROUND_UP / ROUND_DOWN: a span runs from round-half-up(start) to round-half-down(end).  The float is kept
// inside the int range first (vertices that far out have no defined drawing; nothing may trap).
CM_FN int cm_round_up(float f) {
  f = fminf(fmaxf(f, -1073741824.f), 1073741824.f);
  return f >= 0.f ? (int)floorf(f + 0.5f) : -(int)floorf(fabsf(f) + 0.5f);
}
CM_FN int cm_round_down(float f) {
  f = fminf(fmaxf(f, -1073741824.f), 1073741824.f);
  return f >= 0.f ? (int)ceilf(f - 0.5f) : -(int)ceilf(fabsf(f) - 0.5f);
}

// Edge k of a polygon of N vertices p = (x, y) pairs.  PIL adds the closing edge only when the last vertex differs
// from the first; an edge between two equal vertices elsewhere is a flat edge of one pixel.
CM_FN CmEdge cm_make_edge(const int* p, int k, int N) {
  CmEdge e;
  const int j = k + 1 == N ? 0 : k + 1;
  const int x0 = p[2 * k], y0 = p[2 * k + 1], x1 = p[2 * j], y1 = p[2 * j + 1];
  e.x0 = x0; e.y0 = y0;
  e.xmin = x0 < x1 ? x0 : x1; e.xmax = x0 < x1 ? x1 : x0;
  e.ymin = y0 < y1 ? y0 : y1; e.ymax = y0 < y1 ? y1 : y0;
  e.dx = 0.f;
  if (k + 1 == N && x0 == x1 && y0 == y1) { e.kind = CM_ABSENT; return e; }
  if (y0 == y1) { e.kind = CM_FLAT; return e; }
  e.kind = CM_SLOPED;
  e.dx = (float)((long long)x1 - x0) / (float)((long long)y1 - y0);
  return e;
}

// x of a sloped edge on row y: (y - y0) * dx + x0, every step rounded to float32 (PIL's expression, no FMA).
CM_FN float cm_x_at(const CmEdge& e, int y) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fadd_rn(__fmul_rn((float)((long long)y - e.y0), e.dx), (float)e.x0);
#else
  volatile float m = (float)((long long)y - e.y0) * e.dx;
  return m + (float)e.x0;
#endif
}

// What edge k adds to the crossing list of row y.  `last_row` is the polygon's last scan line: max(0, largest y)
// cut at H (one past the canvas, as PIL has it).  Returns the number of values written to out (0, 1 or 2).
//   * an edge that ends on a row other than the last one gives its crossing twice;
//   * otherwise, at either end of an edge that is not vertical, the first earlier edge (table order, flat edges
//     left out) that is not vertical, ends on this row at the same end (both start here or both end here) and
//     crosses it in the same pixel decides: with a slope of the other sign nothing changes; with the same sign the
//     crossing is moved so that the row's span stops one pixel short of the adjacent row's (the next row, on the
//     last row the previous one), never inwards past the vertex.
template <typename EdgeAt>
CM_FN int cm_crossings(EdgeAt edge_at, int k, int y, int last_row, float out[2]) {
  const CmEdge e = edge_at(k);
  if (e.kind != CM_SLOPED || y < e.ymin || y > e.ymax) return 0;
  float x = cm_x_at(e, y);
  if (y == e.ymax && y < last_row) { out[0] = x; out[1] = x; return 2; }
  if ((y == e.ymin || y == e.ymax) && e.dx != 0.f) {
    for (int j = 0; j < k; ++j) {
      const CmEdge o = edge_at(j);
      if (o.kind != CM_SLOPED || o.dx == 0.f) continue;
      if (!((y == e.ymin && y == o.ymin) || (y == e.ymax && y == o.ymax))) continue;
      if (rintf(x) != rintf(cm_x_at(o, y))) continue;
      if ((e.dx > 0.f) == (o.dx > 0.f)) {
        const int adj = y == last_row ? y - 1 : y + 1;
        const float a = cm_x_at(e, adj), b = cm_x_at(o, adj);
        if ((y == e.ymax) != (e.dx > 0.f)) {                  // the span's end
          const float v = (float)(cm_round_up(fminf(a, b)) - 1);
          x = fmaxf(v, x);
        } else {                                              // the span's start
          const float v = (float)(cm_round_up(fmaxf(a, b)) + 1);
          x = fminf(v, x);
        }
      }
      break;
    }
  }
  out[0] = x;
  return 1;
}

// PIL's integer line from (x0, y0) to (x1, y1), both ends drawn: step t = 0 .. max(|dx|, |dy|) along the longer
// axis (y when they tie), the other coordinate advanced by floor((2 * dmin * t + dmaj) / (2 * dmaj)) -- the closed
// form of its error term, a tie going to the far side.  Returns the pixel of step t.  An edge between two equal
// vertices draws nothing (cm_line_steps is -1 for it): a polygon whose vertices are all one point has no outline.
CM_FN long long cm_line_steps(int x0, int y0, int x1, int y1) {
  const long long dx = (long long)x1 - x0, dy = (long long)y1 - y0;
  const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  return ax == 0 && ay == 0 ? -1 : (ax > ay ? ax : ay);
}
CM_FN void cm_line_pixel(int x0, int y0, int x1, int y1, long long t, int* px, int* py) {
  const long long dx = (long long)x1 - x0, dy = (long long)y1 - y0;
  const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
  if (ax > ay) {
    const long long m = (2 * ay * t + ax) / (2 * ax);
    *px = (int)(x0 + sx * t); *py = (int)(y0 + sy * m);
  } else {
    const long long m = ay == 0 ? 0 : (2 * ax * t + ay) / (2 * ay);
    *px = (int)(x0 + sx * m); *py = (int)(y0 + sy * t);
  }
}
