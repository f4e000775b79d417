// Run-length masks ("run-length masks" in centerpoly_hip.h) for gfx950: COCO's column-major RLE of device masks, encoded
// to counts and to the compressed string on the device, and decoded back to planes.  Nothing is read back in between.
//
// Encoder, six launches whatever n is.  The unit of work is an ENTRY: (mask k, column x, row segment s), kSeg segments
// per column, in column-major order e = (k * W + x) * kSeg + s, so the changes of a mask in entry order are its changes
// in pixel order.  A workgroup is a tile of 64 columns, one wave per segment, one lane per column: the wave reads 64
// neighbouring bytes of a row and every lane walks down its column.
//   rle_count_kernel   walk 1: per entry the number of changes and its last three change positions
//   rle_scan_hist      one workgroup per mask: exclusive scan over the entries with the operator "add the counts, keep
//                      the last three positions" -- every entry then knows its rank and the three positions before it,
//                      which is all a count (a difference of positions) and its delta against cnts[i-2] need
//   rle_len_kernel     walk 2: per entry the characters its numbers take and the area of its odd counts
//   rle_scan_sum       one workgroup per mask: exclusive scan of the characters, totals of both
//   rle_finish_kernel  one workgroup: the closing count of every mask, the offsets over the masks, table and head
//   rle_emit_kernel    walk 3: counts and characters to their places, each store checked against its capacity
// The lengths do not go through stored positions, so table and head are complete however small the capacities are.
// With bounds a walk touches the box only (plus column x1 + 1 and, for a box on the bottom row, the rows above it,
// which cost no loads), and so do the entry tables: the scans run over the entries of the box's columns and nothing
// outside them is written or read.  Walks 2 and 3 skip entries without a change.  Vector stores only, no atomics: the same bits on
// every run.
//
// Decoder, two launches: rle_ends_kernel (one workgroup per mask: inclusive scan of the counts in 64 bits, the status)
// and rle_fill_kernel (same tiles; every lane finds its first run by binary search and walks down, so a wave's stores
// of a row are 64 neighbouring bytes).
#include "cp_common.h"

namespace {

constexpr int kSeg = 8;                                  // row segments per column = waves per walking workgroup
constexpr int kWalkThreads = CP_WAVE * kSeg;
constexpr int kRows = 8;                                  // rows a lane loads before it looks at them
constexpr int kScanThreads = 1024, kScanWaves = kScanThreads / CP_WAVE;
constexpr int kMaxPlanes = 128, kMaxIndex = 255, kMaxDecode = 255;
constexpr int kRecs = 256;                               // per-mask records in the workspace

struct Hist { unsigned cnt, h0, h1, h2; };               // changes; the last, the one before, the one before that
struct Sum2 { unsigned bytes, area; };

// a earlier, b later
__device__ __forceinline__ Hist merge(Hist a, Hist b) {
  Hist r;
  r.cnt = a.cnt + b.cnt;
  if (b.cnt >= 3) { r.h0 = b.h0; r.h1 = b.h1; r.h2 = b.h2; }
  else if (b.cnt == 2) { r.h0 = b.h0; r.h1 = b.h1; r.h2 = a.h0; }
  else if (b.cnt == 1) { r.h0 = b.h0; r.h1 = a.h0; r.h2 = a.h1; }
  else { r.h0 = a.h0; r.h1 = a.h1; r.h2 = a.h2; }
  return r;
}
__device__ __forceinline__ Sum2 merge(Sum2 a, Sum2 b) { return Sum2{a.bytes + b.bytes, a.area + b.area}; }
__device__ __forceinline__ unsigned long long merge(unsigned long long a, unsigned long long b) { return a + b; }

__device__ __forceinline__ Hist shfl_up(Hist v, int o) {
  return Hist{__shfl_up(v.cnt, o, CP_WAVE), __shfl_up(v.h0, o, CP_WAVE), __shfl_up(v.h1, o, CP_WAVE),
              __shfl_up(v.h2, o, CP_WAVE)};
}
__device__ __forceinline__ Sum2 shfl_up(Sum2 v, int o) {
  return Sum2{__shfl_up(v.bytes, o, CP_WAVE), __shfl_up(v.area, o, CP_WAVE)};
}
__device__ __forceinline__ unsigned long long shfl_up(unsigned long long v, int o) { return __shfl_up(v, o, CP_WAVE); }

// Scan of one value per thread over a workgroup of kScanThreads: the merge of all values before the thread's, and of
// all.  lds: kScanWaves values, free again after the call's second barrier (the first one guards the call before).
template <class T>
__device__ __forceinline__ void block_scan(T v, T& excl, T& total, T* lds) {
  const int lane = threadIdx.x & (CP_WAVE - 1), w = threadIdx.x / CP_WAVE;
  T inc = v;
#pragma unroll
  for (int o = 1; o < CP_WAVE; o <<= 1) {
    const T t = shfl_up(inc, o);
    if (lane >= o) inc = merge(t, inc);
  }
  T before = shfl_up(inc, 1);
  if (lane == 0) before = T{};
  __syncthreads();
  if (lane == CP_WAVE - 1) lds[w] = inc;
  __syncthreads();
  T wp{}, tot{};
  for (int j = 0; j < kScanWaves; ++j) {
    const T t = lds[j];
    if (j < w) wp = merge(wp, t);
    tot = merge(tot, t);
  }
  excl = merge(wp, before);
  total = tot;
}

// characters of one number of the string
__device__ __forceinline__ int rle_len(int x) {
  int n = 0;
  bool more;
  do {
    const int c = x & 0x1f;
    x >>= 5;
    more = (c & 0x10) ? x != -1 : x != 0;
    ++n;
  } while (more);
  return n;
}

// the characters of x at chars[at ..], none at or beyond cap
__device__ __forceinline__ void rle_put(int x, uint8_t* __restrict__ chars, long long at, long long cap) {
  bool more;
  do {
    int c = x & 0x1f;
    x >>= 5;
    more = (c & 0x10) ? x != -1 : x != 0;
    if (more) c |= 0x20;
    if (at < cap) chars[at] = (uint8_t)(c + 48);
    ++at;
  } while (more);
}

struct Src {
  const uint8_t* planes;      // [n][H][W] or null
  const uint8_t* index;       // [H][W] or null
  const int* bounds;          // [n][4] or null
  int n, H, W;
};

struct Box {
  int x0, y0, x1, y1;         // the mask's box, clipped; x0 = W, x1 = -1 when empty
  int cx1;                    // the last column of the work: x1 + 1 where it exists
  int ry0, ry1;               // the rows of the work, inclusive
};

__device__ __forceinline__ Box load_box(const Src& q, int k) {
  Box b;
  b.x0 = 0; b.y0 = 0; b.x1 = q.W - 1; b.y1 = q.H - 1;
  if (q.bounds) {
    b.x0 = max(q.bounds[4 * k], 0); b.y0 = max(q.bounds[4 * k + 1], 0);
    b.x1 = min(q.bounds[4 * k + 2], q.W - 1); b.y1 = min(q.bounds[4 * k + 3], q.H - 1);
  }
  if (b.x1 < b.x0 || b.y1 < b.y0) {
    b.x0 = q.W; b.x1 = -1; b.cx1 = -1; b.y0 = 0; b.y1 = -1; b.ry0 = 0; b.ry1 = -1;
    return b;
  }
  b.cx1 = min(b.x1 + 1, q.W - 1);
  // a box on the bottom row carries a one into row 0 of the next column: the walk starts at row 0 then (the rows
  // above the box are read as zero without a load)
  b.ry0 = b.y1 == q.H - 1 ? 0 : b.y0;
  b.ry1 = min(b.y1 + 1, q.H - 1);
  return b;
}

// Calls on_change(j) for every change of mask k in column x, rows of segment s, in ascending j = x * H + y.
template <class F>
__device__ __forceinline__ void walk(const Src& q, int k, const Box& b, int x, int s, F&& on_change) {
  const int rows = b.ry1 - b.ry0 + 1, per = (rows + kSeg - 1) / kSeg;
  const int ya = b.ry0 + s * per, yb = min(ya + per, b.ry1 + 1);
  if (ya >= yb) return;
  const uint8_t* base = q.planes ? q.planes + (size_t)k * q.H * q.W : q.index;
  const bool by_index = q.planes == nullptr;
  auto val = [&](int y, int xx) -> int {
    if (xx < b.x0 || xx > b.x1 || y < b.y0 || y > b.y1) return 0;
    const int v = base[(size_t)y * q.W + xx];
    return by_index ? v == k : v != 0;
  };
  int prev = ya == 0 ? (x > 0 ? val(q.H - 1, x - 1) : 0) : val(ya - 1, x);
  const unsigned j0 = (unsigned)x * (unsigned)q.H;
  for (int y = ya; y < yb; y += kRows) {
    int u[kRows];
#pragma unroll
    for (int i = 0; i < kRows; ++i) u[i] = y + i < yb ? val(y + i, x) : -1;
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      if (u[i] >= 0 && u[i] != prev) {
        on_change(j0 + (unsigned)(y + i));
        prev = u[i];
      }
    }
  }
}

__device__ __forceinline__ size_t entry_of(const Src& q, int k, int x, int s) {
  return ((size_t)k * q.W + x) * kSeg + s;
}

__global__ __launch_bounds__(kWalkThreads) void rle_count_kernel(Src q, uint4* __restrict__ E) {
  const int k = blockIdx.y, x = blockIdx.x * CP_WAVE + (threadIdx.x & (CP_WAVE - 1)), s = threadIdx.x / CP_WAVE;
  if (x >= q.W) return;
  const Box b = load_box(q, k);
  if (x < b.x0 || x > b.cx1) return;                                      // (no entry outside the work: nobody reads it)
  Hist h{0, 0, 0, 0};
  walk(q, k, b, x, s, [&](unsigned p) { ++h.cnt; h.h2 = h.h1; h.h1 = h.h0; h.h0 = p; });
  E[entry_of(q, k, x, s)] = make_uint4(h.cnt, h.h0, h.h1, h.h2);
}

// the entries of the work's columns [x0, cx1] of mask k: the scans and the walks touch no other
__device__ __forceinline__ void entry_range(const Src& q, int k, long long& lo, long long& hi) {
  const Box b = load_box(q, k);
  lo = (long long)min(b.x0, q.W) * kSeg;
  hi = max((long long)(b.cx1 + 1) * kSeg, lo);
}

// in place: E[e] becomes the merge of the mask's entries before e; rec[k] the merge of all
__global__ __launch_bounds__(kScanThreads) void rle_scan_hist_kernel(Src q, uint4* __restrict__ E,
                                                                    Hist* __restrict__ rec) {
  __shared__ Hist lds[kScanWaves];
  long long lo, Ne;
  entry_range(q, blockIdx.x, lo, Ne);
  uint4* e = E + (size_t)blockIdx.x * q.W * kSeg;
  Hist carry{0, 0, 0, 0};
  for (long long base = lo; base < Ne; base += kScanThreads) {
    const long long i = base + threadIdx.x;
    Hist v{0, 0, 0, 0};
    if (i < Ne) { const uint4 t = e[i]; v = Hist{t.x, t.y, t.z, t.w}; }
    Hist excl, total;
    block_scan(v, excl, total, lds);
    if (i < Ne) { const Hist r = merge(carry, excl); e[i] = make_uint4(r.cnt, r.h0, r.h1, r.h2); }
    carry = merge(carry, total);
  }
  if (threadIdx.x == 0) rec[blockIdx.x] = carry;
}

// the entry's own number of changes from the scanned table
__device__ __forceinline__ unsigned entry_changes(const uint4* __restrict__ X, const Hist* __restrict__ rec, const Src& q,
                                                  const Box& b, int k, int x, int s, unsigned rank) {
  const bool last = x == b.cx1 && s == kSeg - 1;
  return (last ? rec[k].cnt : X[entry_of(q, k, x, s) + 1].x) - rank;
}

// One change at p of rank r with the history h: the count, its number in the string; then the history moves on.
struct Step { unsigned count; int number; };
__device__ __forceinline__ Step step(Hist& h, unsigned& r, unsigned p) {
  Step st;
  st.count = p - h.h0;
  st.number = (int)st.count - (r > 2 ? (int)(h.h1 - h.h2) : 0);
  h.h2 = h.h1; h.h1 = h.h0; h.h0 = p;
  ++r;
  return st;
}

__global__ __launch_bounds__(kWalkThreads) void rle_len_kernel(Src q, const uint4* __restrict__ X,
                                                              const Hist* __restrict__ rec, uint2* __restrict__ Y) {
  const int k = blockIdx.y, x = blockIdx.x * CP_WAVE + (threadIdx.x & (CP_WAVE - 1)), s = threadIdx.x / CP_WAVE;
  if (x >= q.W) return;
  const Box b = load_box(q, k);
  if (x < b.x0 || x > b.cx1) return;
  const uint4 t = X[entry_of(q, k, x, s)];
  unsigned bytes = 0, area = 0;
  if (entry_changes(X, rec, q, b, k, x, s, t.x) != 0) {
    Hist h{0, t.y, t.z, t.w};
    unsigned r = t.x;
    walk(q, k, b, x, s, [&](unsigned p) {
      const bool ones = r & 1;
      const Step st = step(h, r, p);
      bytes += rle_len(st.number);
      if (ones) area += st.count;
    });
  }
  Y[entry_of(q, k, x, s)] = make_uint2(bytes, area);
}

__global__ __launch_bounds__(kScanThreads) void rle_scan_sum_kernel(Src q, uint2* __restrict__ Y,
                                                                   Sum2* __restrict__ rec) {
  __shared__ Sum2 lds[kScanWaves];
  long long lo, Ne;
  entry_range(q, blockIdx.x, lo, Ne);
  uint2* e = Y + (size_t)blockIdx.x * q.W * kSeg;
  Sum2 carry{0, 0};
  for (long long base = lo; base < Ne; base += kScanThreads) {
    const long long i = base + threadIdx.x;
    Sum2 v{0, 0};
    if (i < Ne) { const uint2 t = e[i]; v = Sum2{t.x, t.y}; }
    Sum2 excl, total;
    block_scan(v, excl, total, lds);
    if (i < Ne) { const Sum2 r = merge(carry, excl); e[i] = make_uint2(r.bytes, r.area); }
    carry = merge(carry, total);
  }
  if (threadIdx.x == 0) rec[blockIdx.x] = carry;
}

__device__ __forceinline__ int clamp_i32(long long v) { return v > 2147483647LL ? 2147483647 : (int)v; }

// the closing count of mask k (rank = its number of changes): its value and its number in the string
__device__ __forceinline__ Step closing(const Hist& h, unsigned HW) {
  Step st;
  st.count = HW - h.h0;
  st.number = (int)st.count - (h.cnt > 2 ? (int)(h.h1 - h.h2) : 0);
  return st;
}

__global__ __launch_bounds__(CP_WAVE) void rle_finish_kernel(int n, unsigned HW, const Hist* __restrict__ recH,
                                                            const Sum2* __restrict__ recS, long long* __restrict__ off,
                                                            int* __restrict__ table, int* __restrict__ head,
                                                            long long cap_counts, long long cap_bytes, int have_counts) {
  if (threadIdx.x != 0) return;
  long long co = 0, bo = 0;
  for (int k = 0; k < n; ++k) {
    const Hist h = recH[k];
    const Step st = closing(h, HW);
    const long long m = (long long)h.cnt + 1, bytes = (long long)recS[k].bytes + rle_len(st.number);
    const long long area = (long long)recS[k].area + ((h.cnt & 1) ? st.count : 0);
    off[2 * k] = co; off[2 * k + 1] = bo;
    table[4 * k] = clamp_i32(m); table[4 * k + 1] = clamp_i32(area);
    table[4 * k + 2] = clamp_i32(bo); table[4 * k + 3] = clamp_i32(bytes);
    co += m; bo += bytes;
  }
  head[0] = clamp_i32(co); head[1] = clamp_i32(bo);
  head[2] = ((have_counts && co > cap_counts) || bo > cap_bytes) ? 1 : 0;
  head[3] = 0;
}

struct Out {
  uint32_t* counts;           // or null
  uint8_t* chars;
  long long cap_counts, cap_bytes;
};

__global__ __launch_bounds__(kWalkThreads) void rle_emit_kernel(Src q, const uint4* __restrict__ X,
                                                               const Hist* __restrict__ rec, const uint2* __restrict__ Y,
                                                               const Sum2* __restrict__ recS,
                                                               const long long* __restrict__ off, Out o) {
  const int k = blockIdx.y, x = blockIdx.x * CP_WAVE + (threadIdx.x & (CP_WAVE - 1)), s = threadIdx.x / CP_WAVE;
  if (x >= q.W) return;
  const long long co = off[2 * k], bo = off[2 * k + 1];
  if (x == 0 && s == 0) {                                                 // the closing count of the mask
    const Hist h = rec[k];
    const Step st = closing(h, (unsigned)q.H * (unsigned)q.W);
    if (o.counts && co + h.cnt < o.cap_counts) o.counts[co + h.cnt] = st.count;
    rle_put(st.number, o.chars, bo + recS[k].bytes, o.cap_bytes);
  }
  const Box b = load_box(q, k);
  if (x < b.x0 || x > b.cx1) return;
  const uint4 t = X[entry_of(q, k, x, s)];
  if (entry_changes(X, rec, q, b, k, x, s, t.x) == 0) return;
  Hist h{0, t.y, t.z, t.w};
  unsigned r = t.x;
  long long at = bo + Y[entry_of(q, k, x, s)].x;
  walk(q, k, b, x, s, [&](unsigned p) {
    const long long ci = co + r;
    const Step st = step(h, r, p);
    if (o.counts && ci < o.cap_counts) o.counts[ci] = st.count;
    rle_put(st.number, o.chars, at, o.cap_bytes);
    at += rle_len(st.number);
  });
}

// ---------------------------------------------------------------------------------------------------- decoder

struct DecTable {
  int off[kMaxDecode];
  int m[kMaxDecode];
};

__global__ __launch_bounds__(kScanThreads) void rle_ends_kernel(const uint32_t* __restrict__ counts, DecTable t,
                                                               unsigned HW, uint32_t* __restrict__ ends,
                                                               int* __restrict__ status) {
  __shared__ unsigned long long lds[kScanWaves];
  const int k = blockIdx.x, off = t.off[k], m = t.m[k];
  unsigned long long carry = 0;
  for (int base = 0; base < m; base += kScanThreads) {
    const int i = base + (int)threadIdx.x;
    const unsigned long long v = i < m ? counts[(size_t)off + i] : 0;
    unsigned long long excl, total;
    block_scan(v, excl, total, lds);
    if (i < m) {
      const unsigned long long end = carry + excl + v;
      ends[(size_t)off + i] = end > HW ? HW + 1u : (unsigned)end;         // (monotone; beyond the image: bad anyway)
    }
    carry += total;
  }
  if (threadIdx.x == 0) status[k] = carry != HW;
}

__global__ __launch_bounds__(kWalkThreads) void rle_fill_kernel(const uint32_t* __restrict__ ends, DecTable t, int H,
                                                               int W, int value, const int* __restrict__ status,
                                                               uint8_t* __restrict__ planes) {
  const int k = blockIdx.y, x = blockIdx.x * CP_WAVE + (threadIdx.x & (CP_WAVE - 1)), s = threadIdx.x / CP_WAVE;
  if (x >= W) return;
  const int per = (H + kSeg - 1) / kSeg, ya = s * per, yb = min(ya + per, H);
  if (ya >= yb) return;
  uint8_t* out = planes + (size_t)k * H * W + x;
  if (status[k]) {
    for (int y = ya; y < yb; ++y) out[(size_t)y * W] = 0;
    return;
  }
  const uint32_t* e = ends + t.off[k];
  const int m = t.m[k];
  unsigned j = (unsigned)x * (unsigned)H + (unsigned)ya;
  int lo = 0, hi = m - 1;                                                 // the first run that ends beyond j: it exists,
  while (lo < hi) {                                                       // the last one ends at H * W
    const int mid = (lo + hi) >> 1;
    if (e[mid] > j) hi = mid; else lo = mid + 1;
  }
  int i = lo;
  unsigned end = e[i];
  for (int y = ya; y < yb; ++y, ++j) {
    while (end <= j) end = e[++i];                                        // (runs of length zero pass here)
    out[(size_t)y * W] = (i & 1) ? (uint8_t)value : (uint8_t)0;
  }
}

size_t entries_of(int n, int W) { return (size_t)n * (size_t)W * kSeg; }
size_t encode_bytes(int n, int W) {
  return entries_of(n, W) * (sizeof(uint4) + sizeof(uint2)) + kRecs * (sizeof(Hist) + sizeof(Sum2) + 2 * sizeof(long long));
}

}  // namespace

extern "C" size_t cp_rle_encode_workspace_bytes(int32_t n, int32_t H, int32_t W, int64_t cap_counts) {
  if (n < 1 || n > kMaxIndex || H < 1 || W < 1 || cap_counts < 0) return 0;
  return encode_bytes(n, W);
}

extern "C" int cp_rle_encode(const uint8_t* planes, const uint8_t* index, int32_t n, int32_t H, int32_t W,
                             const int32_t* bounds, uint32_t* counts, int64_t cap_counts, uint8_t* chars,
                             int64_t cap_bytes, int32_t* table, int32_t* head, void* workspace, size_t workspace_bytes,
                             void* stream) {
  CP_CHECK_ARG(H > 0 && W > 0 && n >= 1 && cap_counts >= 0 && cap_bytes >= 0);
  CP_CHECK_ARG((planes != nullptr) != (index != nullptr));
  if (n > (planes ? kMaxPlanes : kMaxIndex) || (long long)H * W >= (1LL << 31)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(table && head && (chars || cap_bytes == 0));
  CP_CHECK_ARG(((uintptr_t)bounds & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)table & 3) == 0 &&
               ((uintptr_t)head & 3) == 0);
  if (!workspace || workspace_bytes < encode_bytes(n, W)) return CP_EWORKSPACE;
  CP_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
  hipStream_t st = (hipStream_t)stream;
  const size_t ne = entries_of(n, W);
  uint4* E = (uint4*)workspace;
  uint2* Y = (uint2*)(E + ne);
  Hist* recH = (Hist*)(Y + ne);
  long long* off = (long long*)(recH + kRecs);
  Sum2* recS = (Sum2*)(off + 2 * kRecs);
  Src q;
  q.planes = planes; q.index = index; q.bounds = bounds; q.n = n; q.H = H; q.W = W;
  Out o;
  o.counts = counts; o.chars = chars; o.cap_counts = counts ? cap_counts : 0; o.cap_bytes = chars ? cap_bytes : 0;
  const dim3 tiles((W + CP_WAVE - 1) / CP_WAVE, n);
  hipLaunchKernelGGL(rle_count_kernel, tiles, dim3(kWalkThreads), 0, st, q, E);
  hipLaunchKernelGGL(rle_scan_hist_kernel, dim3(n), dim3(kScanThreads), 0, st, q, E, recH);
  hipLaunchKernelGGL(rle_len_kernel, tiles, dim3(kWalkThreads), 0, st, q, E, recH, Y);
  hipLaunchKernelGGL(rle_scan_sum_kernel, dim3(n), dim3(kScanThreads), 0, st, q, Y, recS);
  hipLaunchKernelGGL(rle_finish_kernel, dim3(1), dim3(CP_WAVE), 0, st, n, (unsigned)H * (unsigned)W, recH, recS, off,
                     table, head, o.cap_counts, o.cap_bytes, counts ? 1 : 0);
  hipLaunchKernelGGL(rle_emit_kernel, tiles, dim3(kWalkThreads), 0, st, q, E, recH, Y, recS, off, o);
  return cp_launch_status();
}

extern "C" size_t cp_rle_decode_workspace_bytes(int32_t n, int64_t total_counts) {
  if (n < 1 || n > kMaxDecode || total_counts < 0) return 0;
  return cp_align_up((size_t)total_counts * sizeof(uint32_t), 16) + 16;
}

extern "C" int cp_rle_decode(const uint32_t* counts, const int32_t* table, int32_t n, int32_t H, int32_t W, int32_t value,
                             uint8_t* planes, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(H > 0 && W > 0 && n >= 1 && value >= 0 && value <= 255);
  if (n > kMaxDecode || (long long)H * W >= (1LL << 31)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(table && planes && status);
  CP_CHECK_ARG(((uintptr_t)counts & 3) == 0 && ((uintptr_t)status & 3) == 0);
  DecTable t;
  long long total = 0;
  for (int k = 0; k < kMaxDecode; ++k) {
    t.off[k] = k < n ? table[2 * k] : 0;
    t.m[k] = k < n ? table[2 * k + 1] : 0;
    CP_CHECK_ARG(t.off[k] >= 0 && t.m[k] >= 0);
    total = total > (long long)t.off[k] + t.m[k] ? total : (long long)t.off[k] + t.m[k];
  }
  CP_CHECK_ARG(counts || total == 0);
  if (!workspace || workspace_bytes < cp_rle_decode_workspace_bytes(n, total)) return CP_EWORKSPACE;
  CP_CHECK_ARG(((uintptr_t)workspace & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* ends = (uint32_t*)workspace;
  hipLaunchKernelGGL(rle_ends_kernel, dim3(n), dim3(kScanThreads), 0, st, counts, t, (unsigned)H * (unsigned)W, ends,
                     status);
  hipLaunchKernelGGL(rle_fill_kernel, dim3((W + CP_WAVE - 1) / CP_WAVE, n), dim3(kWalkThreads), 0, st, ends, t, H, W,
                     (int)value, status, planes);
  return cp_launch_status();
}
