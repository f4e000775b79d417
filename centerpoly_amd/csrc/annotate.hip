// Training annotations from ground truth for gfx950: the "regular interval" recipe of the reference's offline tools
// (KITTIPolyStuff/Tools/create_annotations.py, cityscapesStuff/Tools/create_bouding_box_annotations.py method
// regular_interval, IDDStuff/Tools/create_annotations.py) on the device.
//
// For one object with box (x0, y0, x1, y1), a mask on the image's canvas and N vertices the tools
//   put N / 4 points on every side of the box, round(x0 + i * ((x1 - x0) / (N / 4))) and so on in float64,
//   take the centre int(x0 + (x1 - x0) / 2), int(y0 + (y1 - y0) / 2),
//   walk the `bresenham` package's line from every box point to the centre, every pixel clipped to the canvas, and
//   keep the first pixel whose mask is set -- the clipped centre when there is none.
// The mask is `ids == v` of a 16-bit instance image (KITTI) or ImageDraw.polygon(pts, outline=0, fill=255) of the
// object's own ground-truth polygon (Cityscapes, IDD): a full-canvas image and N Python line walks per object there.
//
//   cp_annot_id_instances  one pass over the id image, a run of 16 pixels per lane, integer min / max atomics into a
//                          box table of 65536 entries (a plain read first: a bound that cannot improve the table is
//                          not sent); one workgroup then compacts the table in ascending value.
//   cp_polygon_masks       F \ O of class_masks.hip for polygons of up to 4096 vertices, the workgroup form of
//                          scanline.h: the edges once into the workspace; one workgroup per (polygon, row) collects
//                          the row's crossings in LDS, sorts them there and writes the spans; one lane per edge
//                          clears PIL's integer line; the counts.
//   cp_annot_rays_*        one wave per ray: 64 consecutive steps of the line per iteration from the closed form of
//                          the package's error term, a 64-bit ballot and its first set bit for the hit.
// Integers and correctly rounded float64 / float32 operations with no contraction: the same bits on every run.
#include "cp_common.h"
#include "scanline.h"

namespace {

constexpr int kMaxInst = 1024;                                            // objects of one id image, rays' boxes
constexpr int kMaxClasses = 32;
constexpr int kMaxPolys = 128;                                            // polygons of one cp_polygon_masks call
constexpr int kMaxPolyVerts = kSlMaxGroupVerts;
constexpr int kMaxRayVerts = 64;
constexpr int kIdValues = 65536;
constexpr int kRun = 16;                                                  // pixels of one lane in the id pass

// ---------------------------------------------------------------------------------------------- id instances ----

struct IdInstArgs {
  const unsigned short* ids;  // [H][W]
  int* table;                 // [65536][4]: xmin, ymin, xmax, ymax
  int* n_out;                 // [1]
  int* inst_id;               // [max_inst]
  int* cls;                   // [max_inst]
  int* box;                   // [max_inst][4]
  int H, W, C, divisor, max_inst;
  int label[kMaxClasses];
};

__device__ __forceinline__ int class_of(const IdInstArgs& a, int v) {
  const int lab = v / a.divisor;
  for (int c = 0; c < a.C; ++c)
    if (a.label[c] == lab) return c;
  return -1;
}

__global__ __launch_bounds__(256) void annot_table_init_kernel(int* table) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= kIdValues) return;
  table[4 * v + 0] = INT32_MAX; table[4 * v + 1] = INT32_MAX;
  table[4 * v + 2] = -1; table[4 * v + 3] = -1;
}

__device__ __forceinline__ int table_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void box_flush(int* table, int v, int xlo, int xhi, int y) {
  int* t = table + 4 * v;
  // the table only ever tightens, so a stale read can only send an atomic that was not needed
  if (table_load(t + 0) > xlo) atomicMin(t + 0, xlo);
  if (table_load(t + 1) > y) atomicMin(t + 1, y);
  if (table_load(t + 2) < xhi) atomicMax(t + 2, xhi);
  if (table_load(t + 3) < y) atomicMax(t + 3, y);
}

__global__ __launch_bounds__(256) void annot_id_boxes_kernel(IdInstArgs a) {
  const int runs_per_row = (a.W + kRun - 1) / kRun;
  const long long total = (long long)a.H * runs_per_row;
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < total; r += (long long)gridDim.x * 256) {
    const int y = (int)(r / runs_per_row), x0 = (int)(r - (long long)y * runs_per_row) * kRun;
    const int x1 = min(x0 + kRun, a.W);
    const unsigned short* row = a.ids + (long long)y * a.W;
    int cur = 0, lo = 0;
    for (int x = x0; x < x1; ++x) {
      const int v = row[x];
      if (v != cur) {
        if (cur != 0 && class_of(a, cur) >= 0) box_flush(a.table, cur, lo, x - 1, y);
        cur = v; lo = x;
      }
    }
    if (cur != 0 && class_of(a, cur) >= 0) box_flush(a.table, cur, lo, x1 - 1, y);
  }
}

// one workgroup: thread t owns the values 64 t .. 64 t + 63, an exclusive scan of the kept counts places them
__global__ __launch_bounds__(1024) void annot_id_compact_kernel(IdInstArgs a) {
  __shared__ int s_cnt[1024];
  const int t = threadIdx.x;
  int cnt = 0;
  for (int k = 0; k < 64; ++k) {
    const int v = t * 64 + k;
    if (v != 0 && a.table[4 * v + 3] >= 0 && class_of(a, v) >= 0) ++cnt;
  }
  s_cnt[t] = cnt;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {                                    // inclusive scan
    const int add = t >= o ? s_cnt[t - o] : 0;
    __syncthreads();
    s_cnt[t] += add;
    __syncthreads();
  }
  const int total = s_cnt[1023];
  int at = s_cnt[t] - cnt;
  for (int k = 0; k < 64; ++k) {
    const int v = t * 64 + k;
    if (v == 0 || a.table[4 * v + 3] < 0) continue;
    const int c = class_of(a, v);
    if (c < 0) continue;
    if (at < a.max_inst) {
      a.inst_id[at] = v;
      a.cls[at] = c;
      for (int q = 0; q < 4; ++q) a.box[4 * at + q] = a.table[4 * v + q];
    }
    ++at;
  }
  if (t == 0) a.n_out[0] = total;
  for (int s = t; s < a.max_inst; s += 1024)                              // dead slots
    if (s >= total) {
      a.inst_id[s] = 0;
      a.cls[s] = -1;
      for (int q = 0; q < 4; ++q) a.box[4 * s + q] = 0;
    }
}

// --------------------------------------------------------------------------------------------- polygon masks ----

struct PolyMaskArgs {
  const int* xy;              // [T][2]
  CmEdge* edges;              // [T] (workspace)
  int* yrange;                // [n][2]: smallest and largest y of the polygon (workspace)
  unsigned char* masks;       // [n][H][W]
  int* counts;                // [n]
  int n, H, W;
  int first[kMaxPolys + 1];
};

__global__ __launch_bounds__(256) void poly_edges_kernel(PolyMaskArgs a) {
  const int i = blockIdx.x, base = a.first[i];
  sl_group_edges(a.xy + 2ll * base, a.first[i + 1] - base, a.edges + base, a.yrange + 2 * i);
}

// One row of one polygon (sl_group_row).  The masks were zeroed before: only spans are written.
__global__ __launch_bounds__(256) void poly_fill_kernel(PolyMaskArgs a) {
  __shared__ float s_x[2 * kMaxPolyVerts];
  __shared__ int s_n;
  const int i = blockIdx.y, y = blockIdx.x;
  const int ylo = a.yrange[2 * i], yhi = a.yrange[2 * i + 1];
  if (y < ylo || y > yhi) return;                                         // uniform in the workgroup
  const int base = a.first[i], N = a.first[i + 1] - base;
  const CmEdge* edges = a.edges + base;
  const int last_row = min(max(yhi, 0), a.H);
  unsigned char* row = a.masks + ((long long)i * a.H + y) * a.W;
  sl_group_row(edges, N, y, last_row, a.W, s_x, &s_n, [&](int x) { row[x] = 255; });
}

// PIL's integer line of every edge, the part on the canvas, cleared (outline=0 after fill=255)
__global__ __launch_bounds__(64) void poly_outline_kernel(PolyMaskArgs a) {
  const int i = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
  const int base = a.first[i], N = a.first[i + 1] - base;
  if (k >= N) return;
  const int* p = a.xy + 2ll * base;
  const int j = k + 1 == N ? 0 : k + 1;
  const int x0 = p[2 * k], y0 = p[2 * k + 1], x1 = p[2 * j], y1 = p[2 * j + 1];
  unsigned char* mk = a.masks + (long long)i * a.H * a.W;
  sl_line_clipped(x0, y0, x1, y1, a.W, a.H, [&](long long at) { mk[at] = 0; });
}

__global__ __launch_bounds__(256) void poly_count_kernel(PolyMaskArgs a) {
  __shared__ int s_c[4];
  const int i = blockIdx.y, t = threadIdx.x;
  const long long HW = (long long)a.H * a.W;
  const unsigned char* mk = a.masks + (long long)i * HW;
  int c = 0;
  for (long long p0 = ((long long)blockIdx.x * 256 + t) * 8; p0 < HW; p0 += (long long)gridDim.x * 2048) {
    if (p0 + 8 <= HW) {
      unsigned long long v;
      __builtin_memcpy(&v, mk + p0, 8);                                   // any alignment
      c += __popcll(v & 0x0101010101010101ull);
    } else {
      for (long long q = p0; q < HW; ++q) c += mk[q] != 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((t & 63) == 0) s_c[t >> 6] = c;
  __syncthreads();
  if (t == 0) {
    const int sum = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    if (sum) atomicAdd(&a.counts[i], sum);
  }
}

// ------------------------------------------------------------------------------------------------------ rays ----

struct RayArgs {
  const unsigned short* ids;  // [H][W], or null
  const int* inst_id;         // [n] with ids
  const unsigned char* masks; // [n][H][W], or null
  const double* box;          // [n][4]
  int* poly;                  // [n][N][2]
  int n, N, H, W;
};

// int() of a float64 the tools hold, kept where the line's arithmetic cannot overflow (and a NaN at 0)
__device__ __forceinline__ long long ray_int(double v) {
  if (v != v) return 0;
  return (long long)fmin(fmax(v, -536870912.0), 536870912.0);
}

template <bool kIds>
__global__ __launch_bounds__(256) void annot_rays_kernel(RayArgs a) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= a.n * a.N) return;                                             // uniform in the wave
  const int i = r / a.N, j = r - i * a.N;
  const double x0 = a.box[4 * i], y0 = a.box[4 * i + 1], x1 = a.box[4 * i + 2], y1 = a.box[4 * i + 3];
  const int per = a.N / 4, side = j / per;
  const double f = (double)(j - side * per);
  const double qx = (x1 - x0) / (double)per, qy = (y1 - y0) / (double)per;
  // find_points_from_box: round() is half-to-even on fl(x0 + fl(i * q)); this file is compiled without contraction
  // top and right run forwards from (x0, y0), bottom and left backwards from (x1, y1); a - b is a + (-b) exactly.
  // Written as selects: the four-armed if-chain lost the left side's `bx = x0` in hipcc's control-flow lowering.
  const bool along_x = (side & 1) == 0, forwards = side < 2;
  const double start = along_x ? (forwards ? x0 : x1) : (forwards ? y0 : y1);
  const double step = f * (along_x ? qx : qy);
  const double moved = rint(start + (forwards ? step : -step));
  const double bx = along_x ? moved : (side == 1 ? x1 : x0);
  const double by = along_x ? (side == 0 ? y0 : y1) : moved;
  const long long sx = ray_int(bx), sy = ray_int(by);
  const long long cx = ray_int(x0 + (x1 - x0) / 2.0), cy = ray_int(y0 + (y1 - y0) / 2.0);
  // the package's walk: x-major when |dx| > |dy|; step t has advanced the minor axis by floor((2 d t + D) / (2 D))
  const long long dx = cx - sx, dy = cy - sy;
  const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  const long long xsign = dx > 0 ? 1 : -1, ysign = dy > 0 ? 1 : -1;
  const bool xmajor = adx > ady;
  const long long D = xmajor ? adx : ady, d = xmajor ? ady : adx;
  const long long HW = (long long)a.H * a.W;
  const int want = kIds ? a.inst_id[i] : 0;
  int rx = (int)min(max(cx, 0ll), (long long)a.W - 1), ry = (int)min(max(cy, 0ll), (long long)a.H - 1);
  for (long long t0 = 0; t0 <= D; t0 += 64) {
    const long long t = t0 + lane;
    bool hit = false;
    int px = 0, py = 0;
    if (t <= D) {
      const long long m = D == 0 ? 0 : (2 * d * t + D) / (2 * D);
      const long long ux = xmajor ? sx + xsign * t : sx + xsign * m;
      const long long uy = xmajor ? sy + ysign * m : sy + ysign * t;
      px = (int)min(max(ux, 0ll), (long long)a.W - 1);
      py = (int)min(max(uy, 0ll), (long long)a.H - 1);
      const long long at = (long long)py * a.W + px;
      hit = kIds ? (int)a.ids[at] == want : a.masks[(long long)i * HW + at] > 0;
    }
    const unsigned long long hits = __ballot(hit);
    if (hits) {
      const int src = __ffsll((long long)hits) - 1;
      rx = __shfl(px, src, 64);
      ry = __shfl(py, src, 64);
      break;
    }
  }
  if (lane == 0) {
    a.poly[2 * r] = rx;
    a.poly[2 * r + 1] = ry;
  }
}

int rays_check(const void* src, const double* box, int n, int N, int H, int W, const int* poly) {
  CP_CHECK_ARG(n >= 0 && N >= 4 && N % 4 == 0 && H > 0 && W > 0);
  if (n > kMaxInst || N > kMaxRayVerts || (long long)H * W >= (1ll << 31)) return CP_EUNSUPPORTED;
  if (n == 0) return CP_OK;
  CP_CHECK_ARG(src && box && poly);
  return CP_OK;
}

}  // namespace

extern "C" size_t cp_annot_id_instances_workspace_bytes(void) { return (size_t)kIdValues * 4 * sizeof(int); }

extern "C" int cp_annot_id_instances(const uint16_t* ids, int32_t H, int32_t W, const int32_t* class_label, int32_t C,
                                     int32_t divisor, int32_t max_inst, int32_t* n_out, int32_t* inst_id,
                                     int32_t* cls, int32_t* box, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  CP_CHECK_ARG(H > 0 && W > 0 && C >= 1 && divisor >= 1 && max_inst >= 1);
  if (C > kMaxClasses || max_inst > kMaxInst || (long long)H * W >= (1ll << 31)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(ids && class_label && n_out && inst_id && cls && box && workspace);
  if (workspace_bytes < cp_annot_id_instances_workspace_bytes()) return CP_EWORKSPACE;
  IdInstArgs a;
  a.ids = ids; a.table = (int*)workspace; a.n_out = n_out; a.inst_id = inst_id; a.cls = cls; a.box = box;
  a.H = H; a.W = W; a.C = C; a.divisor = divisor; a.max_inst = max_inst;
  for (int k = 0; k < kMaxClasses; ++k) a.label[k] = k < C ? class_label[k] : -1;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(annot_table_init_kernel, dim3(kIdValues / 256), dim3(256), 0, st, a.table);
  const long long runs = (long long)H * ((W + kRun - 1) / kRun);
  const long long blocks = (runs + 255) / 256;
  hipLaunchKernelGGL(annot_id_boxes_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(annot_id_compact_kernel, dim3(1), dim3(1024), 0, st, a);
  return cp_launch_status();
}

extern "C" size_t cp_polygon_masks_workspace_bytes(int32_t n, int32_t total_vertices) {
  if (n < 0 || total_vertices < 0) return 0;
  return cp_align_up((size_t)total_vertices * sizeof(CmEdge), 16) + (size_t)n * 2 * sizeof(int);
}

extern "C" int cp_polygon_masks(const int32_t* xy, const int32_t* first, int32_t n, int32_t H, int32_t W,
                                uint8_t* masks, int32_t* counts, void* workspace, size_t workspace_bytes,
                                void* stream) {
  CP_CHECK_ARG(n >= 0 && H > 0 && W > 0);
  if (n > kMaxPolys || (long long)H * W >= (1ll << 31)) return CP_EUNSUPPORTED;
  if (n == 0) return CP_OK;
  CP_CHECK_ARG(xy && first && masks && counts && workspace);
  CP_CHECK_ARG(first[0] == 0);
  int longest = 0;
  for (int i = 0; i < n; ++i) {
    const long long len = (long long)first[i + 1] - first[i];
    CP_CHECK_ARG(len >= 3);
    if (len > kMaxPolyVerts) return CP_EUNSUPPORTED;
    longest = len > longest ? (int)len : longest;
  }
  const int T = first[n];
  if (workspace_bytes < cp_polygon_masks_workspace_bytes(n, T)) return CP_EWORKSPACE;
  PolyMaskArgs a;
  a.xy = xy; a.edges = (CmEdge*)workspace;
  a.yrange = (int*)((char*)workspace + cp_align_up((size_t)T * sizeof(CmEdge), 16));
  a.masks = masks; a.counts = counts; a.n = n; a.H = H; a.W = W;
  for (int i = 0; i <= kMaxPolys; ++i) a.first[i] = first[i < n ? i : n];
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(masks, 0, (size_t)n * H * W, st);
  (void)hipMemsetAsync(counts, 0, (size_t)n * sizeof(int), st);
  hipLaunchKernelGGL(poly_edges_kernel, dim3(n), dim3(256), 0, st, a);
  hipLaunchKernelGGL(poly_fill_kernel, dim3(H, n), dim3(256), 0, st, a);
  hipLaunchKernelGGL(poly_outline_kernel, dim3((longest + 63) / 64, n), dim3(64), 0, st, a);
  const long long HW = (long long)H * W;
  const long long blocks = (HW + 2047) / 2048;
  hipLaunchKernelGGL(poly_count_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024), n), dim3(256), 0, st, a);
  return cp_launch_status();
}

extern "C" int cp_annot_rays_ids(const uint16_t* ids, int32_t H, int32_t W, const int32_t* inst_id, const double* box,
                                 int32_t n, int32_t N, int32_t* poly, void* stream) {
  const int rc = rays_check(ids, box, n, N, H, W, poly);
  if (rc != CP_OK || n == 0) return rc;
  CP_CHECK_ARG(inst_id);
  RayArgs a;
  a.ids = ids; a.inst_id = inst_id; a.masks = nullptr; a.box = box; a.poly = poly;
  a.n = n; a.N = N; a.H = H; a.W = W;
  hipLaunchKernelGGL(annot_rays_kernel<true>, dim3((n * N + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  return cp_launch_status();
}

extern "C" int cp_annot_rays_masks(const uint8_t* masks, int32_t H, int32_t W, const double* box, int32_t n, int32_t N,
                                   int32_t* poly, void* stream) {
  const int rc = rays_check(masks, box, n, N, H, W, poly);
  if (rc != CP_OK || n == 0) return rc;
  RayArgs a;
  a.ids = nullptr; a.inst_id = nullptr; a.masks = masks; a.box = box; a.poly = poly;
  a.n = n; a.N = N; a.H = H; a.W = W;
  hipLaunchKernelGGL(annot_rays_kernel<false>, dim3((n * N + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
  return cp_launch_status();
}
