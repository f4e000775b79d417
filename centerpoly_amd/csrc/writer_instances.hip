// The Cityscapes writer's selection of one image on the device, for gfx950.
//
// CITYSCAPES.format_and_write_to_cityscapes (src/lib/datasets/dataset/cityscapes.py:196-283) turns the detections of an
// image into a depth-sorted instance list before it draws: rows above the threshold, every vertex through
// int(float("%.2f" % v)), a stable sort by depth, and per instance the label id, the confidence min(1, 1.2 score)
// and the "hides farther instances" rule.  cp_writer_instances does that on the rows cp_polydet_post_process left on
// the device and writes what cp_instance_masks and the evaluator read, so the detections need not pass through host
// Python between the network and the counting kernels.
//
// One launch of one workgroup: at most 1024 rows, one lane per row.  Every row's sort key (depth, class, row in one
// 64-bit word) lies in LDS; a live row's slot is the number of keys below its own (every lane walks the same LDS
// addresses, 16 bytes at a time, so the reads are broadcasts).  The polygons are then written slot-major by the whole
// workgroup, coalesced.
#include "cp_common.h"

namespace {

constexpr int kMaxRows = 1024;
constexpr int kMaxVerts = 64;
constexpr int kMaxClasses = 32;

struct InstArgs {
  const float* rows;          // [R][2N + 7]: x1,y1,x2,y2,score,cls,poly(2N),depth
  int* n_out;                 // [1]
  int* src;                   // [R]
  int* poly;                  // [R][N][2]
  unsigned char* flags;       // [R]
  int* label;                 // [R]
  float* conf;                // [R]
  float thresh;
  int R, N, C;
  int label_id[kMaxClasses];
  unsigned char has_masks[kMaxClasses];
};

// The three sort keys of a row in one word: the depth as an unsigned number of the same order (-0 and +0 equal, a NaN
// with +inf), the class, the row.  Keys of different rows differ, so "comes before" is one 64-bit comparison.
__device__ __forceinline__ unsigned long long sort_key(float depth, int cls, int row) {
  if (depth != depth) depth = __builtin_inff();                           // NaN sorts last: the order stays total
  if (depth == 0.f) depth = 0.f;
  unsigned u = __float_as_uint(depth);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned)(cls << 16) | (unsigned)row;
}

__global__ __launch_bounds__(kMaxRows) void writer_instances_kernel(InstArgs a) {
  __shared__ unsigned long long s_key[kMaxRows];                          // all ones: not live
  __shared__ int s_src[kMaxRows];                                         // slot -> row
  __shared__ int s_live;
  const int t = threadIdx.x;
  const int ncols = 2 * a.N + 7;
  if (t == 0) s_live = 0;
  float score = 0.f;
  int cls = -1;
  unsigned long long key = ~0ull;
  if (t < a.R) {
    const float* row = a.rows + (long long)t * ncols;
    score = row[4];
    const float c = row[5];
    const float depth = row[ncols - 1];
    const int ci = (c >= 0.f && c < (float)a.C) ? (int)c : -1;
    if (ci >= 0 && (float)ci == c && score > a.thresh) {
      cls = ci;
      key = sort_key(depth, cls, t);                                      // ascending depth, then class, then row:
    }                                                                     // the stable sort over `for cls ... for row`
  }
  s_key[t] = key;
  s_src[t] = -1;
  __syncthreads();
  if (cls >= 0) {
    int before = 0;
    const ulonglong2* keys = reinterpret_cast<const ulonglong2*>(s_key);
    for (int j = 0; j < a.R; j += 8) {                                    // (keys beyond R are dead: 1024 were written)
      ulonglong2 k[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) k[q] = keys[(j >> 1) + q];
#pragma unroll
      for (int q = 0; q < 4; ++q) before += (k[q].x < key ? 1 : 0) + (k[q].y < key ? 1 : 0);
    }
    s_src[before] = t;
    atomicAdd(&s_live, 1);
    a.src[before] = t;
    a.label[before] = a.label_id[cls];
    const float c12 = score * 1.2f;
    a.conf[before] = c12 < 1.0f ? c12 : 1.0f;
    a.flags[before] = (unsigned char)((a.has_masks[cls] ? 1 : 0) | (score >= 0.5f ? 2 : 0));
  }
  __syncthreads();
  const int n = s_live;
  if (t == 0) a.n_out[0] = n;
  if (t >= n && t < a.R) {                                                // dead slots: drawn by nobody
    a.src[t] = -1;
    a.label[t] = -1;
    a.conf[t] = 0.f;
    a.flags[t] = 0;
  }
  // the vertices, slot-major and coalesced; four gathers in flight per lane
  const int per = 2 * a.N, total = a.R * per;
  for (int k0 = t; k0 < total; k0 += 4 * kMaxRows) {
    float v[4];
    bool live[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + q * kMaxRows;
      live[q] = false;
      v[q] = 0.f;
      if (k < total) {
        const int slot = k / per, r = s_src[slot];
        live[q] = r >= 0;
        if (r >= 0) v[q] = a.rows[(long long)r * ncols + 6 + (k - slot * per)];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + q * kMaxRows;
      if (k < total) a.poly[k] = live[q] ? cp_vertex_int(v[q]) : 0;
    }
  }
}

}  // namespace

extern "C" int cp_writer_instances(const float* rows, int32_t R, int32_t N, float thresh, const int32_t* class_table,
                                   int32_t C, int32_t* n_out, int32_t* src, int32_t* poly, uint8_t* flags,
                                   int32_t* label, float* conf, void* stream) {
  CP_CHECK_ARG(R >= 1 && N >= 3 && C >= 1);
  if (R > kMaxRows || N > kMaxVerts || C > kMaxClasses) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(rows && class_table && n_out && src && poly && flags && label && conf);
  CP_CHECK_ARG(thresh == thresh);
  InstArgs a;
  a.rows = rows; a.n_out = n_out; a.src = src; a.poly = poly; a.flags = flags; a.label = label; a.conf = conf;
  a.thresh = thresh; a.R = R; a.N = N; a.C = C;
  for (int k = 0; k < kMaxClasses; ++k) {
    a.label_id[k] = k < C ? class_table[2 * k] : -1;
    a.has_masks[k] = k < C && class_table[2 * k + 1] != 0;
  }
  hipLaunchKernelGGL(writer_instances_kernel, dim3(1), dim3(kMaxRows), 0, (hipStream_t)stream, a);
  return cp_launch_status();
}
