// The KITTI and IDD writers' selection of one image on the device, for gfx950.
//
// format_and_write_to_kitti / format_and_write_to_IDD (src/lib/datasets/dataset/kitti_poly.py:95-136, IDD.py:123-170)
// walk the classes in turn: the rows of a class above the threshold get a text line each, in row order, numbered by
// one counter that runs through the whole image, and are then drawn in ascending depth.  cp_class_writer_instances
// does that on the rows cp_polydet_post_process left on the device and writes what cp_class_instance_masks and the
// evaluator read: the instances in drawing order (class, depth, row), each with the index of its text line (class,
// row), its group (the class), label id, the raw score and the "hides farther instances of its class" bit.
//
// One launch of one workgroup, the shape of writer_instances.hip: at most 1024 rows, one lane per row, both keys of
// every row in LDS, a live row's two ranks counted from broadcast reads, the polygons written slot-major.
#include "cp_common.h"

namespace {

constexpr int kMaxRows = 1024;
constexpr int kMaxVerts = 64;
constexpr int kMaxClasses = 32;

struct ClassInstArgs {
  const float* rows;          // [R][2N + 7]: x1,y1,x2,y2,score,cls,poly(2N),depth
  int* n_out;                 // [1]
  int* src;                   // [R]
  int* poly;                  // [R][N][2]
  int* group;                 // [R]
  unsigned char* flags;       // [R]
  int* label;                 // [R]
  float* conf;                // [R]
  int* text_index;            // [R]
  float thresh;
  int at_threshold;           // 0: score > thresh (KITTI), 1: score >= thresh (IDD)
  int R, N, C;
  int label_id[kMaxClasses];
};

// class, depth (as an unsigned number of the same order: -0 and +0 equal, a NaN with +inf), row: keys of different
// rows differ, so "is drawn before" is one 64-bit comparison and the sort is the stable one of the host loop.
__device__ __forceinline__ unsigned long long draw_key(int cls, float depth, int row) {
  if (depth != depth) depth = __builtin_inff();
  if (depth == 0.f) depth = 0.f;
  unsigned u = __float_as_uint(depth);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)cls << 42) | ((unsigned long long)u << 10) | (unsigned)row;
}

__global__ __launch_bounds__(kMaxRows) void class_writer_instances_kernel(ClassInstArgs a) {
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
    const int ci = (c >= 0.f && c < (float)a.C) ? (int)c : -1;
    const bool above = a.at_threshold ? score >= a.thresh : score > a.thresh;
    if (ci >= 0 && (float)ci == c && above) {
      cls = ci;
      key = draw_key(cls, row[ncols - 1], t);
    }
  }
  s_key[t] = key;
  s_src[t] = -1;
  __syncthreads();
  if (cls >= 0) {
    // slot: keys below this one.  text line: live rows of an earlier class, or of this class and an earlier row
    // (the class is the key's top, the row its bottom: rows are walked in order, so "earlier row" is j < t).
    int before = 0, text = 0;
    const unsigned long long cls_lo = (unsigned long long)cls << 42, cls_hi = (unsigned long long)(cls + 1) << 42;
    const ulonglong2* keys = reinterpret_cast<const ulonglong2*>(s_key);
    for (int j = 0; j < a.R; j += 2) {                                    // (keys beyond R are dead: 1024 were written)
      const ulonglong2 k = keys[j >> 1];
      before += (k.x < key ? 1 : 0) + (k.y < key ? 1 : 0);
      text += (k.x < cls_lo || (k.x < cls_hi && j < t) ? 1 : 0) + (k.y < cls_lo || (k.y < cls_hi && j + 1 < t) ? 1 : 0);
    }
    s_src[before] = t;
    atomicAdd(&s_live, 1);
    a.src[before] = t;
    a.group[before] = cls;
    a.label[before] = a.label_id[cls];
    a.conf[before] = score;
    a.text_index[before] = text;
    a.flags[before] = (unsigned char)(1 | (score >= 0.5f ? 2 : 0));
  }
  __syncthreads();
  const int n = s_live;
  if (t == 0) a.n_out[0] = n;
  if (t >= n && t < a.R) {                                                // dead slots: drawn by nobody
    a.src[t] = -1;
    a.group[t] = -1;
    a.label[t] = -1;
    a.conf[t] = 0.f;
    a.text_index[t] = -1;
    a.flags[t] = 0;
  }
  // the vertices, slot-major and coalesced
  const int per = 2 * a.N, total = a.R * per;
  for (int k = t; k < total; k += kMaxRows) {
    const int slot = k / per, r = s_src[slot];
    a.poly[k] = r >= 0 ? cp_vertex_int(a.rows[(long long)r * ncols + 6 + (k - slot * per)]) : 0;
  }
}

}  // namespace

extern "C" int cp_class_writer_instances(const float* rows, int32_t R, int32_t N, float thresh, int32_t at_threshold,
                                         const int32_t* class_label, int32_t C, int32_t* n_out, int32_t* src,
                                         int32_t* poly, int32_t* group, uint8_t* flags, int32_t* label, float* conf,
                                         int32_t* text_index, void* stream) {
  CP_CHECK_ARG(R >= 1 && N >= 3 && C >= 1 && (at_threshold == 0 || at_threshold == 1));
  if (R > kMaxRows || N > kMaxVerts || C > kMaxClasses) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(rows && class_label && n_out && src && poly && group && flags && label && conf && text_index);
  CP_CHECK_ARG(thresh == thresh);
  ClassInstArgs a;
  a.rows = rows; a.n_out = n_out; a.src = src; a.poly = poly; a.group = group; a.flags = flags; a.label = label;
  a.conf = conf; a.text_index = text_index; a.thresh = thresh; a.at_threshold = at_threshold;
  a.R = R; a.N = N; a.C = C;
  for (int k = 0; k < kMaxClasses; ++k) a.label_id[k] = k < C ? class_label[k] : -1;
  hipLaunchKernelGGL(class_writer_instances_kernel, dim3(1), dim3(kMaxRows), 0, (hipStream_t)stream, a);
  return cp_launch_status();
}
