// The merge of the test scales and soft-NMS on DEVICE rows, for gfx950.
//
// PolydetDetector.merge_outputs (reference: src/lib/detectors/polydet.py:62-76) with the soft_nms of
// external/nms.pyx:77-170, literal behaviour: per class the rows of every scale in order, soft-NMS in place on
// columns 0-4 only (the polygon and depth columns never move, the block keeps its length, the slots at and above
// the live count hold stale data and are part of the result), then the cut at the (total - max_per_image)-th
// smallest score with `>=`.  csrc/soft_nms.hip is the host statement of the same arithmetic; this file follows it
// operation for operation (float differences, `+ 1.0` and the products in double, no contraction).
//
// cp_soft_nms_device: ONE launch, one 64-lane wave per segment.  Columns 0-4 of the segment lie in LDS, column-major;
// the iterations of i run in wave lock-step.  Each iteration is a wave arg-max over [i, N) (strict <, the lowest
// position wins a tie), the swap, and the reference's inner `while` in two phases:
//   A (parallel)   every row of (i, N) decays once; its discard flag is set only inside the overlap branch
//   B (flags only) the hole-filling walk: a flagged position takes columns 0-4 and the flag of row N - 1, N shrinks,
//                  the position is looked at again.  The row moved from N - 1 decays AT pos in the sequential code, so
//                  the stale copy left at N - 1 gets its pre-decay score back unless pos == N - 1.
// The walk skips 64 positions per ballot and is not entered when phase A raised no flag.  The loop is a chain of
// latencies, so: the arg-max is a maximum of 64-bit keys (score, then lowest position) through DPP row operations, not
// LDS shuffles; phase A leaves the next iteration's keys behind (void once phase B moved rows); and phase A keeps up to
// four positions of a lane in flight, loads first, so that their float64 chains overlap.
//
// cp_merge_detections: THREE launches (two with nms == 0): a stable partition by class into the workspace (one
// workgroup; a ballot prefix count per class, no atomics), the soft-NMS kernel above with one wave per class, and the
// cut (one workgroup: the k-th smallest score by rank counting in LDS, a prefix sum of the keep flags, the copy).
// The class rule, the partition, the arg-max's order and the cut are row_merge.h's, shared with mask_nms.hip.
#include <math.h>

#include "cp_common.h"
#include "row_merge.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxRows = 4096;
constexpr int kMaxSegs = 64;
constexpr int kMaxClasses = 64;
constexpr int kThreads = row_merge::kThreads;
constexpr int kCutRows = kMaxRows / kThreads;                             // slots of the cut per thread

using row_merge::score_key;
using row_merge::wave_max_key;
using row_merge::wave_sync;

// bytes of LDS a segment of `cap` rows needs: columns 0-4, the pre-decay score, the flag
__host__ __device__ inline size_t nms_lds_bytes(int cap) { return (size_t)cap * (6 * sizeof(float) + 1); }

struct Decay {                // the segment in LDS and the parameters
  float *x1, *y1, *x2, *y2, *sc, *old;
  unsigned char* flag;
  float sigma, Nt, threshold;
  int method;
};

struct Top {                  // the box of row i and its area
  float x1, y1, x2, y2;
  double area;
};

// Phase A for positions base + q * 64 + lane, q < U: loads first, then U independent chains of the reference's
// arithmetic (a lane beyond N computes on row i and stores nothing), then the stores.  The weight is computed without
// the reference's branches and used only where they are taken; the whole batch skips it when no lane overlaps the box.
template <int U>
__device__ __forceinline__ void decay_batch(const Decay& d, const Top& t, int base, int N, int i, int lane, bool& any,
                                            unsigned long long& best) {
  float x1[U], y1[U], x2[U], y2[U], sc[U], area[U], iw[U], ih[U], ns[U];
  bool in[U], hit[U];
  bool some = false;
#pragma unroll
  for (int q = 0; q < U; ++q) {
    const int pos = base + q * CP_WAVE + lane;
    in[q] = pos < N;
    const int p = in[q] ? pos : i;
    x1[q] = d.x1[p]; y1[q] = d.y1[p]; x2[q] = d.x2[p]; y2[q] = d.y2[p]; sc[q] = d.sc[p];
  }
#pragma unroll
  for (int q = 0; q < U; ++q) {
    area[q] = (float)(((double)(x2[q] - x1[q]) + 1.0) * ((double)(y2[q] - y1[q]) + 1.0));
    iw[q] = (float)((double)((t.x2 <= x2[q] ? t.x2 : x2[q]) - (t.x1 >= x1[q] ? t.x1 : x1[q])) + 1.0);
    ih[q] = (float)((double)((t.y2 <= y2[q] ? t.y2 : y2[q]) - (t.y1 >= y1[q] ? t.y1 : y1[q])) + 1.0);
    hit[q] = in[q] && iw[q] > 0 && ih[q] > 0;
    ns[q] = sc[q];
    some = some || hit[q];
  }
  if (__ballot(some) != 0ull) {
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const float ua = (float)(t.area + (double)area[q] - (double)(iw[q] * ih[q]));
      const float ov = (iw[q] * ih[q]) / ua;
      float weight;
      if (d.method == 1) weight = ov > d.Nt ? (float)(1.0 - (double)ov) : 1.f;
      else if (d.method == 2) weight = (float)exp((double)(-(ov * ov) / d.sigma));
      else weight = ov > d.Nt ? 0.f : 1.f;
      if (hit[q]) ns[q] = weight * sc[q];
    }
  }
#pragma unroll
  for (int q = 0; q < U; ++q) {
    if (in[q]) {
      const int pos = base + q * CP_WAVE + lane;
      const bool f = hit[q] && ns[q] < d.threshold;
      d.sc[pos] = ns[q];
      d.old[pos] = sc[q];
      d.flag[pos] = f ? 1 : 0;
      any = any || f;
      const unsigned long long k = score_key(ns[q], pos);
      best = k > best ? k : best;
    }
  }
}

// soft_nms on the n rows whose columns 0-4 lie column-major in col[c * cap + r]; returns the live count
__device__ int soft_nms_wave(float* col, float* old, unsigned char* flag, int cap, int n, float sigma, float Nt,
                             float threshold, int method, int lane) {
  float* const sx1 = col;
  float* const sy1 = col + cap;
  float* const sx2 = col + 2 * cap;
  float* const sy2 = col + 3 * cap;
  float* const ssc = col + 4 * cap;
  const Decay d = {sx1, sy1, sx2, sy2, ssc, old, flag, sigma, Nt, threshold, method};
  int N = n;
  bool have = false;                                                      // `best` holds this lane's part of the arg-max
  unsigned long long best = 0ull;
  for (int i = 0; i < N - 1; ++i) {                                       // i >= N - 1: the iteration is a no-op
    // arg-max over [i, N): the largest key is the highest score at its lowest position (strict <, as the reference scans)
    if (!have) {
      best = 0ull;
      for (int pos = i + lane; pos < N; pos += CP_WAVE) {
        const unsigned long long k = score_key(ssc[pos], pos);
        best = k > best ? k : best;
      }
    }
    int maxpos = (int)(0xffffffffu - (unsigned)wave_max_key(best));
    if (maxpos < i || maxpos >= N) maxpos = i;                            // (a NaN score: stay inside the segment)
    if (lane < 5 && maxpos != i) {
      float* const c = col + lane * cap;
      const float t = c[i];
      c[i] = c[maxpos];
      c[maxpos] = t;
    }
    wave_sync();
    const float tx1 = sx1[i], ty1 = sy1[i], tx2 = sx2[i], ty2 = sy2[i];
    const Top top = {tx1, ty1, tx2, ty2, ((double)(tx2 - tx1) + 1.0) * ((double)(ty2 - ty1) + 1.0)};
    // phase A, up to four positions of a lane in flight; it leaves the next iteration's arg-max keys in `best`
    bool any = false;
    best = 0ull;
    for (int base = i + 1; base < N; base += 4 * CP_WAVE) {
      const int left = N - base;
      if (left > 2 * CP_WAVE) decay_batch<4>(d, top, base, N, i, lane, any, best);
      else if (left > CP_WAVE) decay_batch<2>(d, top, base, N, i, lane, any, best);
      else decay_batch<1>(d, top, base, N, i, lane, any, best);
    }
    wave_sync();
    have = __ballot(any) == 0ull;                                         // phase B moves rows: the keys are void then
    if (have) continue;
    // phase B
    int pos = i + 1;
    while (pos < N) {
      const int idx = pos + lane;
      const unsigned long long m = __ballot(idx < N && flag[idx] != 0);
      if (m == 0ull) { pos += CP_WAVE; continue; }
      const int p = pos + (__ffsll((long long)m) - 1);                    // the first flagged position, < N
      const int last = N - 1;
      if (p != last) {
        if (lane < 5) {
          float* const c = col + lane * cap;
          c[p] = c[last];
          if (lane == 4) c[last] = old[last];                             // the stale slot keeps the undecayed score
        } else if (lane == 5) {
          flag[p] = flag[last];
        }
      }
      N = last;
      pos = p;                                                            // look at p again
      wave_sync();
    }
  }
  return N;
}

struct NmsArgs {
  float* rows;
  const int* seg_start;
  const int* seg_len;
  int* live;
  int row_stride, cap, method;
  float sigma, Nt, threshold;
};

__global__ __launch_bounds__(CP_WAVE) void soft_nms_segments_kernel(NmsArgs a) {
  extern __shared__ __align__(16) float s_col[];                          // [5][cap], then old [cap], then flag [cap]
  const int lane = threadIdx.x, seg = blockIdx.x;
  const int start = a.seg_start[seg], n = a.seg_len[seg];
  if (n <= 0 || start < 0 || n > a.cap) {                                 // nothing written but the count
    if (lane == 0) a.live[seg] = n > a.cap && start >= 0 ? -1 : 0;
    return;
  }
  float* const old = s_col + 5 * a.cap;
  unsigned char* const flag = reinterpret_cast<unsigned char*>(old + a.cap);
  float* const rows = a.rows + (long long)start * a.row_stride;
  for (int k = lane; k < 5 * n; k += CP_WAVE) {
    const int r = k / 5, c = k - 5 * r;
    s_col[c * a.cap + r] = rows[(long long)r * a.row_stride + c];
  }
  wave_sync();
  const int N = soft_nms_wave(s_col, old, flag, a.cap, n, a.sigma, a.Nt, a.threshold, a.method, lane);
  wave_sync();
  for (int k = lane; k < 5 * n; k += CP_WAVE) {
    const int r = k / 5, c = k - 5 * r;
    rows[(long long)r * a.row_stride + c] = s_col[c * a.cap + r];
  }
  if (lane == 0) a.live[seg] = N;
}

int launch_soft_nms(const NmsArgs& a, int n_seg, hipStream_t st) {
  const size_t lds = nms_lds_bytes(a.cap);
  if (lds > 32 * 1024)
    (void)hipFuncSetAttribute((const void*)soft_nms_segments_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  hipLaunchKernelGGL(soft_nms_segments_kernel, dim3(n_seg), dim3(CP_WAVE), lds, st, a);
  return cp_launch_status();
}

struct MergeArgs {
  const float* rows;          // [M][ncols]
  float* sorted;              // workspace: [M][ncols], the rows class by class
  int* seg_start;             // workspace: [C]
  int* seg_len;               // workspace: [C]
  float* out;                 // [M][ncols]
  int* counts;                // [1 + C]
  int M, ncols, C, max_per_image;
};

__global__ __launch_bounds__(kThreads) void merge_partition_kernel(MergeArgs a) {
  __shared__ signed char s_cls[kMaxRows];
  __shared__ unsigned short s_rank[kMaxRows];                             // position of a row within its class
  __shared__ int s_cnt[kMaxClasses];
  __shared__ int s_start[kMaxClasses];
  const int t = threadIdx.x;
  for (int r = t; r < a.M; r += kThreads)
    s_cls[r] = (signed char)row_merge::class_of(a.rows[(long long)r * a.ncols + 5], a.C);
  row_merge::class_partition(s_cls, s_rank, s_cnt, s_start, a.M, a.C, a.seg_start, a.seg_len);
  const long long total = (long long)a.M * a.ncols;
  for (long long e = t; e < total; e += kThreads) {
    const int r = (int)(e / a.ncols), c = (int)(e - (long long)r * a.ncols);
    const int ci = s_cls[r];
    if (ci >= 0) a.sorted[(long long)(s_start[ci] + s_rank[r]) * a.ncols + c] = a.rows[e];
  }
}

// the slots are the rows of `sorted`, stale ones included: each holds a row, its score is the row's own
__global__ __launch_bounds__(kThreads) void merge_cut_kernel(MergeArgs a) {
  __shared__ row_merge::CutLds<kCutRows> s_cut;
  int total = a.seg_start[a.C - 1] + a.seg_len[a.C - 1];
  total = total < 0 ? 0 : (total > a.M ? a.M : total);
  row_merge::cut_rows(
      s_cut, total, row_merge::EverySlot(), [&](int r) { return a.sorted[(long long)r * a.ncols + 4]; },
      [&](int r) { return a.sorted + (long long)r * a.ncols; }, a.seg_start, a.seg_len, a.C, a.max_per_image, a.ncols,
      a.out, a.counts);
}

size_t sorted_bytes(int S, int K, int ncols) { return cp_align_up((size_t)S * K * ncols * sizeof(float), 16); }

bool merge_shape_ok(int S, int K, int ncols, int C) {
  return S >= 1 && K >= 1 && ncols >= 1 && C >= 1 && (long long)S * K <= kMaxRows && C <= kMaxClasses && ncols >= 7;
}

}  // namespace

extern "C" int cp_soft_nms_device(float* rows, int32_t row_stride, const int32_t* seg_start, const int32_t* seg_len,
                                  int32_t n_seg, float sigma, float Nt, float threshold, int32_t method,
                                  int32_t* live_out, void* stream) {
  CP_CHECK_ARG(n_seg >= 0 && row_stride >= 0);
  CP_CHECK_ARG(method >= 0 && method <= 2);
  CP_CHECK_ARG(rows && seg_start && seg_len && live_out);
  if (row_stride < 5 || n_seg > kMaxSegs) return CP_EUNSUPPORTED;
  if (n_seg == 0) return CP_OK;
  NmsArgs a;
  a.rows = rows; a.seg_start = seg_start; a.seg_len = seg_len; a.live = live_out;
  a.row_stride = row_stride; a.cap = kMaxRows; a.method = method;
  a.sigma = sigma; a.Nt = Nt; a.threshold = threshold;
  return launch_soft_nms(a, n_seg, (hipStream_t)stream);
}

extern "C" size_t cp_merge_detections_workspace_bytes(int32_t S, int32_t K, int32_t ncols, int32_t num_classes) {
  if (!merge_shape_ok(S, K, ncols, num_classes)) return 0;
  return sorted_bytes(S, K, ncols) + cp_align_up((size_t)3 * num_classes * sizeof(int32_t), 16);
}

extern "C" int cp_merge_detections(const float* rows, int32_t S, int32_t K, int32_t ncols, int32_t num_classes,
                                   int32_t max_per_image, int32_t nms, float sigma, float Nt, float threshold,
                                   int32_t method, float* out, int32_t* counts, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(S >= 1 && K >= 1 && ncols >= 1 && num_classes >= 1 && max_per_image >= 1);
  CP_CHECK_ARG(method >= 0 && method <= 2);
  CP_CHECK_ARG(rows && out && counts && workspace && rows != out);
  if (!merge_shape_ok(S, K, ncols, num_classes)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(workspace_bytes >= cp_merge_detections_workspace_bytes(S, K, ncols, num_classes));
  CP_CHECK_ARG((((uintptr_t)workspace) & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  MergeArgs m;
  m.rows = rows; m.out = out; m.counts = counts;
  m.sorted = static_cast<float*>(workspace);
  m.seg_start = reinterpret_cast<int*>(static_cast<char*>(workspace) + sorted_bytes(S, K, ncols));
  m.seg_len = m.seg_start + num_classes;
  m.M = S * K; m.ncols = ncols; m.C = num_classes; m.max_per_image = max_per_image;
  hipLaunchKernelGGL(merge_partition_kernel, dim3(1), dim3(kThreads), 0, st, m);
  int rc = cp_launch_status();
  if (rc != CP_OK) return rc;
  if (nms) {
    NmsArgs a;
    a.rows = m.sorted; a.seg_start = m.seg_start; a.seg_len = m.seg_len; a.live = m.seg_len + num_classes;
    a.row_stride = ncols; a.cap = m.M; a.method = method;
    a.sigma = sigma; a.Nt = Nt; a.threshold = threshold;
    rc = launch_soft_nms(a, num_classes, st);
    if (rc != CP_OK) return rc;
  }
  hipLaunchKernelGGL(merge_cut_kernel, dim3(1), dim3(kThreads), 0, st, m);
  return cp_launch_status();
}
