// Instance masks of the KITTI and IDD result writers for gfx950: PIL's polygon, restated exactly, with per-class
// occlusion.
//
// KITTI.format_and_write_to_kitti and IDD.format_and_write_to_IDD (reference: src/lib/datasets/dataset/
// kitti_poly.py:95-136, IDD.py:123-170) draw every detection, class by class and in ascending depth within a class, as
//   ImageDraw.polygon(points, outline=0, fill=255)  times the class's to_remove_mask,
//   ImageDraw.Draw(to_remove_mask).polygon(points, outline=0, fill=0)   when score >= 0.5
// on a canvas of the image's own size.  With F what PIL's fill sets and O what PIL's outline sets:
//   mask_i = (F_i \ O_i) \ union { F_j : j < i, group_j == group_i, flags_j bit 1 }
// (PIL draws no outline whose ink equals the fill's, so the second call clears F alone: an instance loses its own
// outline but hides farther ones with its fill only).
// There is no contour band here that would hide the difference between PIL's scan-line fill and an even-odd test at
// pixel centres (see result_writer.hip), so F and O are PIL's own rules (class_masks_core.h; scanline.h holds the scan
// line around them, here in its wave form, and the clipped line).  Three kernels and one
// small memset whatever n is; every mask byte is written once by the fill kernel and swept once by the last one:
//   fill kernel     one wave per (instance, row): lane k owns edge k and computes what it adds to the row's crossing
//                   list in float32 (the vertex rule walks the earlier edges in LDS); a bitonic sort of the at most
//                   128 values through wave shuffles; the pairs and the flat edges become a compacted span list, and
//                   the lanes write the whole row, 16 pixels = 16 bytes per lane and step, 1 inside / 0 outside;
//   outline kernel  one thread per edge walks the part of PIL's integer line that lies on the canvas and sets bit 1;
//   occlusion kernel  one thread per 8 pixels walks the drawn instances group by group in input order: 1 becomes 255
//                   unless an earlier occluding instance of the group filled the pixel (bit 0), 2 and 3 become 0;
//                   the counts.
#include "cp_common.h"
#include "scanline.h"

namespace {

constexpr int kMaxInst = 128;
constexpr int kMaxVerts = 64;
constexpr int kRowsPerBlock = 4;                                          // waves of the fill kernel's workgroup

struct ClassMaskArgs {
  const int* poly;            // [n][N][2] (x, y), drawing order
  const int* group;           // [n]
  const unsigned char* flags; // [n]: bit 0 = draw, bit 1 = occludes (score >= 0.5)
  unsigned char* masks;       // [n][H][W]
  int* counts;                // [n]
  int n, N, H, W;
};

struct Bytes16 { unsigned w[4]; };

__global__ __launch_bounds__(64 * kRowsPerBlock) void class_fill_kernel(ClassMaskArgs a) {
  __shared__ CmEdge s_edge[kMaxVerts];
  __shared__ float s_x[kRowsPerBlock][2 * kMaxVerts];
  __shared__ SlSpan s_span[kRowsPerBlock][2 * kMaxVerts];
  const int i = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int y = blockIdx.x * kRowsPerBlock + w;
  const int* p = a.poly + (long long)i * a.N * 2;
  const bool drawn = (a.flags[i] & 1) != 0;                               // uniform in the workgroup
  if (threadIdx.x < kMaxVerts) {
    CmEdge e;
    e.kind = CM_ABSENT;
    if (drawn && threadIdx.x < a.N) e = cm_make_edge(p, threadIdx.x, a.N);
    s_edge[threadIdx.x] = e;
  }
  // the polygon's last scan line: max(0, largest y) cut at H
  int hi = (drawn && lane < a.N) ? p[2 * lane + 1] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hi = max(hi, __shfl_xor(hi, o, 64));
  const int last_row = min(hi, a.H);
  __syncthreads();

  const int nsp = sl_wave_spans(s_edge, s_x[w], s_span[w], lane, y, last_row, a.W);
  if (y >= a.H) return;
  unsigned char* row = a.masks + ((long long)i * a.H + y) * a.W;
  for (int x0 = lane * 16; x0 < a.W; x0 += 64 * 16) {
    unsigned bits = 0;
    for (int s = 0; s < nsp; ++s) {
      const SlSpan q = s_span[w][s];
      const int lo = max(q.lo, x0) - x0, hi2 = min(q.hi, x0 + 15) - x0;
      if (lo <= hi2) bits |= ((2u << hi2) - 1u) & ~((1u << lo) - 1u);
    }
    Bytes16 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v.w[k] = (((bits >> (4 * k)) & 15u) * 0x00204081u) & 0x01010101u;   // bit -> byte
    if (x0 + 16 <= a.W) {
      __builtin_memcpy(row + x0, &v, 16);                                 // any alignment: H * W need not be even
    } else {
      for (int k = 0; x0 + k < a.W; ++k) row[x0 + k] = (unsigned char)((bits >> k) & 1u);
    }
  }
}

__global__ __launch_bounds__(64) void class_outline_kernel(ClassMaskArgs a) {
  const int t = blockIdx.x * 64 + threadIdx.x;                            // edge (instance, vertex)
  if (t >= a.n * a.N) return;
  const int i = t / a.N, k = t - i * a.N;
  if (!(a.flags[i] & 1)) return;
  const int* p = a.poly + (long long)i * a.N * 2;
  const int j = k + 1 == a.N ? 0 : k + 1;
  const int x0 = p[2 * k], y0 = p[2 * k + 1], x1 = p[2 * j], y1 = p[2 * j + 1];
  unsigned char* mk = a.masks + (long long)i * a.H * a.W;
  // (edges that meet store the same byte: fill bit | 2)
  sl_line_clipped(x0, y0, x1, y1, a.W, a.H, [&](long long at) { mk[at] |= 2; });
}

// four pixels per word, every byte bit 0 = filled, bit 1 = on the outline
__device__ __forceinline__ unsigned occlude_word(unsigned v, unsigned& removed, bool occludes, int& count) {
  const unsigned filled = v & 0x01010101u, outline = (v >> 1) & 0x01010101u;
  const unsigned keep = filled & ~outline & ~removed;
  if (occludes) removed |= filled;
  count += __popc(keep);
  return keep * 255u;
}

__global__ __launch_bounds__(256) void class_occlude_kernel(ClassMaskArgs a) {
  __shared__ int s_grp[kMaxInst], s_first[kMaxInst], s_ord[kMaxInst], s_cnt[kMaxInst];
  __shared__ unsigned char s_fl[kMaxInst];
  __shared__ int s_m;
  const int t = threadIdx.x;
  if (t < kMaxInst) {
    s_grp[t] = t < a.n ? a.group[t] : 0;
    s_fl[t] = t < a.n ? a.flags[t] : 0;
    s_cnt[t] = 0;
  }
  if (t == 0) s_m = 0;
  __syncthreads();
  // the drawn instances group by group (groups by first appearance, input order inside a group)
  const bool mine = t < a.n && (s_fl[t] & 1);
  if (mine) {
    int first = t;
    for (int j = 0; j < t; ++j)
      if ((s_fl[j] & 1) && s_grp[j] == s_grp[t]) { first = j; break; }
    s_first[t] = first;
  }
  __syncthreads();
  if (mine) {
    const int first = s_first[t];
    int rank = 0;
    for (int j = 0; j < a.n; ++j)
      if ((s_fl[j] & 1) && (s_first[j] < first || (s_first[j] == first && j < t))) ++rank;
    s_ord[rank] = t | (first == t ? 0x100 : 0) | ((s_fl[t] & 2) ? 0x200 : 0);
    atomicAdd(&s_m, 1);
  }
  __syncthreads();
  const int m = s_m;
  const long long HW = (long long)a.H * a.W;
  const long long p0 = ((long long)blockIdx.x * 256 + t) * 8;
  if (p0 < HW) {
    const bool whole = p0 + 8 <= HW;
    const int tail = whole ? 8 : (int)(HW - p0);
    unsigned rem0 = 0, rem1 = 0;
#pragma unroll 4
    for (int q = 0; q < m; ++q) {
      const int o = s_ord[q], i = o & 0xff;
      if (o & 0x100) { rem0 = 0; rem1 = 0; }
      unsigned char* mk = a.masks + (long long)i * HW + p0;
      unsigned v[2] = {0u, 0u};
      if (whole) {
        __builtin_memcpy(v, mk, 8);
      } else {
        for (int k = 0; k < tail; ++k) v[k >> 2] |= (unsigned)mk[k] << (8 * (k & 3));
      }
      if ((v[0] | v[1]) == 0u) continue;                                  // most pixels of most instances
      int c = 0;
      v[0] = occlude_word(v[0], rem0, (o & 0x200) != 0, c);
      v[1] = occlude_word(v[1], rem1, (o & 0x200) != 0, c);
      if (whole) {
        __builtin_memcpy(mk, v, 8);
      } else {
        for (int k = 0; k < tail; ++k) mk[k] = (unsigned char)(v[k >> 2] >> (8 * (k & 3)));
      }
      if (c) atomicAdd(&s_cnt[i], c);
    }
  }
  __syncthreads();
  if (t < a.n && s_cnt[t]) atomicAdd(&a.counts[t], s_cnt[t]);
}

}  // namespace

extern "C" int cp_class_instance_masks(const int32_t* poly, const int32_t* group, const uint8_t* flags, int32_t n,
                                       int32_t N, int32_t H, int32_t W, uint8_t* masks, int32_t* counts,
                                       void* stream) {
  CP_CHECK_ARG(n >= 0 && N >= 3 && H > 0 && W > 0);
  if (n == 0) return CP_OK;
  CP_CHECK_ARG(poly && group && flags && masks && counts);
  if (n > kMaxInst || N > kMaxVerts || (long long)H * W >= (1ll << 31)) return CP_EUNSUPPORTED;
  ClassMaskArgs a;
  a.poly = poly; a.group = group; a.flags = flags; a.masks = masks; a.counts = counts;
  a.n = n; a.N = N; a.H = H; a.W = W;
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(counts, 0, (size_t)n * sizeof(int), st);
  hipLaunchKernelGGL(class_fill_kernel, dim3((H + kRowsPerBlock - 1) / kRowsPerBlock, n), dim3(64 * kRowsPerBlock), 0,
                     st, a);
  hipLaunchKernelGGL(class_outline_kernel, dim3((n * N + 63) / 64), dim3(64), 0, st, a);
  const long long HW = (long long)H * W;
  hipLaunchKernelGGL(class_occlude_kernel, dim3((unsigned)((HW + 2047) / 2048)), dim3(256), 0, st, a);
  return cp_launch_status();
}
