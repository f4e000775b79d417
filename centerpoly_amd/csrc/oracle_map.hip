// Ground-truth head maps for the --eval_oracle_* switches on gfx950 (reference: utils/oracle_utils.py gen_oracle_map,
// a breadth-first flood fill on the host).
//
// On an unobstructed rectangle the fill has a closed form: a pixel's BFS level is its L1 distance to the nearest seed
// and the queue keeps every level in seed order, so
//   out[b][:][y][x] = feat[b][j*][:],  j* = the LOWEST j among the valid seeds at minimal |x - x_j| + |y - y_j|,
// except at a seed's own pixel, where the HIGHEST j with that ind wins (later duplicates overwrite the pixel, the
// earlier one expands first).  A seed is valid when 0 < ind < h * w; an image without one is all zeros.
//
// One launch over (pixel tiles x B).  A workgroup owns kTileW x kTileH pixels, a thread four pixels along x:
//   1  wave 0 compacts the image's valid seeds into LDS as (x, y), j in j order (ballot + popcount, 64 slots a step);
//   2  when M rows of feat fit (kFeatLds), the valid rows are staged in LDS by table position, odd row stride;
//   3  every thread scans the table once for its four pixels, keeping (best distance, table position) with a strict
//      `<` (lowest j on ties) and taking every distance-0 hit (last duplicate wins);
//   4  the channel loop writes out[b][c][y][x .. x + 3]: one 16-byte store where w % 4 == 0 and out is 16-byte
//      aligned, scalar stores cut at w otherwise.  Every element of out is written, zeros of an empty image included.
// HBM-write bound: B * D * h * w * 4 bytes out, M * (8 + 4 D) bytes in per workgroup (L2 hits after the first).
#include "cp_common.h"

namespace {

constexpr int kMaxSeeds = 1024;                                           // M beyond: CP_EUNSUPPORTED
constexpr int kTileW = 64, kTileH = 8;                                    // pixels of a workgroup
constexpr int kThreads = (kTileW / 4) * kTileH;                           // 128: four pixels along x per thread
constexpr int kFeatLds = 32 * 1024;                                       // bytes of staged feat rows

struct OracleArgs {
  const float* feat;            // [B][M][D]
  const long long* ind;         // [B][M]
  float* out;                   // [B][D][h][w]
  int B, M, D, h, w;
  int tiles_x;
  int stage;                    // feat rows staged in LDS (row stride D | 1)
  int wide;                     // 16-byte stores
};

__global__ __launch_bounds__(kThreads) void oracle_map_kernel(OracleArgs a) {
  __shared__ int2 s_xy[kMaxSeeds];
  __shared__ int s_j[kMaxSeeds];
  __shared__ int s_n;
  extern __shared__ __align__(16) float s_feat[];
  const int tid = threadIdx.x, b = blockIdx.y;
  const long long hw = (long long)a.h * a.w;

  // ---- 1: the valid seeds of image b, in j order ----
  if (tid < 64) {
    const long long* ind = a.ind + (long long)b * a.M;
    const unsigned long long below = (1ull << tid) - 1ull;
    int n = 0;                                                            // (uniform in the wave)
    for (int base = 0; base < a.M; base += 64) {
      const int j = base + tid;
      const long long v = j < a.M ? ind[j] : 0;
      const bool ok = v > 0 && v < hw;
      const unsigned long long m = __ballot(ok);
      if (ok) {
        const int k = n + __popcll(m & below);                            // < M <= kMaxSeeds
        s_xy[k] = make_int2((int)(v % a.w), (int)(v / a.w));
        s_j[k] = j;
      }
      n += __popcll(m);
    }
    if (tid == 0) s_n = n;
  }
  __syncthreads();
  const int n = s_n;

  // ---- 2: the valid rows of feat, by table position ----
  const int ld = a.D | 1;
  if (a.stage) {
    const float* feat = a.feat + (long long)b * a.M * a.D;
    for (int i = tid; i < n * a.D; i += kThreads) {                       // n * D <= M * D < kFeatLds / 4
      const int k = i / a.D, c = i - k * a.D;
      s_feat[k * ld + c] = feat[(long long)s_j[k] * a.D + c];
    }
    __syncthreads();
  }

  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y = ty * kTileH + tid / (kTileW / 4), x0 = tx * kTileW + 4 * (tid % (kTileW / 4));
  if (y >= a.h || x0 >= a.w) return;

  // ---- 3: the owner of each of the four pixels ----
  int best[4], own[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { best[q] = INT32_MAX; own[q] = -1; }
  for (int k = 0; k < n; ++k) {
    const int2 s = s_xy[k];
    const int dy = abs(y - s.y), dx = x0 - s.x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d = dy + abs(dx + q);                                     // <= h + w - 2 + 3
      if (d < best[q] || d == 0) { best[q] = d; own[q] = k; }
    }
  }

  // ---- 4: the channels ----
  const int cnt = min(4, a.w - x0);
  float* o = a.out + (long long)b * a.D * hw + (long long)y * a.w + x0;
  const float* row[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (a.stage) row[q] = s_feat + max(own[q], 0) * ld;
    else row[q] = a.feat + ((long long)b * a.M + (own[q] >= 0 ? s_j[own[q]] : 0)) * a.D;
  }
  const bool any = n > 0;
#pragma unroll 4
  for (int c = 0; c < a.D; ++c) {
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = any ? row[q][c] : 0.f;
    float* oc = o + (long long)c * hw;
    if (a.wide) {
      *reinterpret_cast<f32x4*>(oc) = v;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < cnt) oc[q] = v[q];
    }
  }
}

}  // namespace

extern "C" int cp_oracle_map(const float* feat, const int64_t* ind, int32_t B, int32_t M, int32_t D, int32_t h,
                             int32_t w, float* out, void* stream) {
  CP_CHECK_ARG(feat && ind && out);
  CP_CHECK_ARG(B > 0 && M > 0 && D > 0 && h > 0 && w > 0);
  const long long hw = (long long)h * w;
  // (32-bit pixel coordinates and distances: h + w + kTileW stays far inside int32)
  if (M > kMaxSeeds || B > 65535 || hw >= (1ll << 31) || h > (1 << 30) || w > (1 << 30)) return CP_EUNSUPPORTED;
  const long long tiles_x = (w + kTileW - 1) / kTileW, tiles_y = (h + kTileH - 1) / kTileH;
  OracleArgs a;
  a.feat = feat; a.ind = (const long long*)ind; a.out = out;
  a.B = B; a.M = M; a.D = D; a.h = h; a.w = w;
  a.tiles_x = (int)tiles_x;
  const long long ld = D | 1;
  a.stage = (long long)M * ld * 4 <= kFeatLds;
  a.wide = w % 4 == 0 && ((uintptr_t)out & 15) == 0;
  const size_t lds = a.stage ? (size_t)(M * ld * 4) : 0;
  hipLaunchKernelGGL(oracle_map_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)B), dim3(kThreads), lds,
                     (hipStream_t)stream, a);
  return cp_launch_status();
}
