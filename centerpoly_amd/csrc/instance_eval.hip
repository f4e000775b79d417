// Pixel counting of the Cityscapes instance-level evaluation for gfx950.
//
// The evaluator compares every predicted mask of an image with every ground-truth instance: per pair one
// full-image pass `count_nonzero(gt == instID & pred != 0)`, plus `np.unique` and one `(img == id).sum()` per
// id for the ground-truth table.  All of it is integer counting over data the device already holds
// (cp_instance_masks' output and the 16-bit id image), done here in one streaming pass each:
//   cp_id_histogram       pixels per 16-bit value.  Runs of equal ids are collapsed in registers (a 16-pixel
//                         piece per lane, a whole wave when its 1024 pixels agree), counted in a small
//                         per-workgroup LDS cache keyed by id, and flushed with global atomics.
//   cp_instance_overlaps  a 65536-entry table (workspace), built by a one-workgroup kernel that also zeroes the
//                         outputs, maps an id to its column of `inst_ids` and to "void".  In the counting kernel a
//                         workgroup owns a span of pixels and a slice of masks, keeps slice x (G + 2) counters in
//                         LDS (G columns, void, mask pixels) and flushes the non-zero ones with global atomics.
//                         A lane reads its 16 ids once, maps them once and then streams 16 mask bytes per mask.
//                         Two launches, whatever n and G.
// Integer atomics only: the result does not depend on the order of the additions.
// The piece, span and run scheme and the loaders are pixel_pieces.h's.
#include "pixel_pieces.h"

namespace {

constexpr int kVoidBit = 0x8000;                        // table entry: (column + 1) | kVoidBit
constexpr int kLdsCounters = 8192;                      // 32 KiB of counters: four workgroups and more per CU
constexpr int kBatch = 4;                              // masks a lane loads before it counts them
constexpr int kCacheSlots = 1024;                       // histogram: LDS cache entries per workgroup
constexpr int kMaxMasks = 128, kMaxInst = 1024, kMaxVoid = 64;

// ------------------------------------------------------------------ histogram --
__device__ __forceinline__ void hist_add(int* keys, int* vals, int* hist, int id, int cnt) {
  const int slot = (id * 40503u >> 4) & (kCacheSlots - 1);
  const int old = atomicCAS(&keys[slot], -1, id);
  if (old == -1 || old == id) atomicAdd(&vals[slot], cnt);
  else atomicAdd(&hist[id], cnt);
}

__global__ __launch_bounds__(kThreads) void id_histogram_kernel(const uint16_t* __restrict__ ids, long long HW,
                                                                long long span, int* __restrict__ hist) {
  __shared__ int keys[kCacheSlots], vals[kCacheSlots];
  for (int k = threadIdx.x; k < kCacheSlots; k += kThreads) { keys[k] = -1; vals[k] = 0; }
  __syncthreads();
  const long long begin = (long long)blockIdx.x * span, end = min(begin + span, HW);
  const bool fast = aligned16(ids);
  for (long long t0 = begin; t0 < end; t0 += kTile) {
    const long long p0 = t0 + (long long)threadIdx.x * kPiece;
    const int valid = (int)max(0LL, min((long long)kPiece, end - p0));
    int v[kPiece];
    load_ids(ids, p0, valid, fast, v);
    bool same = valid == kPiece;
#pragma unroll
    for (int k = 1; k < kPiece; ++k) same = same && v[k] == v[0];
    const int first = __shfl(v[0], 0, CP_WAVE);
    if (__all(same && v[0] == first)) {                                   // 1024 pixels of one id
      if ((threadIdx.x & (CP_WAVE - 1)) == 0) hist_add(keys, vals, hist, first, CP_WAVE * kPiece);
    } else if (valid > 0) {
      int id = v[0], cnt = 1;
#pragma unroll
      for (int k = 1; k < kPiece; ++k) {
        if (k < valid) {
          if (v[k] != id) { hist_add(keys, vals, hist, id, cnt); id = v[k]; cnt = 0; }
          ++cnt;
        }
      }
      hist_add(keys, vals, hist, id, cnt);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kCacheSlots; k += kThreads)
    if (vals[k]) atomicAdd(&hist[keys[k]], vals[k]);
}

// ------------------------------------------------------------------- overlaps --
// One workgroup prepares a call: zeroes the table and the three outputs, then enters the ids (one launch instead of
// four fills and a kernel; 128 K table and at most 128 x 1024 output words are a few microseconds for 1024 lanes).
__global__ __launch_bounds__(1024) void overlap_prepare_kernel(const int* __restrict__ inst_ids, int G,
                                                               const int* __restrict__ void_ids, int V,
                                                               uint16_t* __restrict__ table, int* __restrict__ inter,
                                                               int* __restrict__ void_inter,
                                                               int* __restrict__ pred_pixels, int n) {
  const int t = threadIdx.x;
  unsigned* words = reinterpret_cast<unsigned*>(table);                   // hipMalloc'ed workspace: 4-byte aligned
  for (int k = t; k < kIds / 2; k += 1024) words[k] = 0;
  for (int k = t; k < n * G; k += 1024) inter[k] = 0;
  if (t < n) { void_inter[t] = 0; pred_pixels[t] = 0; }
  __syncthreads();
  if (t < G && inst_ids[t] >= 0 && inst_ids[t] < kIds) table[inst_ids[t]] = (uint16_t)(t + 1);
  __syncthreads();
  // (equal void ids write equal values; an id outside 16 bits, the label table's -1, matches no pixel)
  if (t < V && void_ids[t] >= 0 && void_ids[t] < kIds) table[void_ids[t]] |= kVoidBit;
}

struct OverlapArgs {
  const uint8_t* masks;       // [n][HW]
  const uint16_t* ids;        // [HW]
  const uint16_t* table;      // [65536]
  int* inter;                 // [n][G]
  int* void_inter;            // [n]
  int* pred_pixels;           // [n]
  long long HW, span;         // pixels, pixels per workgroup (a multiple of kTile)
  int n, G, slice;            // masks per workgroup
};

// one piece of one mask into the mask's counter row c[G + 2]
__device__ __forceinline__ void count_piece(u32x4 w, int* c, int G, const int (&code)[kPiece], unsigned edges,
                                            bool wave_same) {
  const unsigned nz[4] = {nonzero_bytes(w.x), nonzero_bytes(w.y), nonzero_bytes(w.z), nonzero_bytes(w.w)};
  int total = __popc(nz[0]) + __popc(nz[1]) + __popc(nz[2]) + __popc(nz[3]);
  const int col0 = (code[0] & (kVoidBit - 1)) - 1;
  if (wave_same) {                                                        // every lane is here, with the same code
    if (!__any(total != 0)) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, CP_WAVE);
    if ((threadIdx.x & (CP_WAVE - 1)) == 0) {
      atomicAdd(&c[G + 1], total);
      if (col0 >= 0) atomicAdd(&c[col0], total);
      if (code[0] & kVoidBit) atomicAdd(&c[G], total);
    }
    return;
  }
  if (total == 0) return;
  atomicAdd(&c[G + 1], total);
  if (edges == 0) {                                                       // one id under the whole piece
    if (col0 >= 0) atomicAdd(&c[col0], total);
    if (code[0] & kVoidBit) atomicAdd(&c[G], total);
    return;
  }
  int run = 0, nvoid = 0;
#pragma unroll
  for (int k = 0; k < kPiece; ++k) {
    if (k && (edges >> k & 1)) {
      if (run && (code[k - 1] & (kVoidBit - 1))) atomicAdd(&c[(code[k - 1] & (kVoidBit - 1)) - 1], run);
      if (code[k - 1] & kVoidBit) nvoid += run;
      run = 0;
    }
    run += nz[k >> 2] >> (8 * (k & 3) + 7) & 1;
  }
  if (run && (code[kPiece - 1] & (kVoidBit - 1))) atomicAdd(&c[(code[kPiece - 1] & (kVoidBit - 1)) - 1], run);
  if (code[kPiece - 1] & kVoidBit) nvoid += run;
  if (nvoid) atomicAdd(&c[G], nvoid);
}

__global__ __launch_bounds__(kThreads) void instance_overlaps_kernel(OverlapArgs a) {
  extern __shared__ int cnt[];                                            // [slice][G + 2]: columns, void, pixels
  const int cols = a.G + 2;
  const int m0 = blockIdx.y * a.slice, ms = min(a.slice, a.n - m0);
  for (int k = threadIdx.x; k < ms * cols; k += kThreads) cnt[k] = 0;
  __syncthreads();
  const long long begin = (long long)blockIdx.x * a.span, end = min(begin + a.span, a.HW);
  const bool fast_ids = aligned16(a.ids);
  for (long long t0 = begin; t0 < end; t0 += kTile) {
    const long long p0 = t0 + (long long)threadIdx.x * kPiece;
    // (a lane past the span's end keeps valid == 0 and walks along: the wave votes below need every lane)
    const int valid = (int)max(0LL, min((long long)kPiece, end - p0));
    // the piece's ids -> table codes, once for all masks of the slice; `edges` bit k: pixel k starts a run (the
    // padding repeats the id before it: no edge past `valid`)
    int code[kPiece];
    load_ids(a.ids, p0, valid, fast_ids, code);
    unsigned edges = 0;
    {
      int prev_id = code[0], prev_code = a.table[prev_id];
      code[0] = prev_code;
#pragma unroll
      for (int k = 1; k < kPiece; ++k) {
        if (code[k] != prev_id) { prev_id = code[k]; prev_code = a.table[prev_id]; }
        if (prev_code != code[k - 1]) edges |= 1u << k;
        code[k] = prev_code;
      }
    }
    // most waves lie inside one region: then the wave adds its 1024 pixels up and one lane touches the counters
    const bool wave_same = __all(edges == 0 && valid == kPiece && code[0] == __shfl(code[0], 0, CP_WAVE));
    const uint8_t* mp = a.masks + (long long)m0 * a.HW + p0;
    for (int m = 0; m < ms; m += kBatch, mp += kBatch * a.HW) {           // kBatch loads in flight per lane
      u32x4 w[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {                                  // (a mask starts wherever n * HW falls)
        const uint8_t* mj = mp + j * a.HW;
        w[j] = m + j < ms ? load_bytes<true>(mj, valid, aligned16(mj)) : u32x4{0, 0, 0, 0};
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j)
        if (m + j < ms) count_piece(w[j], cnt + (m + j) * cols, a.G, code, edges, wave_same);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < ms * cols; k += kThreads) {
    const int v = cnt[k];
    if (!v) continue;
    const int m = k / cols, j = k - m * cols;
    int* dst = j < a.G ? a.inter + (long long)(m0 + m) * a.G + j : j == a.G ? a.void_inter + m0 + m : a.pred_pixels + m0 + m;
    atomicAdd(dst, v);
  }
}

}  // namespace

extern "C" int cp_id_histogram(const uint16_t* ids, int32_t H, int32_t W, int32_t* hist, void* stream) {
  CP_CHECK_ARG(ids && hist && H > 0 && W > 0);
  const long long HW = (long long)H * W;
  if (HW >= (1LL << 31)) return CP_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(hist, 0, (size_t)kIds * sizeof(int), st);
  // one workgroup per CU: every workgroup ends with an atomic on the few ids that fill the image (road, sky), and
  // those serialise on one address
  const long long span = span_for(HW, 256);
  hipLaunchKernelGGL(id_histogram_kernel, dim3(span_blocks(HW, span)), dim3(kThreads), 0, st, ids, HW, span, hist);
  return cp_launch_status();
}

extern "C" size_t cp_instance_overlaps_workspace_bytes(int32_t n, int32_t G, int32_t H, int32_t W) {
  (void)n; (void)G; (void)H; (void)W;
  return (size_t)kIds * sizeof(uint16_t);                                 // the id -> column table
}

extern "C" int cp_instance_overlaps(const uint8_t* masks, int32_t n, const uint16_t* gt_ids, int32_t H, int32_t W,
                                    const int32_t* inst_ids, int32_t G, const int32_t* void_ids, int32_t V,
                                    int32_t* inter, int32_t* void_inter, int32_t* pred_pixels, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(n >= 0 && G >= 0 && V >= 0 && H > 0 && W > 0);
  const long long HW = (long long)H * W;
  if (n > kMaxMasks || G > kMaxInst || V > kMaxVoid || HW >= (1LL << 31)) return CP_EUNSUPPORTED;
  if (n == 0) return CP_OK;
  CP_CHECK_ARG(masks && gt_ids && void_inter && pred_pixels && (G == 0 || (inst_ids && inter)) && (V == 0 || void_ids));
  if (!workspace || workspace_bytes < cp_instance_overlaps_workspace_bytes(n, G, H, W)) return CP_EWORKSPACE;
  CP_CHECK_ARG(((uintptr_t)workspace & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  uint16_t* table = (uint16_t*)workspace;
  hipLaunchKernelGGL(overlap_prepare_kernel, dim3(1), dim3(1024), 0, st, inst_ids, G, void_ids, V, table, inter,
                     void_inter, pred_pixels, n);
  OverlapArgs a;
  a.masks = masks; a.ids = gt_ids; a.table = table; a.inter = inter; a.void_inter = void_inter;
  a.pred_pixels = pred_pixels; a.HW = HW; a.n = n; a.G = G;
  a.slice = min(n, kLdsCounters / (G + 2));
  const int slices = (n + a.slice - 1) / a.slice;
  a.span = span_for(HW, (1024 + slices - 1) / slices);
  hipLaunchKernelGGL(instance_overlaps_kernel, dim3(span_blocks(HW, a.span), slices), dim3(kThreads),
                     (size_t)a.slice * (G + 2) * sizeof(int), st, a);
  return cp_launch_status();
}
