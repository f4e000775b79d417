// Boundary bands and their pair counts for gfx950: the pixel work of Boundary IoU / Boundary AP.
//
// band(M, d) = M minus the erosion of M by the (2d + 1)^2 square, pixels outside the image counting as not in M.  The
// erosion is separable and runs on BIT images, 32 pixels of a row per word, kept in the workspace:
//   rows     one thread per word of a line (a row of a plane, or of the id image).  The thread packs its 32 pixels,
//            the workgroup shares the packed line through LDS, and the thread ANDs the 2d + 1 shifts of the 160 bits
//            around its word by doubling (A_2k(x) = A_k(x) & A_k(x + k)): eight steps at d = 64.  For the id image the
//            packed bit is "same value as the pixel to the left" and the window is the 2d pixels right of x - d, so
//            the result is "the 2d + 1 window lies inside the row and is constant"; two more bit images hold "same
//            value as the pixel above" and the left-neighbour bits themselves.
//   columns  one thread per word column and strip of rows (32, 64 from d = 17 on; 8 for the id image) walks down the
//            strip's rows and d rows either side, keeping for each of its 32 columns the length of the run of passing
//            rows in a bit-sliced counter (eight words and a sticky "run >= 2d + 1" word, a ripple carry per row).
//            Row y is decided when row y + d has been added.  For the id image a row whose pixel differs from the one
//            above restarts the run at one.
// A thread of the columns pass loads eight rows of its bit images before it works on them: the loads do not depend on
// its state.  The band word is the mask word without the eroded word.  Band pixels are few, so the pair counts go run
// by run of equal ids within a word (the left-neighbour bits mark them): the id through the id -> column
// table into counters in LDS, flushed once per workgroup with global atomics.
// The id image's band is made first (its own bit image); the planes' pass reads it.
// With bounds a mask is zero outside its clipped bounds, so only words and rows inside them are read, written and
// walked.
// Five launches (three when n == 0; a fill more when band images and bounds are both asked for), whatever n, G and d
// are.  Integer atomics only: the same bits on every run.
#include "pixel_pieces.h"

namespace {

constexpr int kMaxMasks = 128, kMaxInst = 1024, kMaxD = 64;
constexpr int kLineWords = 64;                           // words of a line per workgroup: 2048 pixels
constexpr int kLines = kThreads / kLineWords;            // lines (rows pass) or planes (columns pass) per workgroup
constexpr int kHalo = 2;                                 // words either side of a word that 64 pixels reach into
// Rows a thread of the planes' columns pass decides.  The thread walks them and d rows either side one after the
// other, a chain of strip + 2d dependent steps that sets the pass's time; every strip walks its 2d rows again, which
// sets its work.  Short strips while 2d is small beside them, long ones for wide bands.
constexpr int kStrip = 32, kStripWide = 64, kWideFrom = 17;
// The id image is one plane: short strips and one wave per workgroup spread it over the device.  The d rows walked
// either side of a strip are bit words; the counting, the costly part, is done for the strip's own rows only.
constexpr int kGtStrip = 8, kGtThreads = 64;
constexpr unsigned kMaxBlocks = 1u << 13;                 // of the rows pass: it strides over the groups of lines

struct Bits192 { unsigned long long a0, a1, a2; };       // bit b of a0 is pixel x_base + b

__device__ __forceinline__ Bits192 shr(Bits192 v, int k) {          // k in [0, 128), uniform over the launch
  if (k >= 64) { v.a0 = v.a1; v.a1 = v.a2; v.a2 = 0; k -= 64; }
  if (k) {
    v.a0 = v.a0 >> k | v.a1 << (64 - k);
    v.a1 = v.a1 >> k | v.a2 << (64 - k);
    v.a2 >>= k;
  }
  return v;
}

// AND of the `len` bits from x + first on, for the 32 pixels x of the middle word of five (line[-2 .. 2]):
// 2 <= len <= 129, -64 <= first, first + len <= 65.
__device__ __forceinline__ unsigned window_and(const unsigned* line, int first, int len) {
  Bits192 v = {line[-2] | (unsigned long long)line[-1] << 32, line[0] | (unsigned long long)line[1] << 32, line[2]};
  int k = 1;
  for (; 2 * k <= len; k *= 2) {
    const Bits192 s = shr(v, k);
    v.a0 &= s.a0; v.a1 &= s.a1; v.a2 &= s.a2;
  }
  if (len > k) {
    const Bits192 s = shr(v, len - k);
    v.a0 &= s.a0; v.a1 &= s.a1; v.a2 &= s.a2;
  }
  return (unsigned)shr(v, 64 + first).a0;
}

// bit k: byte k of the 32 at p is non-zero, for the first `valid` of them
__device__ __forceinline__ unsigned pack_nonzero(const uint8_t* p, int valid) {
  unsigned out = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int v = min(kPiece, valid - h * kPiece);
    if (v <= 0) break;
    const u32x4 w = load_bytes<true>(p + h * kPiece, v, aligned16(p));
    const unsigned nz[4] = {nonzero_bytes(w.x), nonzero_bytes(w.y), nonzero_bytes(w.z), nonzero_bytes(w.w)};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned b = nz[j] >> 7;                                      // bits 0, 8, 16, 24
      out |= ((b | b >> 7 | b >> 14 | b >> 21) & 15u) << (h * kPiece + 4 * j);
    }
  }
  return out;
}

// the bits of [lo, hi] (inclusive pixel columns, any integers) that fall into word wc
__device__ __forceinline__ unsigned range_bits(int wc, int lo, int hi) {
  const int a = max(lo - wc * 32, 0), b = min(hi - wc * 32, 31);
  if (a > b) return 0;
  return (0xffffffffu >> (31 - b)) & (0xffffffffu << a);
}

struct Clip { int x0, y0, x1, y1; };                      // inclusive, clipped to the image; x1 < x0 or y1 < y0: empty

__device__ __forceinline__ Clip clip_of(const int* bounds, int i, int H, int W) {
  if (!bounds) return Clip{0, 0, W - 1, H - 1};
  const int* b = bounds + 4 * i;
  return Clip{max(b[0], 0), max(b[1], 0), min(b[2], W - 1), min(b[3], H - 1)};
}

__global__ __launch_bounds__(1024) void boundary_prepare_kernel(const int* __restrict__ inst_ids, int G,
                                                                uint16_t* __restrict__ table, int* __restrict__ b_inter,
                                                                int* __restrict__ b_pred, int* __restrict__ b_gt,
                                                                int n) {
  const int t = threadIdx.x;
  unsigned* words = reinterpret_cast<unsigned*>(table);
  for (int k = t; k < kIds / 2; k += 1024) words[k] = 0;
  for (int k = t; k < n * G; k += 1024) b_inter[k] = 0;
  if (t < n) b_pred[t] = 0;
  if (t < G) b_gt[t] = 0;
  __syncthreads();
  if (t < G && inst_ids[t] >= 0 && inst_ids[t] < kIds) table[inst_ids[t]] = (uint16_t)(t + 1);
}

struct RowArgs {
  const uint8_t* masks;       // [n][H][W]
  const uint16_t* ids;        // [H][W]
  const int* bounds;          // [n][4] or null
  unsigned* mask_bits;        // [n][H][WB]  pixel is in the mask (and its bounds)
  unsigned* row_ok;           // [n][H][WB]  and so are the d pixels either side
  unsigned* gt_row_ok;        // [H][WB]     the 2d + 1 window of the row is inside the image and constant
  unsigned* gt_vsame;         // [H][WB]     same value as the pixel above
  unsigned* gt_hsame;         // [H][WB]     same value as the pixel to the left
  long long lines;            // n * H, or H for the id image
  int H, W, WB, d;
  unsigned tiles;             // workgroups across a line; the grid is tiles x (groups of lines it strides over)
};

// kGt: the lines are the id image's rows, else rows of the planes
template <bool kGt>
__global__ __launch_bounds__(kThreads) void boundary_rows_kernel(RowArgs a) {
  __shared__ unsigned packed[kLines][kLineWords + 2 * kHalo];
  const int tw = threadIdx.x & (kLineWords - 1), lr = threadIdx.x / kLineWords;
  const int wc0 = (int)(blockIdx.x % a.tiles) * kLineWords;
  const long long groups = (a.lines + kLines - 1) / kLines;
  for (long long g = blockIdx.x / a.tiles; g < groups; g += gridDim.x / a.tiles) {
    const long long line = g * kLines + lr;
    const bool live = line < a.lines;
    const int plane = kGt || !live ? 0 : (int)(line / a.H), y = live ? (int)(line - (long long)plane * a.H) : 0;
    Clip c = clip_of(kGt ? nullptr : a.bounds, plane, a.H, a.W);
    const bool row_in = live && y >= c.y0 && y <= c.y1 && c.x0 <= c.x1;
    if (!__syncthreads_or(row_in)) continue;                              // no line of the group meets its bounds
    // this thread's word, and for the first 2 * kHalo threads of a line one word of the halo as well
    for (int pass = 0; pass < 2; ++pass) {
      if (pass && tw >= 2 * kHalo) break;
      const int slot = pass ? (tw < kHalo ? tw : kLineWords + tw) : tw + kHalo;
      const int wc = wc0 + slot - kHalo;
      unsigned bits = 0;
      if (row_in && wc >= 0 && wc < a.WB && wc >= (c.x0 >> 5) && wc <= (c.x1 >> 5)) {
        const int x = wc * 32, valid = min(32, a.W - x);
        if (kGt) {                                                       // bit k: ids[x + k] == ids[x + k - 1]
          const uint16_t* p = a.ids + (long long)y * a.W + x;
          int prev = x ? p[-1] : -1;
          for (int k = 0; k < valid; ++k) {
            const int v = p[k];
            bits |= (unsigned)(v == prev) << k;
            prev = v;
          }
        } else {
          bits = pack_nonzero(a.masks + ((long long)plane * a.H + y) * a.W + x, valid) & range_bits(wc, c.x0, c.x1);
        }
      }
      packed[lr][slot] = bits;
    }
    __syncthreads();
    const int wc = wc0 + tw;
    if (row_in && wc < a.WB && wc >= (c.x0 >> 5) && wc <= (c.x1 >> 5)) {
      const unsigned* mid = &packed[lr][tw + kHalo];
      const long long at = line * a.WB + wc;
      if (kGt) {
        a.gt_hsame[at] = *mid;
        a.gt_row_ok[at] = window_and(mid, 1 - a.d, 2 * a.d);
        const int x = wc * 32, valid = min(32, a.W - x);
        unsigned same = 0;
        if (y > 0) {
          const uint16_t* p = a.ids + (long long)y * a.W + x;
          for (int k = 0; k < valid; ++k) same |= (unsigned)(p[k] == p[k - a.W]) << k;
        }
        a.gt_vsame[at] = same;
      } else {
        a.mask_bits[at] = *mid;
        a.row_ok[at] = window_and(mid, -a.d, 2 * a.d + 1);
      }
    }
    __syncthreads();
  }
}

// The run lengths of 32 columns, bit-sliced: column k's count is 256 - w + run, bit j of it in bit k of c[j];
// `ok` is the carry out of it, sticky while the run lasts: run >= w.
struct Runs {
  unsigned c[8], ok;
  __device__ __forceinline__ void reset(int w) {
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = ((256 - w) >> j & 1) ? 0xffffffffu : 0u;
    ok = 0;
  }
  // one row: `row` the columns that pass it, `keep` those of them that continue the run above (the others start anew)
  __device__ __forceinline__ void add(unsigned row, unsigned keep, int w) {
    ok &= keep;
    unsigned carry = row & ~ok;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned start = ((256 - w) >> j & 1) ? 0xffffffffu : 0u;
      const unsigned v = (c[j] & keep) | (start & ~keep);
      c[j] = v ^ carry;
      carry &= v;
    }
    ok |= carry;
  }
};

struct ColArgs {
  const uint16_t* ids;        // [H][W]
  const uint16_t* table;      // [65536]: column + 1 of an id of interest
  const int* bounds;
  const unsigned* mask_bits;
  const unsigned* row_ok;
  const unsigned* gt_row_ok;
  const unsigned* gt_vsame;
  const unsigned* gt_hsame;
  unsigned* gt_band_bits;     // [H][WB]: written by the id image's pass, read by the planes'
  int* b_inter;               // [n][G]
  int* b_pred;                // [n]
  int* b_gt;                  // [G]
  uint8_t* pred_bands;        // [n][H][W] or null
  uint8_t* gt_band;           // [H][W] or null
  int n, G, H, W, WB, d;
  unsigned tiles;             // workgroups across a row; blockIdx.x = strip * tiles + tile
  int strip;                  // rows per strip of the planes' pass
};

__device__ __forceinline__ void write_band_bytes(uint8_t* dst, unsigned bits, int valid) {
  for (int k = 0; k < valid; ++k) dst[k] = (bits >> k & 1) ? 255 : 0;
}

// The pixels `rest` of a word into counters by id.  Bit k of `hsame`: pixel k has the id of the pixel to its left, so
// a run of equal ids costs one id load, one table look-up and one counter update.
__device__ __forceinline__ void count_by_id(unsigned rest, unsigned hsame, const uint16_t* p, const uint16_t* table,
                                            int* counters) {
  while (rest) {
    const int k = __ffs(rest) - 1;
    const unsigned breaks = ~hsame >> k >> 1;                             // bit j: pixel k + 1 + j starts another id
    const int len = breaks ? __ffs(breaks) : 32;                          // pixels k .. k + len - 1 share one
    const unsigned run = (k + len >= 32 ? 0xffffffffu : (1u << (k + len)) - 1) & (0xffffffffu << k);
    const int col = table[p[k]];
    if (col) atomicAdd(&counters[col - 1], __popc(rest & run));
    rest &= ~run;
  }
}

// Rows a thread of a columns pass loads before it works on them: its loads are independent of its state, so kChunk
// rows of every bit image are in flight at once instead of one load after the other.
constexpr int kChunk = 8;

// grid: strips of kGtStrip rows x tiles of kGtThreads word columns
__global__ __launch_bounds__(kGtThreads) void boundary_gt_columns_kernel(ColArgs a) {
  extern __shared__ int cnt[];                                            // [G]
  for (int k = threadIdx.x; k < a.G; k += kGtThreads) cnt[k] = 0;
  __syncthreads();
  const int w = 2 * a.d + 1;
  const int wc = (int)(blockIdx.x % a.tiles) * kGtThreads + threadIdx.x;
  const int y0 = (int)(blockIdx.x / a.tiles) * kGtStrip, y1 = min(y0 + kGtStrip, a.H);
  if (wc < a.WB) {
    const int x = wc * 32, valid = min(32, a.W - x);
    const unsigned inside = valid == 32 ? 0xffffffffu : (1u << valid) - 1;
    Runs runs;
    runs.reset(w);
    const int yend = y1 + a.d - 1;                                        // rows at and past H pass nothing
    for (int yc = max(y0 - a.d, 0); yc <= yend; yc += kChunk) {
      unsigned row[kChunk], same[kChunk], hs[kChunk];
#pragma unroll
      for (int j = 0; j < kChunk; ++j) {
        const int yy = yc + j, y = yy - a.d;
        const bool in = yy <= yend && yy < a.H, decide = yy <= yend && y >= y0;
        row[j] = in ? a.gt_row_ok[(long long)yy * a.WB + wc] : 0u;
        same[j] = in ? a.gt_vsame[(long long)yy * a.WB + wc] : 0u;
        hs[j] = decide ? a.gt_hsame[(long long)y * a.WB + wc] : 0u;
      }
#pragma unroll
      for (int j = 0; j < kChunk; ++j) {
        const int yy = yc + j, y = yy - a.d;
        if (yy > yend) break;
        runs.add(row[j], row[j] & same[j], w);
        if (y < y0) continue;
        const unsigned band = inside & ~runs.ok;
        a.gt_band_bits[(long long)y * a.WB + wc] = band;
        if (a.gt_band) write_band_bytes(a.gt_band + (long long)y * a.W + x, band, valid);
        count_by_id(band, hs[j], a.ids + (long long)y * a.W + x, a.table, cnt);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < a.G; k += kGtThreads)
    if (cnt[k]) atomicAdd(&a.b_gt[k], cnt[k]);
}

// grid: (strips of kStrip rows x tiles of kLineWords word columns), groups of kLines planes; a wave is one plane's tile
__global__ __launch_bounds__(kThreads) void boundary_plane_columns_kernel(ColArgs a) {
  extern __shared__ int cnt[];                                            // [kLines][G + 1]: columns, band pixels
  const int cols = a.G + 1;
  for (int k = threadIdx.x; k < kLines * cols; k += kThreads) cnt[k] = 0;
  __syncthreads();
  const int w = 2 * a.d + 1;
  const int tw = threadIdx.x & (kLineWords - 1), lr = threadIdx.x / kLineWords;
  const int wc = (int)(blockIdx.x % a.tiles) * kLineWords + tw, plane = blockIdx.y * kLines + lr;
  const int y0 = (int)(blockIdx.x / a.tiles) * a.strip, y1 = min(y0 + a.strip, a.H);
  if (plane < a.n && wc < a.WB) {
    const Clip c = clip_of(a.bounds, plane, a.H, a.W);
    // the mask is empty outside its bounds: nothing of this strip or word to decide there
    if (c.x0 <= c.x1 && wc >= (c.x0 >> 5) && wc <= (c.x1 >> 5) && max(y0, c.y0) <= min(y1 - 1, c.y1)) {
      const int x = wc * 32, valid = min(32, a.W - x);
      const unsigned* ok_bits = a.row_ok + (long long)plane * a.H * a.WB + wc;
      const unsigned* m_bits = a.mask_bits + (long long)plane * a.H * a.WB + wc;
      int* mine = cnt + lr * cols;
      int pixels = 0;
      Runs runs;
      runs.reset(w);
      // rows above the bounds pass nothing, which is the state after reset; rows below them end every run
      const int ya = max(y0, c.y0), yb = min(y1 - 1, c.y1);             // rows to decide
      const int yend = yb + a.d, ylast = min(yend, c.y1);               // rows to walk; the last of them with bits
      for (int yc = max(ya - a.d, c.y0); yc <= yend; yc += kChunk) {
        unsigned row[kChunk], mask[kChunk], gt[kChunk];
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
          const int yy = yc + j, y = yy - a.d;
          const bool decide = yy <= yend && y >= ya;
          row[j] = yy <= ylast ? ok_bits[(long long)yy * a.WB] : 0u;
          mask[j] = decide ? m_bits[(long long)y * a.WB] : 0u;
          gt[j] = decide ? a.gt_band_bits[(long long)y * a.WB + wc] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
          const int yy = yc + j, y = yy - a.d;
          if (yy > yend) break;
          runs.add(row[j], row[j], w);
          if (y < ya) continue;
          const unsigned band = mask[j] & ~runs.ok;
          if (a.pred_bands) write_band_bytes(a.pred_bands + ((long long)plane * a.H + y) * a.W + x, band, valid);
          pixels += __popc(band);
          const unsigned both = band & gt[j];
          if (both)
            count_by_id(both, a.gt_hsame[(long long)y * a.WB + wc], a.ids + (long long)y * a.W + x, a.table, mine);
        }
      }
      if (pixels) atomicAdd(&mine[a.G], pixels);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kLines * cols; k += kThreads) {
    const int v = cnt[k];
    if (!v) continue;
    const int l = k / cols, j = k - l * cols, i = blockIdx.y * kLines + l;
    atomicAdd(j < a.G ? a.b_inter + (long long)i * a.G + j : a.b_pred + i, v);
  }
}

// a band image is written only where a thread decides: the rest of it is zeroed first
__global__ __launch_bounds__(kThreads) void boundary_zero_kernel(uint8_t* p, long long bytes) {
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < bytes; k += (long long)gridDim.x * kThreads)
    p[k] = 0;
}

size_t table_bytes() { return cp_align_up((size_t)kIds * sizeof(uint16_t), 256); }
size_t image_words(int H, int W) { return (size_t)H * ((W + 31) / 32); }

}  // namespace

extern "C" size_t cp_boundary_overlaps_workspace_bytes(int32_t n, int32_t G, int32_t H, int32_t W, int32_t d) {
  (void)G; (void)d;
  if (n < 0 || H <= 0 || W <= 0) return 0;
  return table_bytes() + (4 + 2 * (size_t)n) * image_words(H, W) * sizeof(unsigned);
}

extern "C" int cp_boundary_overlaps(const uint8_t* masks, int32_t n, const int32_t* bounds, const uint16_t* gt_ids,
                                    int32_t H, int32_t W, int32_t d, const int32_t* inst_ids, int32_t G,
                                    int32_t* b_inter, int32_t* b_pred, int32_t* b_gt, uint8_t* pred_bands,
                                    uint8_t* gt_band, void* workspace, size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(n >= 0 && G >= 0 && H > 0 && W > 0 && d >= 1);
  const long long HW = (long long)H * W;
  if (n > kMaxMasks || G > kMaxInst || d > kMaxD || HW >= (1LL << 31)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(gt_ids && (n == 0 || (masks && b_pred)) && (G == 0 || (inst_ids && b_gt)) &&
               (n == 0 || G == 0 || b_inter));
  if (!workspace || workspace_bytes < cp_boundary_overlaps_workspace_bytes(n, G, H, W, d)) return CP_EWORKSPACE;
  CP_CHECK_ARG(((uintptr_t)workspace & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  const int WB = (W + 31) / 32;
  const size_t words = image_words(H, W);
  uint16_t* table = (uint16_t*)workspace;
  unsigned* base = (unsigned*)((char*)workspace + table_bytes());
  unsigned *gt_row_ok = base, *gt_vsame = base + words, *gt_band_bits = base + 2 * words, *gt_hsame = base + 3 * words;
  unsigned *mask_bits = base + 4 * words, *row_ok = mask_bits + (size_t)n * words;

  hipLaunchKernelGGL(boundary_prepare_kernel, dim3(1), dim3(1024), 0, st, inst_ids, G, table, b_inter, b_pred, b_gt, n);
  if (pred_bands && n && bounds) {
    const long long bytes = (long long)n * HW;
    hipLaunchKernelGGL(boundary_zero_kernel, dim3((unsigned)min((bytes + kThreads - 1) / kThreads, 65536LL)),
                       dim3(kThreads), 0, st, pred_bands, bytes);
  }
  RowArgs r;
  r.masks = masks; r.ids = gt_ids; r.bounds = bounds; r.mask_bits = mask_bits; r.row_ok = row_ok;
  r.gt_row_ok = gt_row_ok; r.gt_vsame = gt_vsame; r.gt_hsame = gt_hsame; r.H = H; r.W = W; r.WB = WB; r.d = d;
  const unsigned tiles = (WB + kLineWords - 1) / kLineWords;
  const long long max_groups = max(1u, kMaxBlocks / tiles);
  r.tiles = tiles;
  r.lines = H;
  hipLaunchKernelGGL(boundary_rows_kernel<true>,
                     dim3((unsigned)min((r.lines + kLines - 1) / kLines, max_groups) * tiles), dim3(kThreads), 0, st,
                     r);
  if (n) {
    r.lines = (long long)n * H;
    hipLaunchKernelGGL(boundary_rows_kernel<false>,
                       dim3((unsigned)min((r.lines + kLines - 1) / kLines, max_groups) * tiles), dim3(kThreads), 0, st,
                       r);
  }
  ColArgs c;
  c.ids = gt_ids; c.table = table; c.bounds = bounds; c.mask_bits = mask_bits; c.row_ok = row_ok;
  c.gt_row_ok = gt_row_ok; c.gt_vsame = gt_vsame; c.gt_hsame = gt_hsame; c.gt_band_bits = gt_band_bits;
  c.b_inter = b_inter;
  c.b_pred = b_pred; c.b_gt = b_gt; c.pred_bands = pred_bands; c.gt_band = gt_band;
  c.n = n; c.G = G; c.H = H; c.W = W; c.WB = WB; c.d = d;
  c.tiles = (WB + kGtThreads - 1) / kGtThreads;
  hipLaunchKernelGGL(boundary_gt_columns_kernel, dim3(c.tiles * ((H + kGtStrip - 1) / kGtStrip)), dim3(kGtThreads),
                     (size_t)max(G, 1) * sizeof(int), st, c);
  if (n) {
    c.tiles = tiles;
    c.strip = d < kWideFrom ? kStrip : kStripWide;
    hipLaunchKernelGGL(boundary_plane_columns_kernel,
                       dim3(tiles * ((H + c.strip - 1) / c.strip), (n + kLines - 1) / kLines),
                       dim3(kThreads), (size_t)kLines * (G + 1) * sizeof(int), st, c);
  }
  return cp_launch_status();
}
