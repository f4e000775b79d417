// Device PNG streams ("device PNG stream" in centerpoly_hip.h) for gfx950: the zlib stream of n grey images, 8 or 16
// bit, as one fixed-Huffman deflate block of run-length matches (distance D = bytes per pixel), built on the device so
// that only the compressed bytes go back to the host.
//
// The unit of work is a TILE: kTileBytes consecutive bytes of one image's filtered stream S (rows of a filter byte 0
// and W * D pixel bytes), a workgroup of 256 lanes, one PIECE of 16 bytes per lane.  A byte of S is "equal" when it
// equals its D-predecessor; the tokens of a maximal interval of equal bytes starting at a are the matches at a + 258 m
// and the literals of a remainder below 3, so a byte knows its token from the offset in its interval (mod 258) and the
// interval's end within the next 258 bytes.  Seven launches whatever n is, after one fill of the output with zeros:
//   png_runs_kernel    per tile: the equal bytes at its head and tail, Adler-32 partial sums, minimum and maximum
//   png_phase_kernel   one wave per image: segmented scan of the tails over the tiles -- every tile learns how many equal
//                      bytes lie right before it -- and the image's Adler-32 and value range
//   png_bits_kernel    per tile: the bits of the tokens whose first byte it owns
//   png_offsets_kernel one wave per image: exclusive scan of the bits
//   png_finish_kernel  one lane: byte lengths, the offsets over the images, table and head
//   png_emit_kernel    per tile: token bits into 32-bit words in LDS; whole words leave as vector stores, the two words
//                      a tile shares with its neighbours (and the header and trailer bytes) by an integer atomicOr into
//                      the zeroed output.  OR commutes: the same bytes on every run.
//   png_tail_kernel    one lane: the last cap_bytes % 4 bytes, which the emit kernel keeps in a word of the workspace so
//                      that no word store reaches beyond the capacity
// With bounds a byte outside the image's box is zero without a load.
#include "cp_common.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / CP_WAVE;
constexpr int kPiece = 16;                               // bytes of S per lane
constexpr int kTileBytes = kThreads * kPiece;            // bytes of S per workgroup
constexpr int kMaxMatch = 258;
constexpr int kMaxPlanes = 128, kMaxSide = 16384;
constexpr int kBig = 1 << 30;
// a tile owns at most 4095 literals of 9 bits and one match of 18, shifted by up to 31 bits: 1154 words
constexpr int kTileWords = 1160;

struct Src {
  const uint8_t* planes;      // [n][H][W] or null
  const int* images;          // [n][H][W] or null
  const int* bounds;          // [n][4] or null
  int n, H, W, D;             // D: bytes per pixel
  unsigned row;               // bytes of a row of S: 1 + W * D
  unsigned L;                 // bytes of S: H * row
  unsigned tiles;             // tiles per image
};

struct Box { int x0, y0, x1, y1; };

__device__ __forceinline__ Box load_box(const Src& q, int k) {
  Box b{0, 0, q.W - 1, q.H - 1};
  if (q.bounds) {
    b.x0 = max(q.bounds[4 * k], 0); b.y0 = max(q.bounds[4 * k + 1], 0);
    b.x1 = min(q.bounds[4 * k + 2], q.W - 1); b.y1 = min(q.bounds[4 * k + 3], q.H - 1);
  }
  return b;                                              // (an empty box holds no pixel: every test below fails)
}

struct TileRec {
  unsigned lead, tail;        // equal bytes at the tile's head / tail (both its length when all are equal)
  unsigned s1, s2;            // Adler-32 partial sums mod 65521: sum S[i], sum (L - i) S[i]
  int mn, mx;                 // range of the pixel values the tile touches
  unsigned before;            // equal bytes right before the tile (png_phase_kernel)
  unsigned bits;              // bits of the tokens it owns (png_bits_kernel)
};

struct PlaneRec {
  unsigned long long bits;    // token bits with the block header, without end-of-block
  long long off;              // byte offset of the zlib stream
  unsigned adler;
  int mn, mx, pad;
};

// The piece of lane `threadIdx.x` of tile `tile` of image k: v[i] = S[p0 + i], zero where S has no byte; eq bit i set
// where S[p0 + i] is equal (to S[p0 + i - D], with p0 + i >= D); valid = bytes of the piece inside S; mn, mx the range
// of the pixel values its bytes come from.
struct Piece {
  int v[kPiece];
  unsigned eq;
  int valid;
  int mn, mx;
};

__device__ __forceinline__ void load_piece(const Src& q, int k, unsigned tile, Piece& pc) {
  const long long p0 = (long long)tile * kTileBytes + (long long)threadIdx.x * kPiece;
  const Box b = load_box(q, k);
  const int D = q.D;
  pc.valid = (int)max(0LL, min((long long)kPiece, (long long)q.L - p0));
  pc.mn = INT32_MAX; pc.mx = INT32_MIN; pc.eq = 0;
  const long long j0 = p0 - D;                           // the cursor (row r, byte c of the row) starts D bytes early
  unsigned r = 0, c = 0;
  if (j0 >= 0 && j0 < (long long)q.L) { r = (unsigned)j0 / q.row; c = (unsigned)j0 - r * q.row; }
  const size_t plane = (size_t)k * q.H * q.W;
  int pre[2] = {0, 0};                                   // S[p0 - 2], S[p0 - 1]
#pragma unroll
  for (int i = -2; i < kPiece; ++i) {
    int byte = 0;
    const long long j = p0 + i;
    if (i >= -D && j >= 0 && j < (long long)q.L) {
      if (c != 0) {
        const int x = (int)(c - 1) / D, y = (int)r;
        int val = 0;
        if (x >= b.x0 && x <= b.x1 && y >= b.y0 && y <= b.y1) {
          const size_t at = plane + (size_t)y * q.W + x;
          val = q.planes ? (int)q.planes[at] : q.images[at];
        }
        if (i >= 0) { pc.mn = min(pc.mn, val); pc.mx = max(pc.mx, val); }
        byte = D == 1 ? (val & 0xff) : (((c - 1) & 1) ? (val & 0xff) : ((val >> 8) & 0xff));
      }
      if (++c == q.row) { c = 0; ++r; }
    }
    if (i < 0) pre[i + 2] = byte; else pc.v[i] = byte;
  }
#pragma unroll
  for (int i = 0; i < kPiece; ++i) {
    const int one = i >= 1 ? pc.v[i >= 1 ? i - 1 : 0] : pre[1];
    const int two = i >= 2 ? pc.v[i >= 2 ? i - 2 : 0] : pre[i >= 2 ? 0 : i];
    if (i < pc.valid && p0 + i >= D && pc.v[i] == (D == 1 ? one : two)) pc.eq |= 1u << i;
  }
}

// max of v over the lanes before this one (-1 when none) and over all; lds: kWaves ints
__device__ __forceinline__ void block_max_before(int v, int& before, int& all, int* lds) {
  const int lane = threadIdx.x & (CP_WAVE - 1), w = threadIdx.x / CP_WAVE;
  int inc = v;
#pragma unroll
  for (int o = 1; o < CP_WAVE; o <<= 1) {
    const int t = __shfl_up(inc, o, CP_WAVE);
    if (lane >= o) inc = max(inc, t);
  }
  int ex = __shfl_up(inc, 1, CP_WAVE);
  if (lane == 0) ex = -1;
  __syncthreads();
  if (lane == CP_WAVE - 1) lds[w] = inc;
  __syncthreads();
  all = -1;
  for (int j = 0; j < kWaves; ++j) {
    const int t = lds[j];
    if (j < w) ex = max(ex, t);
    all = max(all, t);
  }
  before = ex;
}

// min of v over the lanes after this one (kBig when none) and over all; lds: kWaves ints
__device__ __forceinline__ void block_min_after(int v, int& after, int& all, int* lds) {
  const int lane = threadIdx.x & (CP_WAVE - 1), w = threadIdx.x / CP_WAVE;
  int inc = v;
#pragma unroll
  for (int o = 1; o < CP_WAVE; o <<= 1) {
    const int t = __shfl_down(inc, o, CP_WAVE);
    if (lane + o < CP_WAVE) inc = min(inc, t);
  }
  int ex = __shfl_down(inc, 1, CP_WAVE);
  if (lane == CP_WAVE - 1) ex = kBig;
  __syncthreads();
  if (lane == 0) lds[w] = inc;
  __syncthreads();
  all = kBig;
  for (int j = 0; j < kWaves; ++j) {
    const int t = lds[j];
    if (j > w) ex = min(ex, t);
    all = min(all, t);
  }
  after = ex;
}

// sum of v over the lanes before this one and over all; lds: kWaves values
template <class T>
__device__ __forceinline__ void block_sum_before(T v, T& before, T& all, T* lds) {
  const int lane = threadIdx.x & (CP_WAVE - 1), w = threadIdx.x / CP_WAVE;
  T inc = v;
#pragma unroll
  for (int o = 1; o < CP_WAVE; o <<= 1) {
    const T t = __shfl_up(inc, o, CP_WAVE);
    if (lane >= o) inc += t;
  }
  T ex = inc - v;
  __syncthreads();
  if (lane == CP_WAVE - 1) lds[w] = inc;
  __syncthreads();
  all = 0;
  for (int j = 0; j < kWaves; ++j) {
    const T t = lds[j];
    if (j < w) ex += t;
    all += t;
  }
  before = ex;
}

// the local indices (in the tile) of the piece's last byte that is not equal (-1: none) and of its first byte that is
// not equal or lies beyond S (kBig: none)
__device__ __forceinline__ void piece_ends(const Piece& pc, int& last_ne, int& first_ne) {
  const int q0 = (int)threadIdx.x * kPiece;
  const unsigned in = pc.valid >= kPiece ? 0xffffu : ((1u << pc.valid) - 1u);
  const unsigned ne = ~pc.eq & in;                       // not equal, inside S
  const unsigned stop = ~pc.eq & 0xffffu;                // not equal, or beyond S
  last_ne = ne ? q0 + 31 - __clz((int)ne) : -1;
  first_ne = stop ? q0 + __ffs((int)stop) - 1 : kBig;
}

__device__ __forceinline__ unsigned tile_len(const Src& q, unsigned tile) {
  return min((unsigned)kTileBytes, q.L - tile * (unsigned)kTileBytes);
}

__global__ __launch_bounds__(kThreads) void png_runs_kernel(Src q, TileRec* __restrict__ recs) {
  __shared__ int lds[kWaves];
  __shared__ unsigned long long lds64[kWaves];
  const int k = blockIdx.y;
  const unsigned tile = blockIdx.x;
  Piece pc;
  load_piece(q, k, tile, pc);
  int last_ne, first_ne;
  piece_ends(pc, last_ne, first_ne);
  int before, last_all, after, first_all;
  block_max_before(last_ne, before, last_all, lds);
  block_min_after(first_ne, after, first_all, lds);
  const long long p0 = (long long)tile * kTileBytes + (long long)threadIdx.x * kPiece;
  unsigned long long a = 0, b = 0;
#pragma unroll
  for (int i = 0; i < kPiece; ++i) {
    if (i < pc.valid) {
      a += (unsigned)pc.v[i];
      b += (unsigned long long)((long long)q.L - (p0 + i)) * (unsigned)pc.v[i];
    }
  }
  unsigned long long ex, sa, sb;
  block_sum_before(a, ex, sa, lds64);
  block_sum_before(b, ex, sb, lds64);
  int mn = pc.mn, mx = pc.mx;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o, CP_WAVE));
    mx = max(mx, __shfl_xor(mx, o, CP_WAVE));
  }
  __syncthreads();
  if ((threadIdx.x & (CP_WAVE - 1)) == 0) lds[threadIdx.x / CP_WAVE] = mn;
  __syncthreads();
  for (int j = 0; j < kWaves; ++j) mn = min(mn, lds[j]);
  __syncthreads();
  if ((threadIdx.x & (CP_WAVE - 1)) == 0) lds[threadIdx.x / CP_WAVE] = mx;
  __syncthreads();
  for (int j = 0; j < kWaves; ++j) mx = max(mx, lds[j]);
  if (threadIdx.x == 0) {
    const int len = (int)tile_len(q, tile);
    TileRec r;
    r.lead = (unsigned)min(first_all, len);
    r.tail = (unsigned)(len - 1 - last_all);
    r.s1 = (unsigned)(sa % 65521u); r.s2 = (unsigned)(sb % 65521u);
    r.mn = mn; r.mx = mx; r.before = 0; r.bits = 0;
    recs[(size_t)k * q.tiles + tile] = r;
  }
}

// Segmented scan over the tiles of one image: `before` of a tile is the number of equal bytes that end right before
// it.  {full, cnt}: all bytes of the segment equal; the equal bytes at its tail.
struct Seg { unsigned full, cnt; };
__device__ __forceinline__ Seg merge(Seg a, Seg b) {     // a earlier, b later
  return Seg{a.full & b.full, b.full ? a.cnt + b.cnt : b.cnt};
}

__global__ __launch_bounds__(CP_WAVE) void png_phase_kernel(Src q, TileRec* __restrict__ recs,
                                                           PlaneRec* __restrict__ planes) {
  const int k = blockIdx.x, lane = threadIdx.x;
  TileRec* rec = recs + (size_t)k * q.tiles;
  Seg carry{1, 0};
  unsigned long long s1 = 0, s2 = 0;
  int mn = INT32_MAX, mx = INT32_MIN;
  for (unsigned base = 0; base < q.tiles; base += CP_WAVE) {
    const unsigned t = base + lane;
    Seg v{1, 0};
    if (t < q.tiles) {
      const TileRec r = rec[t];
      v = Seg{r.tail == tile_len(q, t) ? 1u : 0u, r.tail};
      s1 += r.s1; s2 += r.s2;
      mn = min(mn, r.mn); mx = max(mx, r.mx);
    }
    Seg inc = v;
#pragma unroll
    for (int o = 1; o < CP_WAVE; o <<= 1) {
      const Seg u{__shfl_up(inc.full, o, CP_WAVE), __shfl_up(inc.cnt, o, CP_WAVE)};
      if (lane >= o) inc = merge(u, inc);
    }
    Seg ex{__shfl_up(inc.full, 1, CP_WAVE), __shfl_up(inc.cnt, 1, CP_WAVE)};
    if (lane == 0) ex = Seg{1, 0};
    if (t < q.tiles) rec[t].before = merge(carry, ex).cnt;
    const Seg tot{__shfl(inc.full, CP_WAVE - 1, CP_WAVE), __shfl(inc.cnt, CP_WAVE - 1, CP_WAVE)};
    carry = merge(carry, tot);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, CP_WAVE); s2 += __shfl_xor(s2, o, CP_WAVE);
    mn = min(mn, __shfl_xor(mn, o, CP_WAVE)); mx = max(mx, __shfl_xor(mx, o, CP_WAVE));
  }
  if (lane == 0) {
    const unsigned a = (unsigned)((1u + s1) % 65521u), b = (unsigned)((q.L + s2) % 65521u);
    planes[k].adler = (b << 16) | a;
    planes[k].mn = mn; planes[k].mx = mx; planes[k].pad = 0;
  }
}

// ---- tokens

__device__ __forceinline__ unsigned reverse_bits(unsigned v, int n) { return __brev(v) >> (32 - n); }

struct Token { unsigned code; int n; };                  // n bits, the first of them in bit 0

__device__ __forceinline__ Token literal_token(int v) {
  return v < 144 ? Token{reverse_bits(0x30 + v, 8), 8} : Token{reverse_bits(0x190 + v - 144, 9), 9};
}

__device__ __forceinline__ Token match_token(int len, int D) {
  int k, e;
  const int l = len - 3;
  if (len == kMaxMatch) { k = 28; e = 0; }
  else if (l < 8) { k = l; e = 0; }
  else { e = 29 - __clz(l); k = 4 * e + 4 + ((l >> e) & 3); }       // e = floor(log2 l) - 2
  const int sym = 257 + k;
  Token t = sym <= 279 ? Token{reverse_bits(sym - 256, 7), 7} : Token{reverse_bits(0xC0 + sym - 280, 8), 8};
  t.code |= (unsigned)(l & ((1 << e) - 1)) << t.n;       // (e == 0: no bits)
  t.n += e;
  t.code |= reverse_bits(D - 1, 5) << t.n;
  t.n += 5;
  return t;
}

// What a lane needs beside its piece to know its tokens: m0, the offset of its first byte in that byte's interval of
// equal bytes, mod 258; next_ne, the local index of the first byte after the piece that is not equal or ends S (beyond
// the tile: the tile's length plus the equal bytes that follow it, as far as a match reaches).  lds: kWaves ints.
struct Walk { int m0, next_ne; };

__device__ __forceinline__ Walk piece_walk(const Src& q, const TileRec* __restrict__ rec, unsigned tile, const Piece& pc,
                                           int* lds) {
  int last_ne, first_ne;
  piece_ends(pc, last_ne, first_ne);
  int prev_ne, next_ne, all;
  block_max_before(last_ne, prev_ne, all, lds);
  block_min_after(first_ne, next_ne, all, lds);
  const int q0 = (int)threadIdx.x * kPiece;
  if (next_ne == kBig) {                                 // equal up to the end of a whole tile: look ahead
    const unsigned ahead = tile + 1 < q.tiles ? min(rec[tile + 1].lead, (unsigned)kMaxMatch) : 0u;
    next_ne = (int)tile_len(q, tile) + (int)ahead;
  }
  Walk w;
  w.m0 = prev_ne >= 0 ? (q0 - prev_ne - 1) % kMaxMatch : (int)((rec[tile].before % kMaxMatch + (unsigned)q0) % kMaxMatch);
  w.next_ne = next_ne;
  return w;
}

// The tokens whose first byte lies in this lane's piece, in order: put(Token).  Counting and emitting take the same
// walk.
template <class F>
__device__ __forceinline__ void piece_tokens(const Src& q, const Piece& pc, const Walk& w, F&& put) {
  const int q0 = (int)threadIdx.x * kPiece;
  const unsigned stop = ~pc.eq & 0xffffu;                // not equal, or beyond S
  int m = w.m0;
#pragma unroll
  for (int i = 0; i < kPiece; ++i) {
    if (i < pc.valid) {
      const int byte = pc.v[i];
      if (!(pc.eq >> i & 1)) {
        put(literal_token(byte));
        m = 0;
      } else {
        const unsigned later = stop >> i;                // (bit 0 is clear: this byte is equal)
        const int rem = later ? __ffs((int)later) - 1 : w.next_ne - (q0 + i);
        if (m == 0) {
          const int c = min(rem, kMaxMatch);
          if (c >= 3) put(match_token(c, q.D)); else put(literal_token(byte));
        } else if (m == 1 && rem == 1) {                 // the second byte of a remainder of two
          put(literal_token(byte));
        }
        if (++m == kMaxMatch) m = 0;
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void png_bits_kernel(Src q, TileRec* __restrict__ recs) {
  __shared__ int lds[kWaves];
  __shared__ unsigned ldsu[kWaves];
  const int k = blockIdx.y;
  const unsigned tile = blockIdx.x;
  TileRec* rec = recs + (size_t)k * q.tiles;
  Piece pc;
  load_piece(q, k, tile, pc);
  unsigned bits = 0;
  const Walk w = piece_walk(q, rec, tile, pc, lds);
  piece_tokens(q, pc, w, [&](Token t) { bits += (unsigned)t.n; });
  unsigned ex, all;
  block_sum_before(bits, ex, all, ldsu);
  if (threadIdx.x == 0) rec[tile].bits = all;
}

__global__ __launch_bounds__(CP_WAVE) void png_offsets_kernel(Src q, const TileRec* __restrict__ recs,
                                                             unsigned long long* __restrict__ bitoff,
                                                             PlaneRec* __restrict__ planes) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const TileRec* rec = recs + (size_t)k * q.tiles;
  unsigned long long carry = 3;                          // BFINAL and BTYPE
  for (unsigned base = 0; base < q.tiles; base += CP_WAVE) {
    const unsigned t = base + lane;
    const unsigned long long v = t < q.tiles ? rec[t].bits : 0;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < CP_WAVE; o <<= 1) {
      const unsigned long long u = __shfl_up(inc, o, CP_WAVE);
      if (lane >= o) inc += u;
    }
    if (t < q.tiles) bitoff[(size_t)k * q.tiles + t] = carry + inc - v;
    carry += __shfl(inc, CP_WAVE - 1, CP_WAVE);
  }
  if (lane == 0) planes[k].bits = carry;
}

__device__ __forceinline__ int clamp_i32(long long v) { return v > 2147483647LL ? 2147483647 : (int)v; }

__global__ __launch_bounds__(CP_WAVE) void png_finish_kernel(int n, PlaneRec* __restrict__ planes, int* __restrict__ table,
                                                            int* __restrict__ head, long long cap_bytes) {
  if (threadIdx.x != 0) return;
  long long off = 0;
  for (int k = 0; k < n; ++k) {
    // header 2, the block with its 7 bits of end-of-block padded to a byte, Adler-32
    const long long len = 2 + (long long)((planes[k].bits + 7 + 7) / 8) + 4;
    planes[k].off = off;
    table[4 * k] = clamp_i32(off); table[4 * k + 1] = clamp_i32(len);
    table[4 * k + 2] = planes[k].mn; table[4 * k + 3] = planes[k].mx;
    off += len;
  }
  head[0] = clamp_i32(off); head[1] = off > cap_bytes ? 1 : 0; head[2] = 0; head[3] = 0;
}

struct Out {
  unsigned* words;            // the output as 32-bit words
  unsigned* tail_word;        // stands in for word cap_bytes / 4 when cap_bytes % 4 != 0
  long long cap_bytes;
};

// the word w of the output: null where it lies beyond the capacity
__device__ __forceinline__ unsigned* word_at(const Out& o, long long w) {
  if ((w + 1) * 4 <= o.cap_bytes) return o.words + w;
  if (w * 4 < o.cap_bytes) return o.tail_word;
  return nullptr;
}

__device__ __forceinline__ void or_byte(const Out& o, long long at, unsigned byte) {
  unsigned* p = word_at(o, at >> 2);
  if (p) atomicOr(p, byte << (8 * (int)(at & 3)));
}

__global__ __launch_bounds__(kThreads) void png_emit_kernel(Src q, const TileRec* __restrict__ recs,
                                                           const unsigned long long* __restrict__ bitoff,
                                                           const PlaneRec* __restrict__ planes,
                                                           const int* __restrict__ head, Out o) {
  __shared__ int lds[kWaves];
  __shared__ unsigned ldsu[kWaves];
  __shared__ unsigned words[kTileWords];
  if (head[1]) return;                                   // too small: nothing is written (uniform over the grid)
  const int k = blockIdx.y;
  const unsigned tile = blockIdx.x;
  const TileRec* rec = recs + (size_t)k * q.tiles;
  for (int i = threadIdx.x; i < kTileWords; i += kThreads) words[i] = 0;
  Piece pc;
  load_piece(q, k, tile, pc);
  unsigned bits = 0;
  const Walk w = piece_walk(q, rec, tile, pc, lds);
  piece_tokens(q, pc, w, [&](Token t) { bits += (unsigned)t.n; });
  unsigned ex, all;
  block_sum_before(bits, ex, all, ldsu);                 // (the barriers order the zeroing of `words` before the ORs)
  const PlaneRec pr = planes[k];
  const unsigned long long g0 = ((unsigned long long)pr.off + 2) * 8 + bitoff[(size_t)k * q.tiles + tile];
  const int lead = (int)(g0 & 31);
  {
    const unsigned at = (unsigned)lead + ex;
    int wi = (int)(at >> 5), nacc = (int)(at & 31);
    unsigned long long acc = 0;
    piece_tokens(q, pc, w, [&](Token t) {
      acc |= (unsigned long long)t.code << nacc;
      nacc += t.n;
      if (nacc >= 32) {
        atomicOr(&words[wi], (unsigned)acc);
        ++wi; acc >>= 32; nacc -= 32;
      }
    });
    if (nacc > 0 && acc != 0) atomicOr(&words[wi], (unsigned)acc);
  }
  __syncthreads();
  const unsigned long long g1 = g0 + all;
  const long long w0 = (long long)(g0 >> 5);
  const int nw = (int)((lead + all + 31) >> 5);
  for (int i = threadIdx.x; i < nw; i += kThreads) {
    const bool whole = (i > 0 || lead == 0) && (i < nw - 1 || (g1 & 31) == 0);
    unsigned* p = word_at(o, w0 + i);
    if (!p) continue;
    if (whole) *p = words[i]; else if (words[i]) atomicOr(p, words[i]);
  }
  if (threadIdx.x == 0 && tile == 0) {                   // zlib header; BFINAL = 1, BTYPE = 01
    or_byte(o, pr.off, 0x78);
    or_byte(o, pr.off + 1, 0x01);
    or_byte(o, pr.off + 2, 0x03);
  }
  if (threadIdx.x == 0 && tile == q.tiles - 1) {         // end-of-block is seven zero bits, the padding more; Adler-32
    const long long end = pr.off + 2 + (long long)((pr.bits + 7 + 7) / 8);
    or_byte(o, end, pr.adler >> 24);
    or_byte(o, end + 1, (pr.adler >> 16) & 0xff);
    or_byte(o, end + 2, (pr.adler >> 8) & 0xff);
    or_byte(o, end + 3, pr.adler & 0xff);
  }
}

__global__ __launch_bounds__(CP_WAVE) void png_tail_kernel(const int* __restrict__ head, Out o, uint8_t* __restrict__ out) {
  if (threadIdx.x != 0 || head[1]) return;
  const long long base = o.cap_bytes & ~3LL;
  const unsigned w = *o.tail_word;
  for (long long i = base; i < o.cap_bytes; ++i) out[i] = (uint8_t)(w >> (8 * (int)(i - base)));
}

bool shape_ok(int n, int H, int W, int bits) { return n >= 1 && H >= 1 && W >= 1 && (bits == 8 || bits == 16); }
bool shape_supported(int n, int H, int W, int bits) {
  if (n > kMaxPlanes || H > kMaxSide || W > kMaxSide) return false;
  return (long long)n * H * (1 + (long long)W * (bits / 8)) < (1LL << 31);
}
unsigned tiles_of(int H, int W, int bits) {
  const long long L = (long long)H * (1 + (long long)W * (bits / 8));
  return (unsigned)((L + kTileBytes - 1) / kTileBytes);
}
size_t deflate_bytes(int n, int H, int W, int bits) {
  const size_t nt = (size_t)n * tiles_of(H, W, bits);
  return nt * (sizeof(TileRec) + sizeof(unsigned long long)) + kMaxPlanes * sizeof(PlaneRec) + 16;
}

}  // namespace

extern "C" size_t cp_png_deflate_workspace_bytes(int32_t n, int32_t H, int32_t W, int32_t bits) {
  if (!shape_ok(n, H, W, bits) || !shape_supported(n, H, W, bits)) return 0;
  return deflate_bytes(n, H, W, bits);
}

extern "C" int cp_png_deflate(const uint8_t* planes_u8, const int32_t* images_i32, int32_t n, int32_t H, int32_t W,
                              int32_t bits, const int32_t* bounds, uint8_t* out, int64_t cap_bytes, int32_t* table,
                              int32_t* head, void* workspace, size_t workspace_bytes, void* stream) {
  CP_CHECK_ARG(shape_ok(n, H, W, bits) && cap_bytes >= 0);
  CP_CHECK_ARG((planes_u8 != nullptr) != (images_i32 != nullptr));
  CP_CHECK_ARG(!planes_u8 || bits == 8);
  if (!shape_supported(n, H, W, bits)) return CP_EUNSUPPORTED;
  CP_CHECK_ARG(table && head && (out || cap_bytes == 0));
  CP_CHECK_ARG(((uintptr_t)bounds & 3) == 0 && ((uintptr_t)images_i32 & 3) == 0 && ((uintptr_t)table & 3) == 0 &&
               ((uintptr_t)head & 3) == 0 && ((uintptr_t)out & 3) == 0);
  if (!workspace || workspace_bytes < deflate_bytes(n, H, W, bits)) return CP_EWORKSPACE;
  CP_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
  hipStream_t st = (hipStream_t)stream;
  Src q;
  q.planes = planes_u8; q.images = images_i32; q.bounds = bounds; q.n = n; q.H = H; q.W = W; q.D = bits / 8;
  q.row = 1u + (unsigned)W * (unsigned)q.D;
  q.L = (unsigned)H * q.row;
  q.tiles = tiles_of(H, W, bits);
  const size_t nt = (size_t)n * q.tiles;
  TileRec* recs = (TileRec*)workspace;
  unsigned long long* bitoff = (unsigned long long*)(recs + nt);
  PlaneRec* prec = (PlaneRec*)(bitoff + nt);
  Out o;
  o.words = (unsigned*)out; o.tail_word = (unsigned*)(prec + kMaxPlanes); o.cap_bytes = out ? cap_bytes : 0;
  if (hipMemsetAsync(o.tail_word, 0, 16, st) != hipSuccess) return CP_EHIP;
  if (o.cap_bytes > 0 && hipMemsetAsync(out, 0, (size_t)o.cap_bytes, st) != hipSuccess) return CP_EHIP;
  const dim3 grid(q.tiles, n);
  hipLaunchKernelGGL(png_runs_kernel, grid, dim3(kThreads), 0, st, q, recs);
  hipLaunchKernelGGL(png_phase_kernel, dim3(n), dim3(CP_WAVE), 0, st, q, recs, prec);
  hipLaunchKernelGGL(png_bits_kernel, grid, dim3(kThreads), 0, st, q, recs);
  hipLaunchKernelGGL(png_offsets_kernel, dim3(n), dim3(CP_WAVE), 0, st, q, (const TileRec*)recs, bitoff, prec);
  hipLaunchKernelGGL(png_finish_kernel, dim3(1), dim3(CP_WAVE), 0, st, (int)n, prec, table, head, o.cap_bytes);
  hipLaunchKernelGGL(png_emit_kernel, grid, dim3(kThreads), 0, st, q, (const TileRec*)recs,
                     (const unsigned long long*)bitoff, (const PlaneRec*)prec, (const int*)head, o);
  if (o.cap_bytes & 3)
    hipLaunchKernelGGL(png_tail_kernel, dim3(1), dim3(CP_WAVE), 0, st, (const int*)head, o, out);
  return cp_launch_status();
}
