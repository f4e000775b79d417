// 1x1 / stride 1 forward convolution of the channel concatenation of 1-4 float32 NCHW sources, streamed through
// registers (gfx950): what `Root` and `Tree.project` run at inference (reference: src/lib/models/networks/
// pose_dla_dcn.py:148-166 Root, :206-213 project), + bias + residual + ReLU, float32 NCHW out.
//
// Why a kernel of its own: these layers carry ~5 % of the step's flops and move 6-100 MB each -- they are bandwidth
// problems.  conv_mfma_kernel<.., TAPS = 1> stages every 32-channel chunk through LDS between two barriers with no
// double buffer, so each chunk exposes a whole HBM round trip.  Here nothing is staged -- and every output element is
// the SAME sequence of floating-point operations as in that kernel, so the two give the same bits:
//
//   * The contraction is conv_mfma_kernel's: v_mfma_f32_16x16x32_bf16 over 32-channel chunks in ascending order, pixels
//     on the M side, channels on the N side, three products per chunk in its order (x_hi w_hi, x_lo w_hi, x_hi w_lo), its
//     split of a float into bf16 halves, its prepared weights (cp_conv_mfma_prepare, taps = 1) read as they are, its
//     epilogue order (+ bias, + residual, ReLU).  Its in-workgroup K split is kept too: KS wave groups take the chunks
//     q, q + KS, ... and the partial tiles are added in group order -- the caller passes the KS that kernel would pick.
//   * A pixel is a position in the flattened H x W plane (a 1x1 convolution does not know rows).  Lane (pixel = lane &
//     15, group = lane >> 4) loads the channels 8 group .. 8 group + 7 of the chunk for its pixel -- eight dword buffer
//     loads from eight planes, 4 x 64 contiguous bytes per wave instruction -- and those eight values ARE its A fragment.
//   * The loads of the wave's chunk after next are issued around the MFMAs of the current one: the activations before
//     them, the weight fragments right after, into the registers those MFMAs read.  Both run at the same depth on
//     purpose: the vector memory counter retires in issue order, so a weight fragment fetched only one step ahead would
//     make its wait drain every activation load issued before it.
//   * A workgroup is four waves: 4 / KS neighbouring pixel tiles of one 64-channel block x KS waves per tile.  The
//     partial tiles of a K split meet in LDS once, after the loop: the only LDS and the only barrier of the kernel.
//   * Every global access of a tensor is a buffer access with range checking: a lane past the plane, a channel past the
//     source or past Cout, a chunk past the wave's range get an offset beyond num_records -- loads return 0, stores are
//     dropped.  No edge path.  The accumulator tile gives a lane four consecutive pixels of one channel: 16-byte residual
//     loads and stores where H W is a multiple of 4 and the tensors are 16-byte aligned, dwords otherwise.
#include <type_traits>

#include "cp_common.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int MAXSRC = 4;
constexpr int KC = 32;                    // input channels per chunk (one 16x16x32 MFMA), as in conv_mfma.hip
constexpr int CB = 64;                    // output channels per workgroup: four 16-row weight tiles
constexpr int MT = CB / 16;
#ifndef CP_STREAM_DEPTH
#define CP_STREAM_DEPTH 2
#endif
constexpr int DEPTH = CP_STREAM_DEPTH;    // chunks of loads in flight per wave
constexpr unsigned OOB = 0x80000000u;     // voffset past every num_records (< 2^31, also with the scalar offset added)

struct StreamArgs {
  const float* xsrc[MAXSRC];   // the input is the channel concatenation of up to 4 tensors [B][csrc[i]][H][W]
  int csrc[MAXSRC];            // several sources: each a multiple of 16 (HALF: a chunk may straddle two of them)
  const bf16x8* wp;            // cp_conv_mfma_prepare's fragments, taps = 1
  const float* bias;           // [Cout] or null
  const float* res;            // same shape as out, or null
  float* out;
  int Cin, Cout, HW, nchunk, ncb, relu, vec;
};

// fp32 pair -> bf16 hi pair + bf16 lo pair: hi = bf16(v), lo = bf16(v - hi), round to nearest even -- the split of
// conv_mfma_kernel's staging (and dcn_fwd_region.hip's split2)
__device__ __forceinline__ void split2(float v0, float v1, unsigned& hi, unsigned& lo) {
  const bf16x2 h = __builtin_convertvector(f32x2{v0, v1}, bf16x2);
  const unsigned hb = __builtin_bit_cast(unsigned, h);
  const float h0 = __builtin_bit_cast(float, hb << 16), h1 = __builtin_bit_cast(float, hb & 0xffff0000u);
  const bf16x2 l = __builtin_convertvector(f32x2{v0 - h0, v1 - h1}, bf16x2);
  hi = hb;
  lo = __builtin_bit_cast(unsigned, l);
}

// Workgroup = 4 waves = 4 / KS neighbouring tiles (64 output channels x 16 NT pixels each) of ONE 64-channel block x KS
// waves per tile; wave q of a tile takes the chunks q, q + KS, ...  HALF: the two 16-channel halves of a chunk are
// looked up separately (sources that are odd multiples of 16 channels).
template <int NT, int KS, bool HALF>
__global__ __launch_bounds__(256, 2) void conv1x1_stream_kernel(StreamArgs a) {
  constexpr int PG = 4 / KS;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q = wave % KS, grp = wave / KS;
  const int c = lane & 15, g = lane >> 4;
  // XCD-aware order (conv_mfma.hip): the workgroups that read the SAME pixels -- one per 64-channel block -- are logical
  // neighbours and share an XCD, and with it the pixels' lines in L2
  int lw = blockIdx.x;
  if ((gridDim.x & 7) == 0) lw = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const int cb = lw % a.ncb, pg = (lw / a.ncb) * PG + grp, b = blockIdx.y;     // (a tile past the plane: all lanes OOB)
  const int HW = a.HW, P0 = pg * 16 * NT;
  const unsigned plane = (unsigned)HW * 4u;

  // this lane's pixel of tile n in the first channel of its group of eight (HALF: of its half's group), or OOB
  unsigned vin[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int p = P0 + 16 * n + c;
    vin[n] = p < HW ? ((unsigned)(8 * (HALF ? g & 1 : g)) * (unsigned)HW + (unsigned)p) * 4u : OOB;
  }

  const long long tstride = (long long)a.nchunk * 128;         // fragments per 16-row weight tile
  const bf16x8* wq = a.wp + (long long)cb * MT * tstride + lane;
  const int nmine = a.nchunk > q ? (a.nchunk - q + KS - 1) / KS : 0;          // chunks of this wave: q, q + KS, ...

  // The loads of the wave's i-th chunk: 8 NT activation dwords (issue_x) and the 8 weight fragments (issue_w).  Past
  // the wave's range the activation offsets are OOB (no memory traffic) and the weight chunk is clamped (a re-read of
  // cached lines).  The source of a chunk is picked with scalar selects, not branches: the K loop stays one basic
  // block, which is what lets the compiler count the loads in flight instead of draining them at every join.
  const int e0 = a.csrc[0], e1 = e0 + a.csrc[1], e2 = e1 + a.csrc[2];     // first channels of the sources 1, 2, 3
  auto source = [&](int cc, int& cl) __attribute__((always_inline)) {      // channel cc -> descriptor, channel in it
    const bool g0 = cc >= e0, g1 = cc >= e1, g2 = cc >= e2;
    cl = cc - (g2 ? e2 : g1 ? e1 : g0 ? e0 : 0);
    // (an absent source starts at Cin: 0 channels behind a null pointer, 0 records -- every load returns 0)
    const int cs = g2 ? a.Cin - e2 : g1 ? a.csrc[2] : g0 ? a.csrc[1] : e0;
    const float* xp = g2 ? a.xsrc[3] : g1 ? a.xsrc[2] : g0 ? a.xsrc[1] : a.xsrc[0];
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xp + (long long)b * cs * HW), 0, (int)((unsigned)cs * plane),
                                             0x00020000);
  };
  auto issue_x = [&](int i, float (&v)[NT][8]) __attribute__((always_inline)) {
    const bool live = i < nmine;
    const int cc = live ? (q + i * KS) * KC : 0;
    int cA, cB;
    const __amdgpu_buffer_rsrc_t rsA = source(cc, cA);
    if constexpr (HALF) {
      const __amdgpu_buffer_rsrc_t rsB = source(cc + 16, cB);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const unsigned va = live && g < 2 ? vin[n] : OOB, vb = live && g >= 2 ? vin[n] : OOB;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned x0 = __builtin_amdgcn_raw_buffer_load_b32(rsA, va, (unsigned)(cA + j) * plane, 0);
          const unsigned x1 = __builtin_amdgcn_raw_buffer_load_b32(rsB, vb, (unsigned)(cB + j) * plane, 0);
          v[n][j] = __builtin_bit_cast(float, x0 | x1);         // (the half that is not the lane's reads 0)
        }
      }
    } else {
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const unsigned vo = live ? vin[n] : OOB;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[n][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsA, vo, (unsigned)(cA + j) * plane, 0));
      }
    }
  };
  auto issue_w = [&](int i, bf16x8 (&w)[MT][2]) __attribute__((always_inline)) {
    const bf16x8* wsrc = wq + (long long)min(q + i * KS, a.nchunk - 1) * 128;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      w[m][0] = wsrc[m * tstride];
      w[m][1] = wsrc[m * tstride + 64];
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  float v[DEPTH][NT][8];
  bf16x8 w[DEPTH][MT][2];
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) {       // (in the loop's own issue order: its waits are counted from both ways in)
    issue_x(d, v[d]);
    __builtin_amdgcn_sched_barrier(0);
    issue_w(d, w[d]);
    __builtin_amdgcn_sched_barrier(0);
  }

  // No guard inside: a chunk past the range multiplies the zeros its loads returned (at most DEPTH - 1 of them per wave;
  // x + 0 leaves every bit of x).
  for (int i = 0; i < nmine; i += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      bf16x8 xh[NT], xl[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        unsigned hi[4], lo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) split2(v[d][n][2 * j], v[d][n][2 * j + 1], hi[j], lo[j]);
        xh[n] = __builtin_bit_cast(bf16x8, hi);
        xl[n] = __builtin_bit_cast(bf16x8, lo);
      }
      issue_x(i + d + DEPTH, v[d]);                             // DEPTH chunks ahead, before this chunk's MFMAs
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[n], w[d][m][0], acc[m][n], 0, 0, 0);
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl[n], w[d][m][0], acc[m][n], 0, 0, 0);
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[n], w[d][m][1], acc[m][n], 0, 0, 0);
        }
      // the fragments are reloaded in place once the MFMAs have read them (a copy held across the loads would come back
      // as a loop-carried move of just-loaded registers: a wait for the newest loads in every step)
      __builtin_amdgcn_sched_barrier(0);
      issue_w(i + d + DEPTH, w[d]);
    }
  }

  // ------------------------------------------------------------------ epilogue: D[pixel 4 g + r][co = c]
  // Tile t = m NT + n of the wave tile is finished by wave t % KS of its group.  The residual loads of ALL its tiles are
  // issued first (the prefetch registers are free now), ahead of the LDS exchange: one exposed round trip per wave.
  constexpr int NTILE = MT * NT;
  const unsigned obytes = (unsigned)a.Cout * plane;
  const __amdgpu_buffer_rsrc_t rs_o =
      __builtin_amdgcn_make_buffer_rsrc(a.out + (long long)b * a.Cout * HW, 0, (int)obytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_r = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.res ? a.res + (long long)b * a.Cout * HW : a.out), 0, a.res ? (int)obytes : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_b =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, a.bias ? a.Cout * 4 : 0, 0x00020000);
  // K split: the partial tiles go to LDS, once (added below in group order: conv_mfma_kernel's acc0 += acc1, += acc2 ...)
  __shared__ f32x4 red[KS > 1 ? 4 * NTILE * 64 : 1];           // [wave][tile][lane]
  // (one body per access width, chosen once: a branch per tile would put a full wait between the tiles)
  auto finish = [&](auto wide) __attribute__((always_inline)) {
    constexpr bool VEC = decltype(wide)::value;
    float bv[MT];
    unsigned off[MT][NT];                 // channel 64 cb + 16 m + c, pixels P0 + 16 n + 4 g ..: byte offset in the image, or OOB
    f32x4 rv[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int co = cb * CB + m * 16 + c;
      bv[m] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_b, (unsigned)co * 4u, 0, 0));
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int p = P0 + 16 * n + 4 * g;
        const bool mine = KS == 1 || (m * NT + n) % KS == q;    // (wave-uniform; another wave's tile: no traffic)
        off[m][n] = (mine && co < a.Cout && p < HW) ? ((unsigned)co * (unsigned)HW + (unsigned)p) * 4u : OOB;
        if constexpr (VEC) {
          rv[m][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_r, off[m][n], 0, 0));
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            rv[m][n][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                        rs_r, (off[m][n] != OOB && p + r < HW) ? off[m][n] + 4u * r : OOB, 0, 0));
        }
      }
    }
    if constexpr (KS > 1) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) red[(wave * NTILE + m * NT + n) * 64 + lane] = acc[m][n];
      __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const int t = m * NT + n;
        if (KS > 1 && t % KS != q) continue;                    // (wave-uniform)
        f32x4 s = acc[m][n];
        if constexpr (KS > 1) {
          s = red[((grp * KS + 0) * NTILE + t) * 64 + lane];
#pragma unroll
          for (int k = 1; k < KS; ++k) s += red[((grp * KS + k) * NTILE + t) * 64 + lane];
        }
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = s[r] + bv[m];
          if (a.res) x += rv[m][n][r];
          if (a.relu) x = cp_relu(x);
          o[r] = x;
        }
        if constexpr (VEC) {
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs_o, off[m][n], 0, 0);
        } else {
          const int p = P0 + 16 * n + 4 * g;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)o[r]), rs_o,
                                                  (off[m][n] != OOB && p + r < HW) ? off[m][n] + 4u * r : OOB, 0, 0);
        }
      }
  };
  if (a.vec) finish(std::true_type{});
  else finish(std::false_type{});
}

// The K split conv_mfma.hip's dispatch picks for a 1x1 / stride 1 launch (conv_dispatch, taps = 1): the sums of a wave
// group are what the bits depend on, the tile shape is not.
int staged_ks(int Cin, int Cout, int H, int W, int B) {
  const int nchunk = (Cin + KC - 1) / KC;
  const long long tiles_x = (W + 31) / 32;
  auto wgs = [&](int mt, int th) { return tiles_x * ((H + th - 1) / th) * B * ((Cout + 16 * mt - 1) / (16 * mt)); };
  if (Cout > 32 && wgs(4, 8) >= 448) return 1;
  if (wgs(2, 8) >= 320) return 1;
  if (wgs(2, 4) < 384 && nchunk >= 8) return 4;
  if (wgs(2, 4) < 768 && nchunk >= 4) return 2;
  return 1;
}

// Pixel groups of 32 per wave (never a function of the batch): two pay only where they still leave every SIMD of the
// chip two waves (2048); measured at the Root / project shapes of DLA-34.
int pick_nb(int Cout, long long HW) {
  const long long groups = (HW + 31) / 32, ncb = (Cout + CB - 1) / CB;
  return ((groups + 1) / 2) * ncb >= 2048 ? 2 : 1;
}

bool shape_ok(const int32_t* cs, int32_t nsrc, int32_t Cout, int32_t H, int32_t W) {
  if (!cs || nsrc < 1 || nsrc > MAXSRC || Cout < 1 || H < 1 || W < 1) return false;
  const long long HW = (long long)H * W, ncb = (Cout + CB - 1) / CB;
  long long Cin = 0;
  for (int i = 0; i < nsrc; ++i) {
    if (cs[i] < 16 || cs[i] % 16) return false;
    // 32-bit byte offsets within a source image, also for the channels a ragged last chunk reads past it
    if (cs[i] * HW * 4 >= (1ll << 31) || (cs[i] + 2 * KC) * HW * 4 >= (1ll << 32)) return false;
    Cin += cs[i];
  }
  if (ncb * CB * HW * 4 >= (1ll << 31)) return false;            // ... and within an output image (whole channel blocks)
  if (((HW + 31) / 32) * ncb >= (1ll << 31) || Cin >= (1 << 20)) return false;
  return true;
}

}  // namespace

int cp_conv1x1_stream_supported(const int32_t* cs, int32_t nsrc, int32_t Cout, int32_t H, int32_t W) {
  return shape_ok(cs, nsrc, Cout, H, W) ? 1 : 0;
}

size_t cp_conv1x1_stream_weight_bytes(int32_t Cin, int32_t Cout) {
  if (Cin < 16 || Cin % 16 || Cout < 1) return 0;
  return cp_conv_mfma_weight_bytes(Cin, Cout, 1);
}

int cp_conv1x1_stream_prepare(const float* weight, int32_t Cin, int32_t Cout, void* wperm, void* stream) {
  CP_CHECK_ARG(weight && wperm && Cin >= 1 && Cout >= 1);
  if (Cin % 16) return CP_EUNSUPPORTED;
  return cp_conv_mfma_prepare(weight, Cin, Cout, 1, 0, wperm, stream);
}

int cp_conv1x1_stream_form(int32_t Cin, int32_t Cout, int32_t H, int32_t W, int32_t B) {
  return pick_nb(Cout, (long long)H * W) << 8 | staged_ks(Cin, Cout, H, W, B);
}

// nb / ks: the tile form (pixel groups of 32 per wave 1 | 2, wave groups per tile 1 | 2 | 4), or 0 / 0 for the form of
// cp_conv1x1_stream_form -- the one that gives cp_conv_mfma_forward's bits; tests and probes force the others
int cp_conv1x1_stream_forward_form(const float* const* xs, const int32_t* cs, int32_t nsrc, const void* wperm,
                                   const float* bias, const float* residual, float* out, int32_t B, int32_t H, int32_t W,
                                   int32_t Cout, int32_t relu, int32_t nb, int32_t ks, void* stream) {
  CP_CHECK_ARG(xs && cs && wperm && out && B >= 1 && nsrc >= 1 && nsrc <= MAXSRC && H >= 1 && W >= 1 && Cout >= 1);
  for (int i = 0; i < nsrc; ++i) CP_CHECK_ARG(xs[i] && cs[i] >= 1);
  if (!shape_ok(cs, nsrc, Cout, H, W) || B > 65535) return CP_EUNSUPPORTED;
  StreamArgs a;
  int Cin = 0;
  bool half = false;
  for (int i = 0; i < MAXSRC; ++i) {
    a.xsrc[i] = i < nsrc ? xs[i] : nullptr;
    a.csrc[i] = i < nsrc ? cs[i] : 0;
    Cin += a.csrc[i];
    if (nsrc > 1 && i < nsrc && cs[i] % KC) half = true;
  }
  a.wp = (const bf16x8*)wperm;
  a.bias = bias;
  a.res = residual;
  a.out = out;
  a.Cin = Cin;
  a.Cout = Cout;
  a.HW = H * W;
  a.nchunk = (Cin + KC - 1) / KC;
  a.ncb = (Cout + CB - 1) / CB;
  a.relu = relu;
  a.vec = (a.HW & 3) == 0 && ((reinterpret_cast<unsigned long long>(out) | reinterpret_cast<unsigned long long>(residual)) & 15) == 0;
  if (nb == 0 && ks == 0) {
    nb = pick_nb(Cout, a.HW);
    ks = staged_ks(Cin, Cout, H, W, B);
  }
  if ((nb != 1 && nb != 2) || (ks != 1 && ks != 2 && ks != 4)) return CP_EINVAL;
  const auto launch = [&](auto kernel) {
    const unsigned npg = (unsigned)((a.HW + 32 * nb - 1) / (32 * nb));
    const unsigned pgw = 4 / ks;                               // tiles per workgroup
    hipLaunchKernelGGL(kernel, dim3(((npg + pgw - 1) / pgw) * a.ncb, B), dim3(256), 0, (hipStream_t)stream, a);
  };
  if (half) {                              // (two look-ups per chunk cost registers: one pixel group per wave, whatever nb says)
    nb = 1;
    if (ks == 1) launch(conv1x1_stream_kernel<2, 1, true>);
    else if (ks == 2) launch(conv1x1_stream_kernel<2, 2, true>);
    else launch(conv1x1_stream_kernel<2, 4, true>);
  } else if (nb == 2) {
    if (ks == 1) launch(conv1x1_stream_kernel<4, 1, false>);
    else if (ks == 2) launch(conv1x1_stream_kernel<4, 2, false>);
    else launch(conv1x1_stream_kernel<4, 4, false>);
  } else {
    if (ks == 1) launch(conv1x1_stream_kernel<2, 1, false>);
    else if (ks == 2) launch(conv1x1_stream_kernel<2, 2, false>);
    else launch(conv1x1_stream_kernel<2, 4, false>);
  }
  return cp_launch_status();
}

int cp_conv1x1_stream_forward(const float* const* xs, const int32_t* cs, int32_t nsrc, const void* wperm, const float* bias,
                              const float* residual, float* out, int32_t B, int32_t H, int32_t W, int32_t Cout,
                              int32_t relu, void* stream) {
  return cp_conv1x1_stream_forward_form(xs, cs, nsrc, wperm, bias, residual, out, B, H, W, Cout, relu, 0, 0, stream);
}
