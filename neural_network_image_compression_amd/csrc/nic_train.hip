// Training side path on the matrix cores (tf2_0/src/training.py:74-151):
// the convolutions of the Training step's forward and backward passes -- the codec's
// BaseEncoder / BaseDecoder (encoder.py:7-32, decoder.py:7-32) and the Entropynet's convs
// (training.py:25-42) -- as split-f16 ("f16x3") MFMA GEMMs over NHWC fp32 tensors.
//
// Every convolution of the step is one of two GEMM shapes:
//
//  * gather GEMM  y[m][co] = bias[co] + sum_{tap, ci} x[src(m, tap)][ci] * W(tap, ci, co)
//      m = output pixel (n, oy, ox).  Forward conv (Keras Conv2D, SAME): src = s*o + k - pad.
//      "Transposed" gather: src = (o + pad - k) / s where divisible -- the forward of
//      Conv2DTranspose (SAME) and the input gradient of Conv2D.  The input gradient of
//      Conv2DTranspose is a forward-conv gather.  W(tap, ci, co) reads the stored kernel
//      [tap][ci][co] (wt_layout 0) or [tap][co][ci] (wt_layout 1), so no transposed copy of a
//      kernel is ever made.
//  * weight-gradient GEMM  dW[tap][a][b] = sum_u gat[s*u + k - pad][a] * dir[u][b]
//      (Conv2D: gat = x, dir = dy; Conv2DTranspose: gat = dy, dir = x), K = every pixel of
//      the batch, split into slices whose partial sums a second kernel adds in a fixed order
//      (deterministic, no atomics).
//
// Arithmetic: each operand tile is scaled by an exact power of two (per tensor, from
// nic_absmax_scale: max |x| * scale in [2^13, 2^14), so gradients of 1e-9 keep every bit)
// and split hi = f16(x), lo = f16(x - hi) while it is staged into LDS; three
// v_mfma_f32_16x16x32_f16 per fragment pair (hi*hi + hi*lo + lo*hi) accumulate in fp32;
// the epilogue multiplies by the exact inverse scales.  Error ~2^-22 relative per product,
// fp32-class (tests/test_gpu_train.py: vs torch fp32 autograd).
//
// Tiles: 256-thread blocks, K in chunks of 32 staged through LDS (row pitch 40 f16 = 80 B:
// the 16-B fragment reads of a 16-lane group hit distinct banks); the next chunk's global
// loads are issued before the current chunk's MFMAs (register double buffer).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "nic_kernels.h"

namespace nic {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int TK = 32;  // K per chunk
constexpr int LP = 40;  // LDS row pitch (f16)
constexpr int GM = 64;  // gather GEMM: output pixels per block (4 waves x 16)

__device__ __forceinline__ void split1(float v, _Float16& hi, _Float16& lo) {
  hi = (_Float16)v;
  lo = (_Float16)(v - (float)hi);
}

__device__ __forceinline__ float ld_scale(const float* s) { return s ? *s : 1.0f; }

// ---- gather GEMM -------------------------------------------------------------------------
struct GatherArgs {
  const float* x;      // [n][h][w][cin]
  const f16x8* wp;     // packed split weights (pack_w_kernel): [K/32 chunk][NT/16 co tile][hi, lo][64 lanes]
  const float* bias;   // [cout] or null
  const float* sx;     // device scale of x (power of two) or null
  const float* sw;     // device scale of the weights or null (already applied in wp)
  float* y;            // [n][oh][ow][cout]
  int n, h, w, cin, oh, ow, cout, kh, kw, stride, pad_y, pad_x, transposed;
  int act;             // 1: leaky_relu(0.2) of the biased sum (Keras activation=tf.nn.leaky_relu)
  int K;               // kh * kw * cin
  long long M;         // n * oh * ow
  int ph_blk[5];       // phase mode: first block of output phase (py, px) = (p >> 1, p & 1), then the grid
};

// Output pixel m of the block's set -> (b, oy, ox).  Phase mode: the pixels of one output
// phase (oy % 2, ox % 2) = (py, px) only, so every pixel of the block uses the same taps.
__device__ __forceinline__ bool pixel_of(const GatherArgs& a, bool ph, int py, int px, long long m, int& b, int& oy,
                                         int& ox) {
  if (!ph) {
    if (m >= a.M) return false;
    const long long per = (long long)a.oh * a.ow;
    b = (int)(m / per);
    const int r = (int)(m - (long long)b * per);
    oy = r / a.ow;
    ox = r - oy * a.ow;
    return true;
  }
  const int qh = (a.oh - py + 1) >> 1, qw = (a.ow - px + 1) >> 1;
  const long long per = (long long)qh * qw;
  if (per == 0 || m >= (long long)a.n * per) return false;
  b = (int)(m / per);
  const int r = (int)(m - (long long)b * per), qy = r / qw;
  oy = 2 * qy + py;
  ox = 2 * (r - qy * qw) + px;
  return true;
}

// source pixel of output pixel (b, oy, ox) at tap (ky, kx); -1 when outside / not on the grid
__device__ __forceinline__ long long gather_src(const GatherArgs& a, int b, int oy, int ox, int ky, int kx) {
  int iy, ix;
  if (a.transposed) {
    const int ty = oy + a.pad_y - ky, tx = ox + a.pad_x - kx;
    if (ty < 0 || tx < 0) return -1;
    if (a.stride == 1) {  // (uniform branches: no integer division for the strides in use)
      iy = ty;
      ix = tx;
    } else if (a.stride == 2) {
      if ((ty | tx) & 1) return -1;
      iy = ty >> 1;
      ix = tx >> 1;
    } else {
      if (ty % a.stride || tx % a.stride) return -1;
      iy = ty / a.stride;
      ix = tx / a.stride;
    }
  } else {
    iy = a.stride * oy + ky - a.pad_y;
    ix = a.stride * ox + kx - a.pad_x;
  }
  if ((unsigned)iy >= (unsigned)a.h || (unsigned)ix >= (unsigned)a.w) return -1;
  return ((long long)b * a.h + iy) * a.w + ix;
}

// Weights -> split-f16 MFMA A fragments, once per call: fragment (chunk c, co tile t, hi|lo,
// lane) holds rows co = 16 t + (lane & 15), k = 32 c + 8 (lane >> 4) + j of w * scale, where
// k = tap * cin + ci and W(tap, ci, co) reads layout 0 [tap][ci][co] or 1 [tap][co][ci].
__global__ __launch_bounds__(256) void pack_w_kernel(const float* __restrict__ wt, int layout, int cin, int cout, int K,
                                                     int ntt, int nchunk, const float* __restrict__ sw,
                                                     f16x8* __restrict__ wp) {
  const int total = nchunk * ntt * 64;
  const float s = ld_scale(sw);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int lane = i & 63, ct = i >> 6, t = ct % ntt, c = ct / ntt;
    const int co = 16 * t + (lane & 15);
    f16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 32 * c + 8 * (lane >> 4) + j;
      float v = 0.f;
      if (co < cout && k < K) {
        const int tap = k / cin, ci = k - tap * cin;
        v = layout ? wt[((size_t)tap * cout + co) * cin + ci] : wt[((size_t)tap * cin + ci) * cout + co];
      }
      _Float16 h, l;
      split1(v * s, h, l);
      hi[j] = h;
      lo[j] = l;
    }
    wp[(size_t)(ct * 2 + 0) * 64 + lane] = hi;
    wp[(size_t)(ct * 2 + 1) * 64 + lane] = lo;
  }
}

// NT = output channels per block (16, 32 or 64); VEC: cin % 32 == 0 (a K chunk is 32
// consecutive channels of one tap: two float4 per thread, stored as f16x4 hi / lo), else one
// element per (pixel, k); PH (VEC, transposed, stride 2): the block's pixels share one output
// phase and the K loop visits only that phase's taps (a quarter of them).  The weights'
// A fragments come straight from the packed buffer (one chunk ahead in registers); only the
// gathered activations go through LDS.
template <int NT, bool VEC, bool PH>
__global__ __launch_bounds__(256) void conv_gather_kernel(GatherArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 xs[2][GM * LP];  // [hi, lo][pixel][k]
  constexpr int NTT = NT / 16;
  constexpr int XN = VEC ? 2 : 8;  // x elements (float4s when VEC) per thread per chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l16 = lane & 15;
  int phase = 0, blk = blockIdx.x;
  if constexpr (PH) {
    while (phase < 3 && blk >= a.ph_blk[phase + 1]) ++phase;
    blk -= a.ph_blk[phase];
  }
  const int py = phase >> 1, px = phase & 1;
  const long long m0 = (long long)blk * GM;
  const float sx = ld_scale(a.sx), sw = ld_scale(a.sw);
  // K chunks: all of them, or (PH) the phase's taps ky = ky0 + 2 i, kx = kx0 + 2 j
  const int cc_n = VEC ? a.cin / TK : 1;
  const int ky0 = (py + a.pad_y) & 1, kx0 = (px + a.pad_x) & 1;
  const int tny = (a.kh - ky0 + 1) >> 1, tnx = (a.kw - kx0 + 1) >> 1;
  const int nchunk = PH ? tny * tnx * cc_n : (a.K + TK - 1) / TK;
  auto chunk_tap = [&](int c, int& ky, int& kx, int& ci0, int& gc) {  // VEC: tap and channel block of chunk c
    if constexpr (PH) {
      const int tt = c / cc_n, cc = c - tt * cc_n, iy = tt / tnx;
      ky = ky0 + 2 * iy;
      kx = kx0 + 2 * (tt - iy * tnx);
      ci0 = cc * TK;
      gc = (ky * a.kw + kx) * cc_n + cc;
    } else {
      const int k0 = c * TK, tap = k0 / a.cin;
      ky = tap / a.kw;
      kx = tap - ky * a.kw;
      ci0 = k0 - tap * a.cin;
      gc = c;
    }
  };

  // this thread's staging pixels: VEC px = tid/8 + 32 r; scalar px = tid/32 + 8 e
  int pb[XN], pyy[XN], pxx[XN];
#pragma unroll
  for (int e = 0; e < XN; ++e) {
    const int sp = VEC ? (tid >> 3) + 32 * e : (tid >> 5) + 8 * e;
    if (!pixel_of(a, PH, py, px, m0 + sp, pb[e], pyy[e], pxx[e])) pb[e] = -1;
  }

  f32x4 xv[VEC ? XN : 1];
  float xsv[VEC ? 1 : XN];
  f16x8 wc[NTT][2], wn[NTT][2];  // A fragments of the current / next chunk (static indices: no scratch)
  auto load = [&](int c, f16x8 (&w)[NTT][2]) {
    int ky, kx, ci0, gc;
    if constexpr (VEC) {
      chunk_tap(c, ky, kx, ci0, gc);
#pragma unroll
      for (int e = 0; e < XN; ++e) {
        const long long s = pb[e] >= 0 ? gather_src(a, pb[e], pyy[e], pxx[e], ky, kx) : -1;
        xv[e] = s >= 0 ? *(const f32x4*)(a.x + s * a.cin + ci0 + 4 * (tid & 7)) : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    } else {
      gc = c;
      const int k = c * TK + (tid & 31);
      const int tap = k / a.cin, ci = k - tap * a.cin;
      ky = tap / a.kw;
      kx = tap - ky * a.kw;
#pragma unroll
      for (int e = 0; e < XN; ++e) {
        const long long s = (pb[e] >= 0 && k < a.K) ? gather_src(a, pb[e], pyy[e], pxx[e], ky, kx) : -1;
        xsv[e] = s >= 0 ? a.x[s * a.cin + ci] : 0.f;
      }
    }
#pragma unroll
    for (int t = 0; t < NTT; ++t)
#pragma unroll
      for (int hl = 0; hl < 2; ++hl) w[t][hl] = a.wp[((size_t)(gc * NTT + t) * 2 + hl) * 64 + lane];
  };
  auto stage = [&]() {
    if constexpr (VEC) {
      typedef _Float16 f16x4v __attribute__((ext_vector_type(4)));
#pragma unroll
      for (int e = 0; e < XN; ++e) {
        const int sp = (tid >> 3) + 32 * e, k = 4 * (tid & 7);
        f16x4v hi, lo;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          _Float16 h, l;
          split1(xv[e][r] * sx, h, l);
          hi[r] = h;
          lo[r] = l;
        }
        *(f16x4v*)&xs[0][sp * LP + k] = hi;
        *(f16x4v*)&xs[1][sp * LP + k] = lo;
      }
    } else {
#pragma unroll
      for (int e = 0; e < XN; ++e) {
        const int sp = (tid >> 5) + 8 * e, k = tid & 31;
        split1(xsv[e] * sx, xs[0][sp * LP + k], xs[1][sp * LP + k]);
      }
    }
  };

  f32x4 acc[NTT];
#pragma unroll
  for (int t = 0; t < NTT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (nchunk > 0) load(0, wc);
  for (int c = 0; c < nchunk; ++c) {
    __syncthreads();  // every wave is done with the previous chunk's tile
    stage();
    __syncthreads();
    if (c + 1 < nchunk) load(c + 1, wn);  // in flight during this chunk's MFMAs
    const int bo = (wave * 16 + l16) * LP + 8 * g;
    const f16x8 bh = *(const f16x8*)&xs[0][bo], bl = *(const f16x8*)&xs[1][bo];
#pragma unroll
    for (int t = 0; t < NTT; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wc[t][1], bh, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wc[t][0], bl, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wc[t][0], bh, acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < NTT; ++t) {
      wc[t][0] = wn[t][0];
      wc[t][1] = wn[t][1];
    }
  }
  // D[co = 16t + 4g + r][pixel 16 wave + l16]
  int b, oy, ox;
  if (!pixel_of(a, PH, py, px, m0 + wave * 16 + l16, b, oy, ox)) return;
  const float isx = 1.0f / sx, isw = 1.0f / sw;  // exact: powers of two (applied one at a time)
  float* yp = a.y + (((long long)b * a.oh + oy) * a.ow + ox) * a.cout;
#pragma unroll
  for (int t = 0; t < NTT; ++t) {
    const int co = t * 16 + 4 * g;
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = (acc[t][r] * isx) * isw + (a.bias && co + r < a.cout ? a.bias[co + r] : 0.f);
    if (a.act)  // tf.nn.leaky_relu(z, 0.2) = max(0.2 z, z): z for z > 0, else 0.2 z (one rounding)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = fmaxf(__fmul_rn(v[r], 0.2f), v[r]);
    if ((a.cout & 3) == 0 && co + 4 <= a.cout) {
      *(f32x4*)(yp + co) = v;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (co + r < a.cout) yp[co + r] = v[r];
    }
  }
}

// ---- activation + bias gradient of a layer ------------------------------------------------
// dz = dy * (act && !(y > 0) ? 0.2 : 1): tf.nn.leaky_relu's gradient (z > 0 ? dy : 0.2 dy),
// read from the layer's output y (y > 0 iff z > 0); db[c] = sum over rows of dz[row][c]
// (BiasAddGrad); and the power-of-two operand scale of dz (nic_absmax_scale's, from the same
// pass).  A block takes kAbgRows rows; thread t owns V consecutive columns (V = 4: 16-B loads
// when cols % 4 == 0) of row lane t / (cols / V), summed per thread in row order, then over
// the row lanes in order into part[block][c] (max |dz| into part[nblk * cols + block]);
// abg_reduce_kernel adds the blocks' partials of a column in a fixed order (deterministic).
constexpr int kAbgRows = 256;
template <int V>
__global__ __launch_bounds__(256) void act_bias_grad_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                            long long rows, int cols, int act, float* __restrict__ dz,
                                                            float* __restrict__ part) {
  typedef float fv __attribute__((ext_vector_type(V)));
  __shared__ float red[256 * V];
  __shared__ float wm[4];
  const int cg = cols / V, nrl = 256 / cg, t = threadIdx.x, c0 = (t % cg) * V, rl = t / cg;
  const long long r0 = (long long)blockIdx.x * kAbgRows;
  const long long r1 = r0 + kAbgRows < rows ? r0 + kAbgRows : rows;
  fv s = {};
  float m = 0.f;
  if (rl < nrl) {
#pragma unroll 4
    for (long long r = r0 + rl; r < r1; r += nrl) {
      const long long e = r * cols + c0;
      fv g = *(const fv*)(dy + e);
      if (act) {
        const fv yv = *(const fv*)(y + e);
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (!(yv[k] > 0.f)) g[k] = __fmul_rn(g[k], 0.2f);
      }
      if (dz) *(fv*)(dz + e) = g;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        s[k] = __fadd_rn(s[k], g[k]);
        m = fmaxf(m, fabsf(g[k]));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) red[t * V + k] = s[k];
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((t & 63) == 0) wm[t >> 6] = m;
  __syncthreads();
  if (t < cols) {  // column t: lane group t / V of every row lane, in row-lane order
    float b = 0.f;
    for (int k = 0; k < nrl; ++k) b = __fadd_rn(b, red[(k * cg + t / V) * V + t % V]);
    part[(long long)blockIdx.x * cols + t] = b;
  }
  if (t == 0) part[(long long)gridDim.x * cols + blockIdx.x] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
}

// Block c < cols: db[c] = sum of the blocks' partials of column c (thread k adds partials k,
// k + 256, ... in order, then a fixed pairwise tree over the threads); block cols: the scale
// of the blocks' max |dz| (nic_absmax_scale's formula)
__global__ __launch_bounds__(256) void abg_reduce_kernel(const float* __restrict__ part, int nblk, int cols,
                                                         float* __restrict__ db, float* __restrict__ scale) {
  __shared__ float red[256];
  const int c = blockIdx.x, t = threadIdx.x;
  if (c < cols) {
    if (!db) return;
    float s = 0.f;
    for (int k = t; k < nblk; k += 256) s = __fadd_rn(s, part[(long long)k * cols + c]);
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) red[t] = __fadd_rn(red[t], red[t + o]);
      __syncthreads();
    }
    if (t == 0) db[c] = red[0];
  } else {
    if (!scale) return;
    float m = 0.f;
    for (int k = t; k < nblk; k += 256) m = fmaxf(m, part[(long long)nblk * cols + k]);
    red[t] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) red[t] = fmaxf(red[t], red[t + o]);
      __syncthreads();
    }
    if (t == 0) {
      m = red[0];
      float sc = 1.0f;
      if (m > 0.f && isfinite(m)) sc = ldexpf(1.0f, min(max(13 - ilogbf(m), -126), 126));
      *scale = sc;
    }
  }
}

// ---- SSIM terms of both losses from the filtered maps (tf.image.ssim, training.py:119-121) ---
// Per pixel of the VALID map, from mx = G*x, my = G*y, sxy = G*(x y), sxx = G*(x^2 + y^2):
//   num0 = (mx my) 2, den0 = mx mx + my my, lum = (num0 + c1) / (den0 + c1),
//   cs = ((2 sxy - num0) + c2) / ((sxx - den0) + c2), v = lum cs
// in tf.image.ssim's op order, every op rounded.  The SSIM loss is the plane mean of v, the
// MS-SSIM loss reads the plane mean of cs as well: one kernel pair (below) gives both.
constexpr int kSsimPix = 1024;  // map pixels per block
struct SsimTerms {
  float num0, den0, lum, cs, a, b, c, d;
};
__device__ __forceinline__ SsimTerms ssim_terms(float mx, float my, float sxy, float sxx, float c1, float c2) {
  SsimTerms t;
  t.num0 = __fmul_rn(__fmul_rn(mx, my), 2.0f);
  t.den0 = __fadd_rn(__fmul_rn(mx, mx), __fmul_rn(my, my));
  t.a = __fadd_rn(t.num0, c1);
  t.b = __fadd_rn(t.den0, c1);
  t.lum = __fdiv_rn(t.a, t.b);
  t.c = __fadd_rn(__fsub_rn(__fmul_rn(sxy, 2.0f), t.num0), c2);
  t.d = __fadd_rn(__fsub_rn(sxx, t.den0), c2);
  t.cs = __fdiv_rn(t.c, t.d);
  return t;
}

// ---- One scale's two means (the SSIM loss: its only scale), and the step between scales ------
// tf.image.ssim_multiscale keeps, per scale, the plane means of cs (scales 0 .. K-2) and of
// lum cs (scale K-1); tf.image.ssim is the latter alone.  msssim_terms_kernel gives both from
// ssim_terms in one pass: block bk of plane n sums its kSsimPix pixels, thread t its
// pixels 4t .. 4t+3 in that order (one 16-byte load per map when VEC: hw % 4 == 0 and the maps
// 16-byte aligned; the scalar form adds in the same order), then the tree over the 256 threads;
// part[2 blk] / part[2 blk + 1] hold the lum cs / cs partials, msssim_mean_kernel adds them in
// block order.
__device__ __forceinline__ void ld4(float* dst, const float* src) {  // src 16-byte aligned
  const float4 v = *reinterpret_cast<const float4*>(src);
  dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
}
__device__ __forceinline__ void st4(float* dst, const float* src) {  // dst 16-byte aligned
  *reinterpret_cast<float4*>(dst) = make_float4(src[0], src[1], src[2], src[3]);
}
template <bool VEC>
__global__ __launch_bounds__(256) void msssim_terms_kernel(const float* __restrict__ mx, const float* __restrict__ my,
                                                           const float* __restrict__ sxy, const float* __restrict__ sxx,
                                                           long long hw, int bpi, float c1, float c2,
                                                           float* __restrict__ part) {
  __shared__ float red[2][256];
  const int n = blockIdx.x / bpi, bk = blockIdx.x - n * bpi, t = threadIdx.x;
  const long long p = (long long)bk * kSsimPix + 4 * t, e = (long long)n * hw + p;
  float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4], c[4], d[4];
  int cnt = 0;
  if constexpr (VEC) {
    if (p < hw) {  // hw % 4 == 0: the four pixels are all inside the plane
      ld4(a, mx + e);
      ld4(b, my + e);
      ld4(c, sxy + e);
      ld4(d, sxx + e);
      cnt = 4;
    }
  } else {
    for (int k = 0; k < 4 && p + k < hw; ++k, ++cnt) {
      a[k] = mx[e + k];
      b[k] = my[e + k];
      c[k] = sxy[e + k];
      d[k] = sxx[e + k];
    }
  }
  float s = 0.f, sc = 0.f;
  for (int k = 0; k < cnt; ++k) {
    const SsimTerms q = ssim_terms(a[k], b[k], c[k], d[k], c1, c2);
    s = __fadd_rn(s, __fmul_rn(q.lum, q.cs));
    sc = __fadd_rn(sc, q.cs);
  }
  red[0][t] = s;
  red[1][t] = sc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      red[0][t] = __fadd_rn(red[0][t], red[0][t + o]);
      red[1][t] = __fadd_rn(red[1][t], red[1][t + o]);
    }
    __syncthreads();
  }
  if (t == 0) {
    part[2 * (long long)blockIdx.x] = red[0][0];
    part[2 * (long long)blockIdx.x + 1] = red[1][0];
  }
}
__global__ __launch_bounds__(64) void msssim_mean_kernel(const float* __restrict__ part, int n, int bpi, long long hw,
                                                         float* __restrict__ lcs_mean, float* __restrict__ cs_mean) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f, sc = 0.f;
  for (int k = 0; k < bpi; ++k) {
    s = __fadd_rn(s, part[2 * ((long long)i * bpi + k)]);
    sc = __fadd_rn(sc, part[2 * ((long long)i * bpi + k) + 1]);
  }
  lcs_mean[i] = __fdiv_rn(s, (float)hw);
  cs_mean[i] = __fdiv_rn(sc, (float)hw);
}
// The four terms' gradients of sum_n g_ssim[n] mean(lum cs) + g_cs[n] mean(cs).  On the first
// path (G1 = g_ssim / hw = d mean / d v), v = (a / b) (c / d):
//   dv/dnum0 = cs / b - lum / d, dv/dden0 = lum cs / d - lum cs / b, dv/d(2 sxy) = lum / d,
//   dv/dsxx = -lum cs / d;
// on the second (G2 = g_cs / hw), cs = c / d:
//   dcs/dnum0 = -1/d, dcs/dden0 = cs/d, dcs/d(2 sxy) = 1/d, dcs/dsxx = -cs/d.
// With g_cs = 0 (the SSIM loss) every G2 product is 0 and the sums return the first path's value.
struct SsimTermGrads {
  float gmx, gmy, gsxy, gsxx;
};
__device__ __forceinline__ SsimTermGrads msssim_term_grads(float x, float y, float sxy, float sxx, float c1, float c2,
                                                           float G1, float G2) {
  const SsimTerms q = ssim_terms(x, y, sxy, sxx, c1, c2);
  const float ib = __frcp_rn(q.b), id = __frcp_rn(q.d), v = __fmul_rn(q.lum, q.cs);
  const float csd = __fmul_rn(q.cs, id);
  const float dnum0 = __fsub_rn(__fmul_rn(G1, __fsub_rn(__fmul_rn(q.cs, ib), __fmul_rn(q.lum, id))), __fmul_rn(G2, id));
  const float dden0 = __fadd_rn(__fmul_rn(G1, __fsub_rn(__fmul_rn(v, id), __fmul_rn(v, ib))), __fmul_rn(G2, csd));
  SsimTermGrads r;
  r.gmx = __fmul_rn(2.0f, __fadd_rn(__fmul_rn(dnum0, y), __fmul_rn(dden0, x)));
  r.gmy = __fmul_rn(2.0f, __fadd_rn(__fmul_rn(dnum0, x), __fmul_rn(dden0, y)));
  r.gsxy = __fmul_rn(2.0f, __fadd_rn(__fmul_rn(G1, __fmul_rn(q.lum, id)), __fmul_rn(G2, id)));
  r.gsxx = -__fadd_rn(__fmul_rn(G1, __fmul_rn(v, id)), __fmul_rn(G2, csd));
  return r;
}
template <bool VEC>
__global__ __launch_bounds__(256) void msssim_terms_grad_kernel(
    const float* __restrict__ mx, const float* __restrict__ my, const float* __restrict__ sxy,
    const float* __restrict__ sxx, const float* __restrict__ g_ssim, const float* __restrict__ g_cs, int n, long long hw,
    float c1, float c2, float* __restrict__ gmx, float* __restrict__ gmy, float* __restrict__ gsxy,
    float* __restrict__ gsxx) {
  constexpr int V = VEC ? 4 : 1;  // VEC: hw % 4 == 0, so the four elements share their plane
  const long long total = (long long)n * hw / V;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long e = i * V, pl = e / hw;
    const float G1 = __fdiv_rn(g_ssim[pl], (float)hw), G2 = __fdiv_rn(g_cs[pl], (float)hw);
    float a[V], b[V], c[V], d[V], o0[V], o1[V], o2[V], o3[V];
    if constexpr (VEC) {
      ld4(a, mx + e);
      ld4(b, my + e);
      ld4(c, sxy + e);
      ld4(d, sxx + e);
    } else {
      a[0] = mx[e], b[0] = my[e], c[0] = sxy[e], d[0] = sxx[e];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const SsimTermGrads r = msssim_term_grads(a[k], b[k], c[k], d[k], c1, c2, G1, G2);
      o0[k] = r.gmx, o1[k] = r.gmy, o2[k] = r.gsxy, o3[k] = r.gsxx;
    }
    if constexpr (VEC) {
      st4(gmx + e, o0);
      st4(gmy + e, o1);
      st4(gsxy + e, o2);
      st4(gsxx + e, o3);
    } else {
      gmx[e] = o0[0], gmy[e] = o1[0], gsxy[e] = o2[0], gsxx[e] = o3[0];
    }
  }
}

// ---- The rate losses: the code length of a latent under per-channel tables -------------------
// One kernel set, a template on NX, the number of contexts per row.  L is (groups * C, NX, 256):
// L[r][x][j] = -log2 p_r(j | x).  Plane m of y (m, h, w, C) belongs to group m / (m_total / groups)
// and its channel c reads row r = group * C + c.  Per element, every op one fp32 rounding:
//   v = fminf(fmaxf(255 y, 0), 255) (a NaN becomes 0), k = min((int)floorf(v), 254), t = v - k,
//   bits = L[r][x][k] + t (L[r][x][k+1] - L[r][x][k])
// so k + 1 <= 255 whatever y holds.  NX = 1 is the table rate: x = 0, and `if constexpr` leaves no
// read of yc, anchors or seg in that instantiation.  NX = 3 is the context rate: anchors holds
// groups * C bytes, and element (m, q, c), q the row-major pixel inside plane m, reads context
//   x = 0 if q % seg == 0, else min(2, |(int)rintf(fminf(fmaxf(255 yc[m][q-1][c], 0), 255)) - anchors[r]|)
// q % seg != 0 implies q >= 1, so the left read stays inside plane m.  Both instantiations share
// every order below, so NX equal rows give the table rate's bits and dy bit for bit.
// rate_kernel: block bk of plane m sums its kRatePix elements, thread t its elements t, t + 256,
// t + 512, t + 768 in that order, then the tree over the 256 threads; rate_table_sum_kernel adds a
// plane's partials in block order.
constexpr int kRatePix = 1024;  // elements per block of rate_kernel
struct RateElem {
  int k;
  float t;
};
__device__ __forceinline__ RateElem rate_elem(float y) {
  const float v = fminf(fmaxf(__fmul_rn(255.0f, y), 0.0f), 255.0f);
  RateElem e;
  e.k = min((int)floorf(v), 254);
  e.t = __fsub_rn(v, (float)e.k);
  return e;
}
__device__ __forceinline__ int rate_ctx(const float* __restrict__ yc, long long elem, int C, int q, int seg, int anchor) {
  if (q % seg == 0) return 0;
  const float v = fminf(fmaxf(__fmul_rn(255.0f, yc[elem - C]), 0.0f), 255.0f);
  return min(2, abs((int)rintf(v) - anchor));
}
// the table of row r for element `elem` (pixel q of its plane): &L[r][x][0]
template <int NX>
__device__ __forceinline__ const float* rate_row(const float* __restrict__ L, const float* __restrict__ yc,
                                                 const unsigned char* __restrict__ anchors, int r, long long elem,
                                                 int C, int q, int seg) {
  if constexpr (NX == 1)
    return L + (long long)r * 256;
  else
    return L + ((long long)r * NX + rate_ctx(yc, elem, C, q, seg, anchors[r])) * 256;
}
template <int NX>
__global__ __launch_bounds__(256) void rate_kernel(const float* __restrict__ y, const float* __restrict__ yc,
                                                   const float* __restrict__ L,
                                                   const unsigned char* __restrict__ anchors, int elems, int C,
                                                   int ppg, int bpp, int seg, float* __restrict__ part) {
  __shared__ float red[256];
  const int m = blockIdx.x / bpp, bk = blockIdx.x - m * bpp, t = threadIdx.x;
  const int r0 = (m / ppg) * C;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kRatePix / 256; ++i) {
    const int e = bk * kRatePix + i * 256 + t;
    if (e < elems) {
      const long long idx = (long long)m * elems + e;
      const int q = e / C;
      const float* row = rate_row<NX>(L, yc, anchors, r0 + (e - q * C), idx, C, q, seg);
      const RateElem el = rate_elem(y[idx]);
      const float l0 = row[el.k];
      s = __fadd_rn(s, __fadd_rn(l0, __fmul_rn(el.t, __fsub_rn(row[el.k + 1], l0))));
    }
  }
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] = __fadd_rn(red[t], red[t + o]);
    __syncthreads();
  }
  if (t == 0) part[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(64) void rate_table_sum_kernel(const float* __restrict__ part, int m, int bpp,
                                                            float* __restrict__ plane_bits) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= m) return;
  float s = 0.f;
  for (int k = 0; k < bpp; ++k) s = __fadd_rn(s, part[(long long)i * bpp + k]);
  plane_bits[i] = s;
}
// Backward for an upstream g[m] per plane.  dy = (255 g[m]) (L[r][x][k+1] - L[r][x][k]), one thread
// per element, written once.
template <int NX>
__global__ __launch_bounds__(256) void rate_dy_kernel(const float* __restrict__ y, const float* __restrict__ yc,
                                                      const float* __restrict__ L,
                                                      const unsigned char* __restrict__ anchors,
                                                      const float* __restrict__ g, long long total, int elems, int C,
                                                      int ppg, int seg, float* __restrict__ dy) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int m = (int)(i / elems), e = (int)(i - (long long)m * elems), q = e / C;
    const float* row = rate_row<NX>(L, yc, anchors, (m / ppg) * C + (e - q * C), i, C, q, seg);
    const RateElem el = rate_elem(y[i]);
    dy[i] = __fmul_rn(__fmul_rn(255.0f, g[m]), __fsub_rn(row[el.k + 1], row[el.k]));
  }
}
// dL[r][x][j] = sum over the elements of row r in context x of g (1 - t) at j = k and of g t at
// j = k + 1, with no atomics: owner-computes in LDS.  Block (group, slab, x) is one wave and takes
// kRateSlab consecutive pixels of one group (a group's planes are consecutive, so its pixels are
// one contiguous range).  Its 64 KB of LDS hold R = 64 / C replicas of the group's C x 256 partial
// table, laid out [replica][j][c] (channel fastest: the C threads of a replica fall on C different
// banks).  Thread (replica, c) owns column c of its replica alone: it takes the slab's pixels
// replica, replica + R, ... in that order and, where the pixel's context is x, adds its two terms
// with plain LDS read-modify-write, so every word has one writer and one order.  A slab that begins
// mid-segment reads its left pixel from the slab before it in global memory (never from before its
// plane: see above).  The replicas are then added in replica order into the block's partial in
// `part` ([(group, slab, x)][j][c]); rate_dl_reduce_kernel adds the slabs of a (group, x) in a
// fixed order (fours of fours of fours in block order, then those sums in order).  With every pixel
// in context 0 (seg = 1) the x = 0 blocks do exactly the NX = 1 kernel's work.
constexpr int kRateSlab = 128;         // pixels per block of rate_dl_kernel
constexpr int kRateLdsFloats = 16384;  // 64 KB: floor(64 / C) replicas of C x 256 floats
template <int NX>
__global__ __launch_bounds__(64) void rate_dl_kernel(const float* __restrict__ y, const float* __restrict__ yc,
                                                     const unsigned char* __restrict__ anchors,
                                                     const float* __restrict__ g, int C, int hw, long long P, int spg,
                                                     int seg, float* __restrict__ part) {
  __shared__ float tab[kRateLdsFloats];
  const int R = 64 / C, T = C * 256, t = threadIdx.x, rep = t / C, c = t - rep * C;
  const int x = blockIdx.x % NX, gs = blockIdx.x / NX, grp = gs / spg, slab = gs - grp * spg;
  for (int i = t; i < R * T; i += 64) tab[i] = 0.f;
  __syncthreads();
  if (rep < R) {
    float* mine = tab + rep * T + c;
    int anchor = 0;
    if constexpr (NX > 1) anchor = anchors[grp * C + c];
    const long long p0 = (long long)slab * kRateSlab, p1 = p0 + kRateSlab < P ? p0 + kRateSlab : P;
    for (long long p = p0 + rep; p < p1; p += R) {
      const long long px = (long long)grp * P + p, plane = px / hw;
      const long long idx = px * C + c;
      if constexpr (NX > 1)
        if (rate_ctx(yc, idx, C, (int)(px - plane * hw), seg, anchor) != x) continue;
      const float gm = g[plane];
      const RateElem q = rate_elem(y[idx]);
      float* lo = mine + q.k * C;
      lo[0] = __fadd_rn(lo[0], __fmul_rn(gm, __fsub_rn(1.0f, q.t)));
      lo[C] = __fadd_rn(lo[C], __fmul_rn(gm, q.t));
    }
  }
  __syncthreads();
  for (int i = t; i < T; i += 64) {
    float s = tab[i];
    for (int r = 1; r < R; ++r) s = __fadd_rn(s, tab[r * T + i]);
    part[(long long)blockIdx.x * T + i] = s;
  }
}
template <int NX>
__global__ __launch_bounds__(256) void rate_dl_reduce_kernel(const float* __restrict__ part, int groups, int C, int spg,
                                                             float* __restrict__ dL) {
  const int T = C * 256, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= groups * NX * T) return;
  const int gx = i / T, rem = i - gx * T, grp = gx / NX, x = gx - grp * NX, j = rem / C, c = rem - j * C;
  const float* src = part + ((long long)grp * spg * NX + x) * T + rem;  // slab b at src[b * NX T]
  const long long step = (long long)NX * T;
  float total = 0.f;
  for (int b0 = 0; b0 < spg; b0 += 64) {
    float s3 = 0.f;
    for (int b1 = b0; b1 < b0 + 64 && b1 < spg; b1 += 16) {
      float s2 = 0.f;
      for (int b2 = b1; b2 < b1 + 16 && b2 < spg; b2 += 4) {
        float s1 = 0.f;
        for (int b = b2; b < b2 + 4 && b < spg; ++b) s1 = __fadd_rn(s1, src[b * step]);
        s2 = __fadd_rn(s2, s1);
      }
      s3 = __fadd_rn(s3, s2);
    }
    total = __fadd_rn(total, s3);
  }
  dL[(((long long)grp * C + c) * NX + x) * 256 + j] = total;
}

// The step between scales (tf.image.ssim_multiscale: an odd height or width SYMMETRIC-padded by
// one on the far side, i.e. its last row / column repeated, then a 2x2 average pool, stride 2) and
// the two product planes the Gaussian reads next.  One thread per four output columns of one output
// row (VEC: w % 8 == 0 and everything 16-byte aligned, so two float4 loads per input row and one
// float4 store per output; otherwise the same work with scalar accesses):
//   x' = 0.25 ((x[2i][2j] + x[2i][2j+1]) + (x[2i+1][2j] + x[2i+1][2j+1])),  P = x' y',  Q = x' x' + y' y'
struct PoolPrepArgs {
  const float *x, *y;          // (n, h, w)
  float *xp, *yp, *pxy, *pss;  // (n, oh, ow); null: not written
  int n, h, w, oh, ow;
  int pool;                    // 0: x' = x (oh = h, ow = w)
};
__device__ __forceinline__ float pool4(float a, float b, float c, float d) {
  return __fmul_rn(0.25f, __fadd_rn(__fadd_rn(a, b), __fadd_rn(c, d)));
}
template <bool VEC>
__global__ __launch_bounds__(256) void pool2_prep_kernel(PoolPrepArgs a) {
  const int gw = (a.ow + 3) / 4;  // groups of four output columns per row
  const long long total = (long long)a.n * a.oh * gw;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int g = (int)(i % gw);
    const long long r = i / gw;  // output row over all planes
    const int oy = (int)(r % a.oh);
    const long long b = r / a.oh;
    const int ox = 4 * g, cnt = min(4, a.ow - ox);
    float xv[4], yv[4];
    if (a.pool) {
      const int y0 = 2 * oy, y1 = min(2 * oy + 1, a.h - 1);
      const long long r0 = (b * a.h + y0) * a.w, r1 = (b * a.h + y1) * a.w;
      float t0[8], t1[8], u0[8], u1[8];
      if constexpr (VEC) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          ld4(t0 + 4 * k, a.x + r0 + 2 * ox + 4 * k);
          ld4(t1 + 4 * k, a.x + r1 + 2 * ox + 4 * k);
          ld4(u0 + 4 * k, a.y + r0 + 2 * ox + 4 * k);
          ld4(u1 + 4 * k, a.y + r1 + 2 * ox + 4 * k);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int xx = min(2 * ox + k, a.w - 1);  // the repeated last column; past cnt: unused
          t0[k] = a.x[r0 + xx], t1[k] = a.x[r1 + xx], u0[k] = a.y[r0 + xx], u1[k] = a.y[r1 + xx];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xv[k] = pool4(t0[2 * k], t0[2 * k + 1], t1[2 * k], t1[2 * k + 1]);
        yv[k] = pool4(u0[2 * k], u0[2 * k + 1], u1[2 * k], u1[2 * k + 1]);
      }
    } else {
      const long long r0 = r * a.w + ox;
      if constexpr (VEC) {
        ld4(xv, a.x + r0);
        ld4(yv, a.y + r0);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int kk = min(k, cnt - 1);
          xv[k] = a.x[r0 + kk], yv[k] = a.y[r0 + kk];
        }
      }
    }
    float pv[4], qv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pv[k] = __fmul_rn(xv[k], yv[k]);
      qv[k] = __fadd_rn(__fmul_rn(xv[k], xv[k]), __fmul_rn(yv[k], yv[k]));
    }
    const long long o = r * a.ow + ox;
    if constexpr (VEC) {
      if (a.xp) st4(a.xp + o, xv);
      if (a.yp) st4(a.yp + o, yv);
      if (a.pxy) st4(a.pxy + o, pv);
      if (a.pss) st4(a.pss + o, qv);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < cnt) {
          if (a.xp) a.xp[o + k] = xv[k];
          if (a.yp) a.yp[o + k] = yv[k];
          if (a.pxy) a.pxy[o + k] = pv[k];
          if (a.pss) a.pss[o + k] = qv[k];
        }
      }
    }
  }
}
// Its adjoint.  At the coarse size the gradient that reaches x' is gx = dx' + dP y' + 2 dQ x' (and
// gy = dy' + dP x' + 2 dQ y'); every fine pixel (r, c) belongs to exactly one 2x2 window, the
// repeated last row / column of an odd size a second time to the same one, so
//   dx[r][c] = 0.25 gx[r / 2][c / 2] (2 if r is the repeated row) (2 if c is the repeated column)
// and each output element is written once.  One thread per four fine columns of one fine row.
struct PoolPrepGradArgs {
  const float *dxp, *dyp, *dp, *dq;  // (n, oh, ow); null: zero
  const float *xp, *yp;              // the saved x', y' (read only with dp or dq)
  float *dx, *dy;                    // (n, h, w)
  int n, h, w, oh, ow, pool;
};
template <bool VEC>
__global__ __launch_bounds__(256) void pool2_prep_grad_kernel(PoolPrepGradArgs a) {
  const int gw = (a.w + 3) / 4;
  const long long total = (long long)a.n * a.h * gw;
  const bool prod = a.dp || a.dq;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int g = (int)(i % gw);
    const long long r = i / gw;  // fine row over all planes
    const int fy = (int)(r % a.h);
    const long long b = r / a.h;
    const int fx = 4 * g, cnt = min(4, a.w - fx);
    // the coarse elements under the four fine columns: two (pool) or four (no pool)
    const int nc = a.pool ? 2 : 4;
    const int cy = a.pool ? fy >> 1 : fy, cx = a.pool ? fx >> 1 : fx;
    const long long co = (b * a.oh + cy) * a.ow + cx;
    float gx[4], gy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      gx[k] = 0.f, gy[k] = 0.f;
      if (k < nc && cx + k < a.ow) {
        const long long e = co + k;
        const float dxp = a.dxp ? a.dxp[e] : 0.f, dyp = a.dyp ? a.dyp[e] : 0.f;
        float sx = dxp, sy = dyp;
        if (prod) {
          const float xv = a.xp[e], yv = a.yp[e];
          const float dp = a.dp ? a.dp[e] : 0.f, dq2 = a.dq ? __fmul_rn(2.0f, a.dq[e]) : 0.f;
          sx = fmaf(dq2, xv, fmaf(dp, yv, dxp));
          sy = fmaf(dq2, yv, fmaf(dp, xv, dyp));
        }
        gx[k] = sx, gy[k] = sy;
      }
    }
    float ox[4], oy[4];
    if (a.pool) {
      const float ry = ((a.h & 1) && fy == a.h - 1) ? 0.5f : 0.25f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float f = ((a.w & 1) && fx + k == a.w - 1) ? __fmul_rn(2.0f, ry) : ry;
        ox[k] = __fmul_rn(f, gx[k >> 1]);
        oy[k] = __fmul_rn(f, gy[k >> 1]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) ox[k] = gx[k], oy[k] = gy[k];
    }
    const long long o = r * a.w + fx;
    if constexpr (VEC) {
      st4(a.dx + o, ox);
      st4(a.dy + o, oy);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < cnt) a.dx[o + k] = ox[k], a.dy[o + k] = oy[k];
      }
    }
  }
}

// ---- separable Gaussian of the SSIM loss (tf.image.ssim's 11-tap window) --------------------
// One-channel planes (n, h, w): VALID correlation along x (vertical = 0) or y, or its adjoint
// (the input gradient: a full convolution with the same taps).
__global__ __launch_bounds__(256) void gauss1d_kernel(const float* __restrict__ in, int n, int hi, int wi,
                                                      const float* __restrict__ taps, int nt, int vertical, int adjoint,
                                                      float* __restrict__ out, int ho, int wo) {
  const long long total = (long long)n * ho * wo;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % wo);
    const long long r = i / wo;
    const int y = (int)(r % ho), b = (int)(r / ho);
    const float* src = in + (long long)b * hi * wi;
    float s = 0.f;
    for (int k = 0; k < nt; ++k) {
      const int yy = vertical ? (adjoint ? y - k : y + k) : y;
      const int xx = vertical ? x : (adjoint ? x - k : x + k);
      if ((unsigned)yy < (unsigned)hi && (unsigned)xx < (unsigned)wi) s = fmaf(taps[k], src[(long long)yy * wi + xx], s);
    }
    out[i] = s;
  }
}

// ---- weight-gradient GEMM ------------------------------------------------------------------
struct WgradArgs {
  const float* gat;   // [n][gh][gw][ca], read at s*u + k - pad
  const float* dir;   // [n][uh][uw][cb]
  const float* sg;    // device scales or null
  const float* sd;
  float* part;        // [slices][taps * ca rows][cb]
  int n, gh, gw, ca, uh, uw, cb, kh, kw, stride, pad_y, pad_x;
  int rows;           // taps * ca: the GEMM's M (row r = tap * ca + a)
  long long U;        // n * uh * uw
  int slice_len;      // pixels per slice (multiple of TK)
};

// M = (tap, a) rows flattened (r = tap * ca + a), N = b, K = the slice's pixels.  NA rows
// per block (16 ... 64: one tap of a 64-channel gat, two taps of a 32-channel one, or all
// 25 taps of a one-channel one), NB >= cb; block (row block, slice) stages the dir
// tile once for all its rows; wave w owns the 16 x 16 output tiles w, w + 4, ...
template <int NA, int NB>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
  constexpr int NMAX = NA > NB ? NA : NB;
  __shared__ __attribute__((aligned(16))) _Float16 gs[2][NMAX * LP];  // [hi, lo][a][u]
  __shared__ __attribute__((aligned(16))) _Float16 ds[2][NMAX * LP];  // [hi, lo][b][u]
  constexpr int NTA = NA / 16, NTB = NB / 16, NTILE = NTA * NTB, TPW = (NTILE + 3) / 4;
  // staging: thread item = (channel, 4 consecutive pixels u): 4 loads coalesced across the
  // channel-contiguous lanes, one f16x4 hi and one lo store into the [channel][u] tiles
  constexpr int GE = (TK / 4 * NA + 255) / 256, DE = (TK / 4 * NB + 255) / 256;
  typedef _Float16 f16x4v __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, l16 = lane & 15;
  const int r0 = blockIdx.x * NA, slice = blockIdx.y;
  const long long u0 = (long long)slice * a.slice_len;
  const long long u1 = u0 + a.slice_len < a.U ? u0 + a.slice_len : a.U;
  const float sg = ld_scale(a.sg), sd = ld_scale(a.sd);
  const long long per = (long long)a.uh * a.uw;

  f32x4 gv[GE], dv[DE];
  // pixel coordinates (b, uy, ux) of each gat item's first u, advanced by TK per chunk with
  // compares instead of the per-element integer divisions they replace
  int ib_[GE], iy_[GE], ix_[GE];
#pragma unroll
  for (int e = 0; e < GE; ++e) {
    const long long u = u0 + 4 * ((tid + 256 * e) / NA);
    ib_[e] = (int)(u / per);
    const int r = (int)(u - (long long)ib_[e] * per);
    iy_[e] = r / a.uw;
    ix_[e] = r - iy_[e] * a.uw;
  }
  auto step_pix = [&](int& b, int& y, int& x, int d) {
    x += d;
    while (x >= a.uw) {
      x -= a.uw;
      if (++y == a.uh) {
        y = 0;
        ++b;
      }
    }
  };
  auto load = [&](long long ub) {
#pragma unroll
    for (int e = 0; e < GE; ++e) {
      const int idx = tid + 256 * e, ug = idx / NA, row = r0 + idx % NA;
      const int tap = row / a.ca, ch = row - tap * a.ca, ky = tap / a.kw, kx = tap - ky * a.kw;
      int b = ib_[e], uy = iy_[e], ux = ix_[e];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long u = ub + 4 * ug + i;
        if (i) step_pix(b, uy, ux, 1);
        float v = 0.f;
        if (idx < TK / 4 * NA && row < a.rows && u < u1) {
          const int gy = a.stride * uy + ky - a.pad_y, gx = a.stride * ux + kx - a.pad_x;
          if ((unsigned)gy < (unsigned)a.gh && (unsigned)gx < (unsigned)a.gw)
            v = a.gat[(((size_t)b * a.gh + gy) * a.gw + gx) * a.ca + ch];
        }
        gv[e][i] = v;
      }
      step_pix(ib_[e], iy_[e], ix_[e], TK);  // this item's first u in the next chunk
    }
#pragma unroll
    for (int e = 0; e < DE; ++e) {
      const int idx = tid + 256 * e, ug = idx / NB, ch = idx % NB;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long u = ub + 4 * ug + i;
        dv[e][i] = (idx < TK / 4 * NB && ch < a.cb && u < u1) ? a.dir[u * a.cb + ch] : 0.f;
      }
    }
  };
  auto put = [&](_Float16 (&tile)[2][(NA > NB ? NA : NB) * LP], int row, int col, const f32x4& v, float s) {
    f16x4v hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      _Float16 h, l;
      split1(v[i] * s, h, l);
      hi[i] = h;
      lo[i] = l;
    }
    *(f16x4v*)&tile[0][row * LP + col] = hi;
    *(f16x4v*)&tile[1][row * LP + col] = lo;
  };
  auto stage = [&]() {
#pragma unroll
    for (int e = 0; e < GE; ++e) {
      const int idx = tid + 256 * e;
      if (idx < TK / 4 * NA) put(gs, idx % NA, 4 * (idx / NA), gv[e], sg);
    }
#pragma unroll
    for (int e = 0; e < DE; ++e) {
      const int idx = tid + 256 * e;
      if (idx < TK / 4 * NB) put(ds, idx % NB, 4 * (idx / NB), dv[e], sd);
    }
  };

  f32x4 acc[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (u0 < u1) load(u0);
  for (long long ub = u0; ub < u1; ub += TK) {
    __syncthreads();
    stage();
    __syncthreads();
    if (ub + TK < u1) load(ub + TK);
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int t = wave + 4 * j;
      if (t >= NTILE) break;  // wave-uniform
      const int ta = t / NTB, tb = t - ta * NTB;
      const int ao = (ta * 16 + l16) * LP + 8 * g, bo = (tb * 16 + l16) * LP + 8 * g;
      const f16x8 ah = *(const f16x8*)&gs[0][ao], al = *(const f16x8*)&gs[1][ao];
      const f16x8 bh = *(const f16x8*)&ds[0][bo], bl = *(const f16x8*)&ds[1][bo];
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc[j], 0, 0, 0);
    }
  }
  const float isg = 1.0f / sg, isd = 1.0f / sd;
  float* out = a.part + ((size_t)slice * a.rows + r0) * a.cb;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int t = wave + 4 * j;
    if (t >= NTILE) break;
    const int ta = t / NTB, tb = t - ta * NTB, bcol = tb * 16 + l16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int arow = ta * 16 + 4 * g + r;
      if (r0 + arow < a.rows && bcol < a.cb) out[(size_t)arow * a.cb + bcol] = (acc[j][r] * isg) * isd;
    }
  }
}

// dw[i] = sum over slices of part[s][i]: 8 independent loads in flight per thread, summed
// in a fixed order (deterministic)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int slices, long long nw,
                                                           float* __restrict__ dw) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nw; i += (long long)gridDim.x * 256) {
    float s = 0.f;
    int k = 0;
    for (; k + 8 <= slices; k += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = part[(size_t)(k + j) * nw + i];
      s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    for (; k < slices; ++k) s += part[(size_t)k * nw + i];
    dw[i] = s;
  }
}

// ---- power-of-two operand scales -------------------------------------------------------------
constexpr int kScaleBlocks = 512;

__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, long long n, float* __restrict__ part) {
  float m = 0.f;
  const long long n4 = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) ? n / 4 : 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const f32x4 v = ((const f32x4*)x)[i];
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
  }
  for (long long i = 4 * n4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    m = fmaxf(m, fabsf(x[i]));
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  __shared__ float wm[4];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
}

// scale = 2^(13 - floor(log2 max)): max * scale in [2^13, 2^14) (1 for a zero / infinite max;
// fmaxf skips NaN elements, so they never reach max)
__global__ __launch_bounds__(256) void scale_finish_kernel(const float* __restrict__ part, int nb, float* __restrict__ scale) {
  float m = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) m = fmaxf(m, part[i]);
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  __shared__ float wm[4];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    float s = 1.0f;
    if (m > 0.f && isfinite(m)) s = ldexpf(1.0f, min(max(13 - ilogbf(m), -126), 126));
    *scale = s;
  }
}

template <int NT, bool VEC, bool PH>
hipError_t launch_gather_t(const GatherArgs& a, hipStream_t st) {
  const long long blocks = PH ? a.ph_blk[4] : (a.M + GM - 1) / GM;
  hipLaunchKernelGGL((conv_gather_kernel<NT, VEC, PH>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

template <int NA, int NB>
hipError_t launch_wgrad_t(const WgradArgs& a, int slices, hipStream_t st) {
  hipLaunchKernelGGL((conv_wgrad_kernel<NA, NB>), dim3((a.rows + NA - 1) / NA, slices), dim3(256), 0, st, a);
  return hipGetLastError();
}

int tile16(int c) { return c <= 16 ? 16 : c <= 32 ? 32 : 64; }

}  // namespace

size_t train_scale_work_floats() { return kScaleBlocks; }

hipError_t launch_absmax_scale(const float* x, long long n, float* scale, float* work, hipStream_t st) {
  const long long want = (n / 4 + 255) / 256;
  const int nb = (int)(want < 1 ? 1 : want > kScaleBlocks ? kScaleBlocks : want);
  hipLaunchKernelGGL(absmax_kernel, dim3(nb), dim3(256), 0, st, x, n, work);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(scale_finish_kernel, dim3(1), dim3(256), 0, st, work, nb, scale);
  return hipGetLastError();
}

size_t train_gather_work_bytes(int kh, int kw, int cin, int cout) {
  return (size_t)((kh * kw * cin + TK - 1) / TK) * (tile16(cout) / 16) * 2 * 64 * sizeof(f16x8);
}

size_t train_abg_work_floats(long long rows, int cols) {
  return (size_t)((rows + kAbgRows - 1) / kAbgRows) * (cols + 1);
}

hipError_t launch_act_bias_grad(const float* y, const float* dy, long long rows, int cols, int act, float* dz, float* db,
                                float* dz_scale, float* work, hipStream_t st) {
  const long long nblk = (rows + kAbgRows - 1) / kAbgRows;
  if (nblk > INT32_MAX) return hipErrorInvalidValue;
  if (nblk == 0 && db) {
    const hipError_t e = hipMemsetAsync(db, 0, (size_t)cols * sizeof(float), st);
    if (e != hipSuccess) return e;
  }
  if (nblk > 0) {
    const bool vec = cols % 4 == 0 && (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)dz) & 15) == 0;
    if (vec)
      hipLaunchKernelGGL(act_bias_grad_kernel<4>, dim3((unsigned)nblk), dim3(256), 0, st, y, dy, rows, cols, act, dz, work);
    else
      hipLaunchKernelGGL(act_bias_grad_kernel<1>, dim3((unsigned)nblk), dim3(256), 0, st, y, dy, rows, cols, act, dz, work);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if ((db && nblk > 0) || dz_scale) {  // (an empty tensor's scale: 1)
    hipLaunchKernelGGL(abg_reduce_kernel, dim3((unsigned)cols + 1), dim3(256), 0, st, work, (int)nblk, cols,
                       nblk > 0 ? db : nullptr, dz_scale);
    return hipGetLastError();
  }
  return hipSuccess;
}

hipError_t launch_conv_gather(const float* x, int n, int h, int w, int cin, const float* wt, int kh, int kw, int layout,
                              int stride, int pad_y, int pad_x, int transposed, const float* bias, const float* x_scale,
                              const float* w_scale, float* y, int oh, int ow, int cout, int act, void* work,
                              hipStream_t st) {
  GatherArgs a{};
  a.act = act;
  a.x = x; a.wp = (const f16x8*)work; a.bias = bias; a.y = y;
  a.sx = x_scale; a.sw = w_scale;
  a.n = n; a.h = h; a.w = w; a.cin = cin; a.oh = oh; a.ow = ow; a.cout = cout; a.kh = kh; a.kw = kw;
  a.stride = stride; a.pad_y = pad_y; a.pad_x = pad_x; a.transposed = transposed;
  a.K = kh * kw * cin;
  a.M = (long long)n * oh * ow;
  if (a.M == 0) return hipSuccess;
  const int ntt = tile16(cout) / 16, nchunk = (a.K + TK - 1) / TK;
  {
    const int total = nchunk * ntt * 64;
    hipLaunchKernelGGL(pack_w_kernel, dim3((total + 255) / 256), dim3(256), 0, st, wt, layout, cin, cout, a.K, ntt,
                       nchunk, w_scale, (f16x8*)work);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const bool vec = cin % TK == 0 && ((uintptr_t)x & 15) == 0;
  const bool ph = vec && transposed && stride == 2;
  if (ph) {  // blocks per output phase
    a.ph_blk[0] = 0;
    for (int p = 0; p < 4; ++p) {
      const long long qh = (oh - (p >> 1) + 1) / 2, qw = (ow - (p & 1) + 1) / 2;
      a.ph_blk[p + 1] = a.ph_blk[p] + (int)((n * qh * qw + GM - 1) / GM);
    }
    if (a.ph_blk[4] == 0) return hipSuccess;
  }
  switch (tile16(cout) | (vec ? 1 : 0) | (ph ? 2 : 0)) {
    case 16: return launch_gather_t<16, false, false>(a, st);
    case 17: return launch_gather_t<16, true, false>(a, st);
    case 19: return launch_gather_t<16, true, true>(a, st);
    case 32: return launch_gather_t<32, false, false>(a, st);
    case 33: return launch_gather_t<32, true, false>(a, st);
    case 35: return launch_gather_t<32, true, true>(a, st);
    case 64: return launch_gather_t<64, false, false>(a, st);
    case 65: return launch_gather_t<64, true, false>(a, st);
    default: return launch_gather_t<64, true, true>(a, st);
  }
}

static bool aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if ((uintptr_t)p & 15) return false;  // (null counts as aligned: it is not accessed)
  return true;
}

// two partials (lum cs, cs) per block of kSsimPix pixels
size_t train_msssim_work_floats(int n, long long hw) { return 2 * (size_t)n * ((hw + kSsimPix - 1) / kSsimPix); }

hipError_t launch_msssim_terms(const float* mx, const float* my, const float* sxy, const float* sxx, int n,
                               long long hw, float c1, float c2, float* lcs_mean, float* cs_mean, float* work,
                               hipStream_t st) {
  const long long bpi = (hw + kSsimPix - 1) / kSsimPix;
  if (n == 0) return hipSuccess;
  if (bpi * n > INT32_MAX || bpi > INT32_MAX) return hipErrorInvalidValue;
  const bool vec = hw % 4 == 0 && aligned16({mx, my, sxy, sxx});
  const dim3 grid((unsigned)(bpi * n));
  if (vec)
    hipLaunchKernelGGL(msssim_terms_kernel<true>, grid, dim3(256), 0, st, mx, my, sxy, sxx, hw, (int)bpi, c1, c2, work);
  else
    hipLaunchKernelGGL(msssim_terms_kernel<false>, grid, dim3(256), 0, st, mx, my, sxy, sxx, hw, (int)bpi, c1, c2, work);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(msssim_mean_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, work, n, (int)bpi, hw,
                     lcs_mean, cs_mean);
  return hipGetLastError();
}

hipError_t launch_msssim_terms_grad(const float* mx, const float* my, const float* sxy, const float* sxx,
                                    const float* g_ssim, const float* g_cs, int n, long long hw, float c1, float c2,
                                    float* gmx, float* gmy, float* gsxy, float* gsxx, hipStream_t st) {
  if ((long long)n * hw == 0) return hipSuccess;
  const bool vec = hw % 4 == 0 && aligned16({mx, my, sxy, sxx, gmx, gmy, gsxy, gsxx});
  const long long blocks = ((long long)n * hw / (vec ? 4 : 1) + 255) / 256;
  const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536));
  if (vec)
    hipLaunchKernelGGL(msssim_terms_grad_kernel<true>, grid, dim3(256), 0, st, mx, my, sxy, sxx, g_ssim, g_cs, n, hw, c1,
                       c2, gmx, gmy, gsxy, gsxx);
  else
    hipLaunchKernelGGL(msssim_terms_grad_kernel<false>, grid, dim3(256), 0, st, mx, my, sxy, sxx, g_ssim, g_cs, n, hw,
                       c1, c2, gmx, gmy, gsxy, gsxx);
  return hipGetLastError();
}

// the forward's partial per block of kRatePix elements, or the backward's C x 256 partial table per
// block of kRateSlab pixels of a group and per context, whichever is more (one `work` serves both
// calls)
static long long rate_slabs(int m, int h, int w, int groups) {
  return ((long long)(m / groups) * h * w + kRateSlab - 1) / kRateSlab;
}
size_t train_rate_work_floats(int m, int h, int w, int c, int groups, int contexts) {
  const long long fwd = (long long)m * (((long long)h * w * c + kRatePix - 1) / kRatePix);
  const long long bwd = (long long)contexts * groups * rate_slabs(m, h, w, groups) * c * 256;
  return (size_t)(fwd > bwd ? fwd : bwd);
}

template <int NX>
static hipError_t rate_fwd(const float* y, const float* yc, const float* L, const unsigned char* anchors, int m, int h,
                           int w, int c, int groups, int seg_pixels, float* plane_bits, float* work, hipStream_t st) {
  const int elems = h * w * c, bpp = (elems + kRatePix - 1) / kRatePix;
  if ((long long)m * bpp > INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rate_kernel<NX>, dim3((unsigned)(m * bpp)), dim3(256), 0, st, y, yc, L, anchors, elems, c,
                     m / groups, bpp, seg_pixels, work);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rate_table_sum_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, work, m, bpp, plane_bits);
  return hipGetLastError();
}

template <int NX>
static hipError_t rate_bwd(const float* y, const float* yc, const float* L, const unsigned char* anchors, const float* g,
                           int m, int h, int w, int c, int groups, int seg_pixels, float* dy, float* dL, float* work,
                           hipStream_t st) {
  const int elems = h * w * c;
  if (dy) {
    const long long total = (long long)m * elems, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(rate_dy_kernel<NX>, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, y, yc, L,
                       anchors, g, total, elems, c, m / groups, seg_pixels, dy);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (dL) {
    const long long spg = rate_slabs(m, h, w, groups);
    if (NX * groups * spg > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rate_dl_kernel<NX>, dim3((unsigned)(NX * groups * spg)), dim3(64), 0, st, y, yc, anchors, g, c,
                       h * w, (long long)(m / groups) * h * w, (int)spg, seg_pixels, work);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rate_dl_reduce_kernel<NX>, dim3((unsigned)((groups * NX * c * 256 + 255) / 256)), dim3(256), 0,
                       st, work, groups, c, (int)spg, dL);
    return hipGetLastError();
  }
  return hipSuccess;
}

hipError_t launch_rate(const float* y, const float* L, int contexts, const float* yc, const unsigned char* anchors,
                       int seg_pixels, int m, int h, int w, int c, int groups, float* plane_bits, float* work,
                       hipStream_t st) {
  if (contexts != 1 && contexts != 3) return hipErrorInvalidValue;
  if (m == 0) return hipSuccess;
  if (!yc) yc = y;
  return contexts == 1 ? rate_fwd<1>(y, yc, L, anchors, m, h, w, c, groups, seg_pixels, plane_bits, work, st)
                       : rate_fwd<3>(y, yc, L, anchors, m, h, w, c, groups, seg_pixels, plane_bits, work, st);
}

hipError_t launch_rate_grad(const float* y, const float* L, int contexts, const float* yc, const unsigned char* anchors,
                            int seg_pixels, const float* g, int m, int h, int w, int c, int groups, float* dy,
                            float* dL, float* work, hipStream_t st) {
  if (contexts != 1 && contexts != 3) return hipErrorInvalidValue;
  if (m == 0) return dL ? hipMemsetAsync(dL, 0, (size_t)groups * c * contexts * 256 * sizeof(float), st) : hipSuccess;
  if (!yc) yc = y;
  return contexts == 1 ? rate_bwd<1>(y, yc, L, anchors, g, m, h, w, c, groups, seg_pixels, dy, dL, work, st)
                       : rate_bwd<3>(y, yc, L, anchors, g, m, h, w, c, groups, seg_pixels, dy, dL, work, st);
}

hipError_t launch_pool2_prep(const float* x, const float* y, int n, int h, int w, int pool, float* xp, float* yp,
                             float* pxy, float* pss, hipStream_t st) {
  PoolPrepArgs a;
  a.x = x, a.y = y, a.xp = xp, a.yp = yp, a.pxy = pxy, a.pss = pss;
  a.n = n, a.h = h, a.w = w, a.pool = pool;
  a.oh = pool ? (h + 1) / 2 : h, a.ow = pool ? (w + 1) / 2 : w;
  const long long total = (long long)n * a.oh * ((a.ow + 3) / 4);
  if (total == 0) return hipSuccess;
  const bool vec = w % (pool ? 8 : 4) == 0 && aligned16({x, y, xp, yp, pxy, pss});
  const long long blocks = (total + 255) / 256;
  const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536));
  if (vec)
    hipLaunchKernelGGL(pool2_prep_kernel<true>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(pool2_prep_kernel<false>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_pool2_prep_grad(const float* dxp, const float* dyp, const float* dp, const float* dq, const float* xp,
                                  const float* yp, int n, int h, int w, int pool, float* dx, float* dy, hipStream_t st) {
  PoolPrepGradArgs a;
  a.dxp = dxp, a.dyp = dyp, a.dp = dp, a.dq = dq, a.xp = xp, a.yp = yp, a.dx = dx, a.dy = dy;
  a.n = n, a.h = h, a.w = w, a.pool = pool;
  a.oh = pool ? (h + 1) / 2 : h, a.ow = pool ? (w + 1) / 2 : w;
  const long long total = (long long)n * h * ((w + 3) / 4);
  if (total == 0) return hipSuccess;
  const bool vec = w % 4 == 0 && aligned16({dx, dy});
  const long long blocks = (total + 255) / 256;
  const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536));
  if (vec)
    hipLaunchKernelGGL(pool2_prep_grad_kernel<true>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(pool2_prep_grad_kernel<false>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_gauss1d(const float* in, int n, int hi, int wi, const float* taps, int nt, int vertical, int adjoint,
                          float* out, int ho, int wo, hipStream_t st) {
  const long long total = (long long)n * ho * wo;
  if (total == 0) return hipSuccess;
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(gauss1d_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, in, n, hi,
                     wi, taps, nt, vertical, adjoint, out, ho, wo);
  return hipGetLastError();
}

// rows per block: 64 (one tap of a 64-channel gat, two of a 32-channel one) / 32 / 16 rows
// (all 25 taps of a one-channel gat)
static int wgrad_na(int taps, int ca) {
  const int rows = taps * ca;
  (void)taps;
  return rows > 32 ? 64 : rows > 16 ? 32 : 16;  // (two taps of 64 channels per block, NA 128: measured 35 % slower)
}

// slices so that row blocks x slices fills the chip about eight times over, each slice
// >= 4 chunks
static int wgrad_slices(long long U, int rowblocks) {
  long long want = (2048 + rowblocks - 1) / rowblocks;
  const long long maxs = (U + 4 * TK - 1) / (4 * TK);
  if (want > maxs) want = maxs;
  return (int)(want < 1 ? 1 : want);
}

size_t train_wgrad_work_floats(int n, int uh, int uw, int kh, int kw, int ca, int cb) {
  const long long U = (long long)n * uh * uw;
  const int rows = kh * kw * ca, na = wgrad_na(kh * kw, ca);
  return (size_t)wgrad_slices(U, (rows + na - 1) / na) * rows * cb;
}

hipError_t launch_conv_wgrad(const float* gat, int n, int gh, int gw, int ca, const float* dir, int uh, int uw, int cb,
                             int kh, int kw, int stride, int pad_y, int pad_x, const float* gat_scale,
                             const float* dir_scale, float* dw, float* work, hipStream_t st) {
  WgradArgs a{};
  a.gat = gat; a.dir = dir; a.sg = gat_scale; a.sd = dir_scale;
  a.part = work;
  a.n = n; a.gh = gh; a.gw = gw; a.ca = ca; a.uh = uh; a.uw = uw; a.cb = cb; a.kh = kh; a.kw = kw;
  a.stride = stride; a.pad_y = pad_y; a.pad_x = pad_x;
  a.U = (long long)n * uh * uw;
  const int taps = kh * kw;
  const long long nw = (long long)taps * ca * cb;
  if (nw == 0) return hipSuccess;
  if (a.U == 0) return hipMemsetAsync(dw, 0, nw * sizeof(float), st);
  a.rows = taps * ca;
  const int na = wgrad_na(taps, ca);
  const int slices = wgrad_slices(a.U, (a.rows + na - 1) / na);
  a.slice_len = (int)(((a.U + slices - 1) / slices + TK - 1) / TK * TK);
  hipError_t e;
  switch (na * 1000 + tile16(cb)) {
    case 16016: e = launch_wgrad_t<16, 16>(a, slices, st); break;
    case 16032: e = launch_wgrad_t<16, 32>(a, slices, st); break;
    case 16064: e = launch_wgrad_t<16, 64>(a, slices, st); break;
    case 32016: e = launch_wgrad_t<32, 16>(a, slices, st); break;
    case 32032: e = launch_wgrad_t<32, 32>(a, slices, st); break;
    case 32064: e = launch_wgrad_t<32, 64>(a, slices, st); break;
    case 64016: e = launch_wgrad_t<64, 16>(a, slices, st); break;
    case 64032: e = launch_wgrad_t<64, 32>(a, slices, st); break;
    default: e = launch_wgrad_t<64, 64>(a, slices, st); break;
  }
  if (e != hipSuccess) return e;
  const long long rb = (nw + 255) / 256;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(rb < 1024 ? rb : 1024)), dim3(256), 0, st, work, slices, nw, dw);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// tf.keras Adam (training.py:147-149 `optimizer.apply_gradients`; Keras' OptimizerV2 Adam calls
// TensorFlow's ResourceApplyAdam with use_nesterov = false) over many tensors in one launch.
// TF's ApplyAdam functor (training_ops, published algorithm; TF is not in the reference tree):
//   alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t)     (host, fp32, as Keras' iteration powers)
//   m += (g - m) * (1 - beta1);  v += (g * g - v) * (1 - beta2)
//   var -= (m * alpha) / (sqrt(v) + epsilon)
// every op an fp32 rounding in that order (no contraction: -ffp-contract=off; sqrt and the
// division correctly rounded, as NumPy's fp32 ops: the GPU test is bit-exact against them).  Block (x, k) updates elements [1024 x, 1024 x + 1024) of
// tensor k, then the same range one grid-width further on (n > max_n is covered), k's {var, m, v, grad, n} record is table[5k .. 5k+4].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_keras_kernel(const long long* __restrict__ table, float alpha, float b1c,
                                                         float b2c, float eps) {
  const long long* r = table + 5 * blockIdx.y;
  float* var = (float*)r[0];
  float* m = (float*)r[1];
  float* v = (float*)r[2];
  const float* g = (const float*)r[3];
  const long long n = r[4];
  // grid-stride over the record: a record longer than the max_n that sized the grid is
  // still updated whole
  for (long long base = (long long)blockIdx.x * 1024; base < n; base += (long long)gridDim.x * 1024)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = base + k * 256 + threadIdx.x;
    if (i >= n) break;
    const float gi = g[i];
    const float mi = __fadd_rn(m[i], __fmul_rn(__fsub_rn(gi, m[i]), b1c));
    const float vi = __fadd_rn(v[i], __fmul_rn(__fsub_rn(__fmul_rn(gi, gi), v[i]), b2c));
    m[i] = mi;
    v[i] = vi;
    // sqrt correctly rounded: the f64 square root rounded to f32 (double rounding is exact for
    // sqrt at 53 >= 2 x 24 + 2 bits; v_sqrt_f32 alone is within 1 ulp, not correctly rounded)
    const float sv = (float)__dsqrt_rn((double)vi);
    var[i] = __fsub_rn(var[i], __fdiv_rn(__fmul_rn(mi, alpha), __fadd_rn(sv, eps)));
  }
}

hipError_t launch_adam_keras(const long long* table, int count, long long max_n, float alpha, float beta1,
                             float beta2, float eps, hipStream_t st) {
  if (count <= 0 || max_n <= 0) return hipSuccess;
  const long long bx = (max_n + 1023) / 1024;
  if (bx > INT32_MAX || count > 65535) return hipErrorInvalidValue;
  const float b1c = 1.0f - beta1, b2c = 1.0f - beta2;  // fp32, as T(1) - beta
  hipLaunchKernelGGL(adam_keras_kernel, dim3((unsigned)bx, (unsigned)count), dim3(256), 0, st, table, alpha, b1c, b2c,
                     eps);
  return hipGetLastError();
}

}  // namespace nic
