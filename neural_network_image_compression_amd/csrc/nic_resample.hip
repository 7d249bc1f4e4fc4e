// Crops for training: boxes of any sizes out of u8 NHWC images, resized to one oh x ow output,
// mirrored, normalised and laid out for the model, one launch (nic.h, "Crops of mixed sizes";
// DESIGN.md, "Crops of mixed sizes, resized on the device").
//
// The resize is torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=True):
// per axis, with s = in / out and support = max(s, 1), output i has its centre at c = s (i + 0.5), taps
// [lo, hi) = [max(0, int(c - support + 0.5)), min(int(c + support + 0.5), in)) and tap p the weight
// 1 - |p + 0.5 - c| / support, divided by the taps' sum.  Everything about a tap is a ratio of small
// integers, so the kernel keeps it that way: with D = 2 max(in, out) and
//   N(p) = (2 p + 1) out - in (2 i + 1),            |N(p)| <= D for every tap of [lo, hi),
// tap p weighs D - |N(p)| (an integer, exact in fp32 below 2^24) and the taps' sum is an integer in
// closed form.  lo and hi are floor divisions of integers.  An output pixel is
//   (sum_y wy (sum_x wx v) / sum_wx) / sum_wy
// in fp32: the inner sum is a sum of integers, the outer one rounds once per tap row, the two
// divisions are IEEE.  At in == out the one tap that counts weighs D and the output is the source
// pixel itself.
//
// grid (tiles of kTH x kTW output pixels, n), block 256 = one thread per pixel of the tile:
//   1. the block reads its table row and leaves if the row is not one the kernel may act on;
//   2. kTH + kTW threads compute the tile's per-row and per-column taps {lo, cnt, N(lo), sum} into
//      LDS -- 16 bytes per output row or column whatever the scale, the weights follow from N;
//   3. the source rectangle the tile's taps cover is staged into LDS as dwords, row by row, each row
//      from the dword that holds its first byte (coalesced 4-byte loads; a dword that is not wholly
//      inside the image is assembled from guarded bytes).  A rectangle above kStageDwords is not
//      staged: the taps then read the image in global memory, the same loop over another pointer;
//   4. every thread resamples its pixel and applies the value rule;
//   5. the tile is stored: fp32 planes straight from the registers (4 bytes per lane, contiguous
//      along ow), f16 planes and the u8 NHWC rows through an LDS tile, as whole aligned dwords with
//      single elements only where a run starts or ends inside a dword.
//
// Steps 2 to 5 are resample_tile, which knows one source image by its first byte, its shape and its
// end.  resample_boxes finds image i of a dense (n, Hs, Ws, 3) stack; resample_ragged finds it in a pool
// of images of any shapes through the row's own offset, Hs and Ws ("Images of mixed sizes,
// resized and encoded in one batch").  There the pitch 3 Ws and the base differ per row, and a source
// row starts at any of a dword's four bytes; step 3 already aligns by the address and guards by the
// image's own end, so it is the same code.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nic.h"
#include "nic_kernels.h"

namespace nic {
namespace {

constexpr int kTH = 8, kTW = 32;     // the tile: output rows x columns, one thread each
constexpr int kStageDwords = 8192;   // 32 KB of source per block: scales up to about 5.5 are staged
constexpr long long kMaxPixels = 1ll << 29;  // Hs Ws of one source: nic_resample_boxes' limit, a ragged row's too

struct Taps {
  int lo, cnt, n0;  // the first tap, the tap count, N(lo)
  float sum;        // the sum of the taps' integer weights
};

__device__ Taps axis_taps(int in, int out, int i) {
  const long long c2 = (long long)in * (2 * i + 1);        // 2 out c
  const long long d = 2ll * (in > out ? in : out);         // D = 2 out support
  long long lo = (c2 - d + out) / (2ll * out);             // negative numerators end at 0 either way
  long long hi = (c2 + d + out) / (2ll * out);
  lo = lo < 0 ? 0 : lo;
  hi = hi > in ? in : hi;
  const long long cnt = hi - lo, step = 2ll * out;
  const long long n0 = (2 * lo + 1) * out - c2;
  // sum_j |n0 + j step| over j < cnt: the first k terms are negative
  long long k = n0 >= 0 ? 0 : (-n0 + step - 1) / step;
  k = k > cnt ? cnt : k;
  const long long all = n0 * cnt + step * (cnt * (cnt - 1) / 2), neg = n0 * k + step * (k * (k - 1) / 2);
  Taps t;
  t.lo = (int)lo;
  t.cnt = (int)cnt;
  t.n0 = (int)n0;
  t.sum = (float)(cnt * d - (all - 2 * neg));
  return t;
}

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

// One output pixel: rows Y of the source, columns X, from p = the byte of (row Y.lo, column X.lo,
// channel 0); row_bytes to the next source row.
template <typename Row>
__device__ __forceinline__ void resample_pixel(const Taps& Y, const Taps& X, int dy, int dx, int stepy, int stepx, Row row,
                                               float val[3]) {
  float acc[3] = {0.f, 0.f, 0.f};
  int ny = Y.n0;
  for (int jy = 0; jy < Y.cnt; ++jy, ny += stepy) {
    const float wy = (float)(dy - iabs(ny));
    const uint8_t* p = row(Y.lo + jy);
    float h[3] = {0.f, 0.f, 0.f};
    int nx = X.n0;
    for (int jx = 0; jx < X.cnt; ++jx, nx += stepx, p += 3) {
      const float wx = (float)(dx - iabs(nx));
      h[0] = __builtin_fmaf(wx, (float)p[0], h[0]);
      h[1] = __builtin_fmaf(wx, (float)p[1], h[1]);
      h[2] = __builtin_fmaf(wx, (float)p[2], h[2]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = __builtin_fmaf(wy, h[c] / X.sum, acc[c]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) val[c] = acc[c] / Y.sum;
}

struct Float3 {
  float v[3];
};

// One tile of one table row, for both kernels: `image` is the row's (Hs, Ws, 3) source, whose first byte
// and whose end are all the staging knows of the memory around it; the caller has checked the row.
template <int kKind>
__device__ __forceinline__ void resample_tile(const uint8_t* __restrict__ image, int Hs, int Ws, int oy, int ox, int bh, int bw,
                                              int flip, int dst, int oh, int ow, const Float3& scale, const Float3& bias,
                                              void* __restrict__ out, int tiles_x) {
  __shared__ Taps ytab[kTH], xtab[kTW];
  __shared__ uint32_t stage[kStageDwords];
  __shared__ float otile[kKind == NIC_RESAMPLE_F32 ? 1 : 3 * kTH * kTW];

  const int t = threadIdx.x;
  const int Y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kTH, X0 = (int)(blockIdx.x % (unsigned)tiles_x) * kTW;
  const int th = oh - Y0 < kTH ? oh - Y0 : kTH, tw = ow - X0 < kTW ? ow - X0 : kTW;  // the tile's valid part, both >= 1

  if (t < th) {
    ytab[t] = axis_taps(bh, oh, Y0 + t);
  } else if (t >= kTH && t < kTH + tw) {
    const int xo = X0 + t - kTH;
    xtab[t - kTH] = axis_taps(bw, ow, flip ? ow - 1 - xo : xo);
  }
  __syncthreads();

  // the source rectangle of the tile, in the box's coordinates: lo and lo + cnt grow with the index,
  // and a flipped tile walks its columns backwards
  const int y_lo = ytab[0].lo, y_hi = ytab[th - 1].lo + ytab[th - 1].cnt;
  const Taps xa = xtab[flip ? tw - 1 : 0], xb = xtab[flip ? 0 : tw - 1];
  const int x_lo = xa.lo, x_hi = xb.lo + xb.cnt;
  const int nrows = y_hi - y_lo, ncols = x_hi - x_lo;
  const long long pitch = (3ll * ncols + 3) / 4 + 1;  // dwords: a row's bytes and the up to 3 before its first
  const bool staged = (long long)nrows * pitch <= kStageDwords;
  const size_t row_bytes = 3 * (size_t)Ws;
  const uint8_t* first = image + (size_t)(oy + y_lo) * row_bytes + 3 * (size_t)(ox + x_lo);  // (y_lo, x_lo) of the box

  if (staged) {
    const uint8_t* image_end = image + (size_t)Hs * row_bytes;
    const int count = nrows * (int)pitch;
    for (int at = t; at < count; at += 256) {
      const int r = at / (int)pitch, k = at - r * (int)pitch;
      const uint8_t* p = first + (size_t)r * row_bytes;
      p = p - ((uintptr_t)p & 3) + 4 * (size_t)k;
      uint32_t word = 0;
      if (p >= image && p + 4 <= image_end) {
        word = *(const uint32_t*)p;
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (p + b >= image && p + b < image_end) word |= (uint32_t)p[b] << (8 * b);
      }
      stage[at] = word;
    }
    __syncthreads();
  }

  const int r = t / kTW, cx = t % kTW;
  const bool mine = r < th && cx < tw;
  float val[3] = {0.f, 0.f, 0.f};
  if (mine) {
    const Taps Y = ytab[r], X = xtab[cx];
    const int dy = 2 * (bh > oh ? bh : oh), dx = 2 * (bw > ow ? bw : ow);
    if (staged) {
      const uint8_t* lds = (const uint8_t*)stage;
      resample_pixel(Y, X, dy, dx, 2 * oh, 2 * ow,
                     [&](int y) {
                       const uintptr_t lead = (uintptr_t)(first + (size_t)(y - y_lo) * row_bytes) & 3;
                       return lds + (size_t)(y - y_lo) * (size_t)pitch * 4 + lead + 3 * (size_t)(X.lo - x_lo);
                     },
                     val);
    } else {
      resample_pixel(Y, X, dy, dx, 2 * oh, 2 * ow,
                     [&](int y) { return first + (size_t)(y - y_lo) * row_bytes + 3 * (size_t)(X.lo - x_lo); }, val);
    }
    if constexpr (kKind == NIC_RESAMPLE_U8) {
#pragma unroll
      for (int c = 0; c < 3; ++c) val[c] = fminf(fmaxf(rintf(val[c]), 0.f), 255.f);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) val[c] = __builtin_fmaf(val[c], scale.v[c], bias.v[c]);
    }
  }

  const size_t plane = (size_t)oh * ow;
  if constexpr (kKind == NIC_RESAMPLE_F32) {
    if (mine) {
      float* o = (float*)out + (size_t)dst * 3 * plane + (size_t)(Y0 + r) * ow + X0 + cx;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * plane] = val[c];
    }
  } else {
#pragma unroll
  for (int c = 0; c < 3; ++c) otile[(c * kTH + r) * kTW + cx] = val[c];
  __syncthreads();
  if constexpr (kKind == NIC_RESAMPLE_F16) {
    // per plane and tile row a run of tw halves; slot q holds the aligned pair (e & ~1) + 2 q, + 1
    constexpr int kSlots = kTW / 2 + 1;
    __half* o = (__half*)out;
    for (int at = t; at < 3 * kTH * kSlots; at += 256) {
      const int q = at % kSlots, run = at / kSlots, rr = run % kTH, c = run / kTH;
      if (rr >= th) continue;
      const size_t e0 = ((size_t)dst * 3 + c) * plane + (size_t)(Y0 + rr) * ow + X0;  // the run's first element
      const long long xa0 = 2ll * q - (long long)(e0 & 1);                              // the pair's columns in the tile
      const float* v = otile + (c * kTH + rr) * kTW;
      const bool a = xa0 >= 0 && xa0 < tw, b = xa0 + 1 >= 0 && xa0 + 1 < tw;
      if (a && b) {
        *(__half2*)(o + e0 + xa0) = __halves2half2(__float2half_rn(v[xa0]), __float2half_rn(v[xa0 + 1]));
      } else if (a) {
        o[e0 + xa0] = __float2half_rn(v[xa0]);
      } else if (b) {
        o[e0 + xa0 + 1] = __float2half_rn(v[xa0 + 1]);
      }
    }
  } else {
    // per tile row a run of 3 tw bytes of the NHWC output; slot q holds the aligned dword (b0 & ~3) + 4 q
    constexpr int kSlots = (3 * kTW + 3) / 4 + 1;
    uint8_t* o = (uint8_t*)out;
    for (int at = t; at < kTH * kSlots; at += 256) {
      const int q = at % kSlots, rr = at / kSlots;
      if (rr >= th) continue;
      const size_t b0 = (((size_t)dst * oh + (Y0 + rr)) * ow + X0) * 3;  // the run's first byte
      const long long k0 = 4ll * q - (long long)(b0 & 3);                 // the dword's bytes in the run
      uint32_t word = 0;
      int inside = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const long long k = k0 + b;
        if (k >= 0 && k < 3ll * tw) {
          const int x = (int)k / 3, c = (int)k - 3 * x;
          word |= (uint32_t)otile[(c * kTH + rr) * kTW + x] << (8 * b);
          ++inside;
        }
      }
      if (inside == 4) {
        *(uint32_t*)(o + b0 + k0) = word;
      } else if (inside) {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (k0 + b >= 0 && k0 + b < 3ll * tw) o[b0 + k0 + b] = (uint8_t)(word >> (8 * b));
      }
    }
  }
  }
}

// Sources of one shape, stacked: row i of the table is a box of image i.
template <int kKind>
__global__ __launch_bounds__(256) void resample_boxes(const uint8_t* __restrict__ src, int Hs, int Ws,
                                                       const int* __restrict__ table, int oh, int ow, int n_out, Float3 scale,
                                                       Float3 bias, void* __restrict__ out, int tiles_x) {
  const int img = blockIdx.y;
  const int* row6 = table + 6 * (size_t)img;
  const int oy = row6[0], ox = row6[1], bh = row6[2], bw = row6[3], flip = row6[4], dst = row6[5];
  // the table is the device's: a row the kernel may not act on stores nothing
  if (bh < 1 || bw < 1 || oy < 0 || ox < 0 || (long long)oy + bh > Hs || (long long)ox + bw > Ws || (flip != 0 && flip != 1) ||
      dst < 0 || dst >= n_out)
    return;
  resample_tile<kKind>(src + (size_t)img * Hs * (3 * (size_t)Ws), Hs, Ws, oy, ox, bh, bw, flip, dst, oh, ow, scale, bias, out,
                       tiles_x);
}

// Sources of any shapes, packed into one pool: row i of the table names its image by offset and shape
// (nic.h, nic_resample_ragged).  Every field is a 64-bit integer of the device's, so every comparison
// below is made where it cannot overflow, and only a row that passes all of them is narrowed to int.
template <int kKind>
__global__ __launch_bounds__(256) void resample_ragged(const uint8_t* __restrict__ pool, long long pool_bytes,
                                                        const long long* __restrict__ table, int oh, int ow, int n_out,
                                                        Float3 scale, Float3 bias, void* __restrict__ out, int tiles_x) {
  const long long* row8 = table + 8 * (size_t)blockIdx.y;
  const long long offset = row8[0], Hs = row8[1], Ws = row8[2], oy = row8[3], ox = row8[4], bh = row8[5], bw = row8[6];
  const long long flip = row8[7] >> 32;
  const int dst = (int)(uint32_t)row8[7];
  if (offset < 0 || (offset & 3) || offset > pool_bytes) return;
  if (Hs < 1 || Ws < 1 || Hs > kMaxPixels || Ws > kMaxPixels || Hs * Ws > kMaxPixels) return;
  if (3 * Hs * Ws > pool_bytes - offset) return;
  if (bh < 1 || bw < 1 || oy < 0 || ox < 0 || oy > Hs - bh || ox > Ws - bw) return;
  if ((flip != 0 && flip != 1) || dst < 0 || dst >= n_out) return;
  resample_tile<kKind>(pool + offset, (int)Hs, (int)Ws, (int)oy, (int)ox, (int)bh, (int)bw, (int)flip, dst, oh, ow, scale, bias, out,
                       tiles_x);
}

}  // namespace

hipError_t launch_resample_boxes(const uint8_t* images, int n, int Hs, int Ws, const int* table, int oh, int ow, int n_out,
                                 int out_kind, const float* scale3, const float* bias3, void* out, hipStream_t st) {
  const int tiles_x = (ow + kTW - 1) / kTW, tiles_y = (oh + kTH - 1) / kTH;
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)n);
  Float3 s{{1.f, 1.f, 1.f}}, b{{0.f, 0.f, 0.f}};
  if (out_kind != NIC_RESAMPLE_U8)
    for (int c = 0; c < 3; ++c) s.v[c] = scale3[c], b.v[c] = bias3[c];
  switch (out_kind) {
    case NIC_RESAMPLE_F32: resample_boxes<NIC_RESAMPLE_F32><<<grid, 256, 0, st>>>(images, Hs, Ws, table, oh, ow, n_out, s, b, out, tiles_x); break;
    case NIC_RESAMPLE_F16: resample_boxes<NIC_RESAMPLE_F16><<<grid, 256, 0, st>>>(images, Hs, Ws, table, oh, ow, n_out, s, b, out, tiles_x); break;
    case NIC_RESAMPLE_U8: resample_boxes<NIC_RESAMPLE_U8><<<grid, 256, 0, st>>>(images, Hs, Ws, table, oh, ow, n_out, s, b, out, tiles_x); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_resample_ragged(const uint8_t* pool, long long pool_bytes, int n, const long long* table, int oh, int ow,
                                  int n_out, int out_kind, const float* scale3, const float* bias3, void* out, hipStream_t st) {
  const int tiles_x = (ow + kTW - 1) / kTW, tiles_y = (oh + kTH - 1) / kTH;
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)n);
  Float3 s{{1.f, 1.f, 1.f}}, b{{0.f, 0.f, 0.f}};
  if (out_kind != NIC_RESAMPLE_U8)
    for (int c = 0; c < 3; ++c) s.v[c] = scale3[c], b.v[c] = bias3[c];
  switch (out_kind) {
    case NIC_RESAMPLE_F32: resample_ragged<NIC_RESAMPLE_F32><<<grid, 256, 0, st>>>(pool, pool_bytes, table, oh, ow, n_out, s, b, out, tiles_x); break;
    case NIC_RESAMPLE_F16: resample_ragged<NIC_RESAMPLE_F16><<<grid, 256, 0, st>>>(pool, pool_bytes, table, oh, ow, n_out, s, b, out, tiles_x); break;
    case NIC_RESAMPLE_U8: resample_ragged<NIC_RESAMPLE_U8><<<grid, 256, 0, st>>>(pool, pool_bytes, table, oh, ow, n_out, s, b, out, tiles_x); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace nic
