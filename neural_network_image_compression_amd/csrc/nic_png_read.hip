// The device PNG reader: the zlib streams of PNG files (their concatenated IDAT payloads, cut out and
// CRC-checked on the host by nic_png_inspect) inflated, Adler-checked and unfiltered on the device
// (format and measurements: DESIGN.md "The device PNG reader"; entry points: include/nic.h
// nic_png_device_read*).
//
// png_inflate (one wave per image): every lane runs nic_inflate.h's inflate_stream on the same values,
// so control flow is wave-uniform and nothing diverges; the lanes differ only where work is shared:
// staging the input through an LDS ring, building the lookup tables, match and stored-block copies.
// The last 32 KB of output live in an LDS ring (the source of every match); every output byte also
// goes to the image's filtered stream in the workspace.
// png_unfilter (one wave per image): the Adler-32 of the filtered stream as per-lane sums, then the
// rows as a skewed wavefront: lane l holds row 64 k + l and is l pixels behind lane 0, so the pixel
// above and above-left arrive from lane l - 1 by a shuffle and the pixel to the left is the lane's own
// previous result.  All five filters run through the one loop.
//
// Untrusted bytes: every index is checked in nic_inflate.h before the Env below is called, and the Env
// clamps again: input reads to the stream's size, window indices by mask, stores to the image's own
// workspace.  No wave waits for another; a block is one wave.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nic.h"
#include "nic_inflate.h"
#include "nic_kernels.h"

namespace nic {

namespace {

constexpr int kWin = 32768;     // deflate's window
constexpr int kInRing = 2048;   // staged input bytes
constexpr int kMaxRow = 16384;  // bytes of a row (w * channels)

struct WaveEnv {
  const uint8_t* in;   // the stream
  uint32_t size;       // its bytes
  uint8_t* out;        // the image's filtered stream in the workspace
  uint32_t T;          // its bytes
  uint8_t* win;        // LDS: kWin
  uint8_t* ring;       // LDS: kInRing
  uint32_t staged_hi;  // ring holds input [staged_hi - kInRing, staged_hi)
  int ln;

  __device__ int lane() const { return ln; }
  __device__ int lanes() const { return 64; }
  __device__ void sync() const { __syncthreads(); }
  __device__ uint32_t in_byte(uint32_t pos) {
    if (pos >= staged_hi) {  // wave-uniform: pos is
      // 64 bytes of history stay staged: after a stored block's LEN / NLEN, and for the Adler-32, the
      // reader steps back over the up to 8 bytes it had buffered
      const uint32_t base = pos >= 64u ? pos - 64u : 0u;
      __syncthreads();
      for (int k = 0; k < kInRing / 64; ++k) {
        const uint32_t o = base + (uint32_t)(k * 64 + ln);
        ring[o & (kInRing - 1)] = (o >= base && o < size) ? in[o] : (uint8_t)0;
      }
      staged_hi = base + kInRing;
      __syncthreads();
    }
    return ring[pos & (kInRing - 1)];
  }
  __device__ void put(uint32_t at, uint32_t byte) {
    if (ln == 0 && at < T) {
      win[at & (kWin - 1)] = (uint8_t)byte;
      out[at] = (uint8_t)byte;
    }
  }
  // For dist > kWin - len a match's source slots are ring slots its own destination overwrites (lane i
  // reads what index i + kWin - dist stores; at dist = kWin both are one slot): right only because the
  // wave loads every lane's byte of a trip before any lane stores, and a later trip's stores come after
  // (tests/test_gpu_png_read.py::test_edge_streams_are_read_as_pillow_reads_them[far] holds it).
  __device__ void copy_match(uint32_t at, uint32_t dist, uint32_t len) {
    __syncthreads();
    if (dist == 0 || dist > at || len > 258u || at > T || len > T - at) return;
    for (uint32_t i = (uint32_t)ln; i < len; i += 64u) {
      const uint32_t src = at - dist + (dist < len ? i % dist : i);
      const uint8_t v = win[src & (kWin - 1)];
      win[(at + i) & (kWin - 1)] = v;
      out[at + i] = v;
    }
    __syncthreads();
  }
  __device__ void copy_stored(uint32_t at, uint32_t pos, uint32_t len) {
    __syncthreads();
    if (len > 65535u || pos > size || len > size - pos || at > T || len > T - at) return;
    for (uint32_t i = (uint32_t)ln; i < len; i += 64u) {
      const uint8_t v = in[pos + i];
      win[(at + i) & (kWin - 1)] = v;
      out[at + i] = v;
    }
    __syncthreads();
  }
};

__device__ __forceinline__ uint32_t clamp_size(long long s, long long stride) {
  s = s < 0 ? 0 : s;
  s = s > stride ? stride : s;
  return (uint32_t)(s > 0x7fffffffll ? 0x7fffffffll : s);
}

// ---- 1: inflate.  grid (n), block 64 ---------------------------------------------------------------
__global__ __launch_bounds__(64) void png_inflate(const uint8_t* __restrict__ streams, long long stride,
                                                  const long long* __restrict__ sizes, uint32_t T, uint8_t* __restrict__ filt,
                                                  size_t fstride, uint32_t* __restrict__ meta) {
  __shared__ uint8_t win[kWin];
  __shared__ uint8_t ring[kInRing];
  __shared__ inflate::Huff lit, dst;
  __shared__ uint8_t lens[inflate::kLensSize];
  const int img = blockIdx.x;
  WaveEnv env;
  env.in = streams + (size_t)img * (size_t)stride;
  env.size = clamp_size(sizes[img], stride);
  env.out = filt + (size_t)img * fstride;
  env.T = T;
  env.win = win;
  env.ring = ring;
  env.staged_hi = 0;
  env.ln = threadIdx.x;
  uint32_t adler = 0;
  const int status = inflate::inflate_stream(env, lit, dst, lens, env.size, T, &adler, nullptr);
  if (threadIdx.x == 0) {
    meta[2 * img + 0] = (uint32_t)status;
    meta[2 * img + 1] = adler;
  }
}

// ---- 2: Adler-32 and unfilter.  grid (n), block 64 ------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ uint32_t wave_sum_mod(unsigned long long v) {
  uint32_t r = (uint32_t)(v % 65521ull);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o, 64);
  return r % 65521u;  // 64 * 65520 < 2^32
}

__global__ __launch_bounds__(64) void png_unfilter(const uint8_t* __restrict__ filt, size_t fstride, uint32_t T, int h, int w, int bpp,
                                                   const uint32_t* __restrict__ meta, uint8_t* __restrict__ images,
                                                   int* __restrict__ status) {
  __shared__ uint8_t uprow[2][kMaxRow];  // the last row of the band before this one, and of this one
  const int img = blockIdx.x, lane = threadIdx.x;
  const uint8_t* f = filt + (size_t)img * fstride;
  int st = (int)meta[2 * img];
  if (st) {  // wave-uniform
    if (lane == 0) status[img] = st;
    return;
  }
  // Adler-32: s1 = sum of bytes, s2 = sum of (T - i) * byte[i]; a lane adds at most T / 64 + 1 terms
  // below 2^38 each, T <= 2^30: no overflow of 64 bits
  unsigned long long s1 = 0, s2 = 0;
  for (uint32_t i = (uint32_t)lane; i < T; i += 64u) {
    const uint32_t v = f[i];
    s1 += v;
    s2 += (unsigned long long)(T - i) * v;
  }
  if (inflate::adler_from_sums(wave_sum_mod(s1), wave_sum_mod(s2), T) != meta[2 * img + 1]) {
    if (lane == 0) status[img] = inflate::kStAdler;
    return;
  }
  const int wb = w * bpp;
  uint8_t* out = images + (size_t)img * (size_t)h * (size_t)wb;
  for (int r0 = 0; r0 < h; r0 += 64) {  // wave-uniform
    const int r = r0 + lane, rows = min(64, h - r0);
    const bool row = lane < rows;
    const uint8_t* src = f + (size_t)(row ? r : r0) * (size_t)(wb + 1);
    int ft = row ? src[0] : 0;
    if (ft > 4) {
      st |= inflate::kStFilter;
      ft = 0;
    }
    uint8_t* dstp = out + (size_t)(row ? r : r0) * (size_t)wb;
    const uint8_t* upr = uprow[(r0 >> 6) & 1];  // written by lane 63 of the band before
    uint8_t* upn = uprow[((r0 >> 6) + 1) & 1];
    uint32_t prev1 = 0, prev2 = 0;  // this lane's pixels of the last two steps (0 while outside its row)
    const int steps = w + rows - 1;
    for (int t = 0; t < steps; ++t) {  // wave-uniform
      const int x = t - lane;
      const bool on = row && x >= 0 && x < w;
      uint32_t up = __shfl_up(prev1, 1, 64), upl = __shfl_up(prev2, 1, 64);
      if (lane == 0) {
        up = upl = 0;
        if (on && r0 > 0)
          for (int c = 0; c < bpp; ++c) {
            up |= (uint32_t)upr[(x * bpp + c) & (kMaxRow - 1)] << (8 * c);
            if (x > 0) upl |= (uint32_t)upr[((x - 1) * bpp + c) & (kMaxRow - 1)] << (8 * c);
          }
      }
      uint32_t cur = 0;
      if (on) {
        for (int c = 0; c < bpp; ++c) {
          const int raw = src[1 + x * bpp + c];
          const int a = (prev1 >> (8 * c)) & 255, b = (up >> (8 * c)) & 255, cc = (upl >> (8 * c)) & 255;
          const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? ((a + b) >> 1) : paeth(a, b, cc);
          const uint32_t v = (uint32_t)(raw + pred) & 255u;
          cur |= v << (8 * c);
          dstp[x * bpp + c] = (uint8_t)v;
          if (lane == 63) upn[(x * bpp + c) & (kMaxRow - 1)] = (uint8_t)v;  // the row above the next band
        }
      }
      prev2 = prev1;
      prev1 = cur;
    }
    __syncthreads();  // lane 63's row is whole before lane 0 of the next band reads it
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) st |= __shfl_xor(st, o, 64);
  if (lane == 0) status[img] = st;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

void png_read_plan(int n, int h, int w, int channels, PngReadPlan* pl) {
  const size_t N = (size_t)n;
  pl->total = (uint32_t)((size_t)h * ((size_t)w * channels + 1));
  pl->fstride = align256((size_t)pl->total + 16);
  pl->filt = 0;
  pl->meta = align256(N * pl->fstride);
  pl->bytes = pl->meta + align256(N * 2 * 4);
}

hipError_t launch_png_dev_read(const uint8_t* streams, long long stride, const long long* sizes, int n, int h, int w, int channels,
                               char* ws, const PngReadPlan& pl, uint8_t* images, int* status, hipStream_t st) {
  uint8_t* filt = (uint8_t*)(ws + pl.filt);
  uint32_t* meta = (uint32_t*)(ws + pl.meta);
  png_inflate<<<dim3(n), 64, 0, st>>>(streams, stride, sizes, pl.total, filt, pl.fstride, meta);
  png_unfilter<<<dim3(n), 64, 0, st>>>(filt, pl.fstride, pl.total, h, w, channels, meta, images, status);
  return hipGetLastError();
}

}  // namespace nic
