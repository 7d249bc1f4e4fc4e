// The .nic container (version 1): a static per-channel byte-wise rANS bitstream, coded and
// decoded on the device (format: DESIGN.md "The .nic container"; entry points: include/nic.h
// nic_rans_*).  One file per image:
//   header 16 B | 96 channel tables | nseg u32 segment lengths | the segments' bytes
// Segment k codes the latent bytes [k K, min((k+1) K, 96 h8 w8)), K = 96 seg_pixels, in NHWC
// order; the byte at offset j is a symbol of channel j % 96.  One lane codes one segment, so
// every lane of a wave is at the same channel at the same time and reads the same table row.
//
// Encode: rans_hist (96 histograms per image) -> rans_normalise (12-bit tables, their file
// bytes and cumulative rows) -> rans_encode_segments (each lane walks its segment backwards
// and writes backwards into its own worst-case region of the scratch) -> rans_layout (prefix
// sums of table and segment lengths, file sizes) -> rans_assemble (header, tables, segment
// table and payload into out + i * stride).
// Decode: rans_parse (header check, tables -> cumulative rows, segment offsets; all on the
// device) -> rans_decode_segments (binary search of the LDS cumulative row per slot).
//
// Versions 2 (a codec-level prior) and 3 (a context prior: three rows per channel, chosen by the
// left neighbour) run the same kernels: every kernel that differs between versions is one template,
// over the version (rans_parse, rans_layout, rans_assemble) or over the rows of an image (Rows<>:
// rans_tables, rans_encode_segments, rans_decode_segments), instantiated per case.
// Region decode runs the same parse and segment kernel over a latent window: one window for every
// file of the call, or (batched region decode) a window of one shape at each file's own place in its
// own frame, from a per-file table on the device; cut_boxes then cuts each image's pixel box.

#include <hip/hip_runtime.h>

#include <zlib.h>

#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/nic.h"
#include "nic_kernels.h"

namespace nic {

namespace {

constexpr int kCh = 96;                  // latent channels
constexpr int kProbBits = 12;
constexpr uint32_t kProbScale = 1u << kProbBits;
constexpr uint32_t kRansL = 1u << 23;    // lower bound of the normalised state interval
constexpr int kCumRow = 257;             // start[0..256] of one channel
constexpr int kCumWords = kCh * kCumRow; // u16 per image (49,344 B: the LDS table)
constexpr int kTabRow = 772;             // >= 1 + 3 * 256 file bytes of one channel's table
constexpr int kHeader = 16;
constexpr int kHeader2 = 40;             // versions 2 and 3: + u32 H, u32 W, u32 prior_id, 12-byte channel mask

// Version 3's row pitch in LDS: all 64 lanes are at one channel, spread over its three rows, and most
// of them at symbols near the anchor.  At 257 u16 (128.5 dwords) the same symbol of the three rows
// falls onto one or two neighbouring banks; at 278 u16 (139 dwords = 4 x 32 + 11) the rows sit 11
// and 22 banks apart.  288 rows x 556 B = 160,128 B of the 163,840.
constexpr int kCtx = 3;
constexpr int kCtxRow = 278;
constexpr int kCtxWords = kCh * kCtx * kCtxRow;  // u16 per image
static_assert(kCtxRow % 2 == 0 && kCtxRow >= kCumRow && kCtxWords * 2 + 64 <= 160 * 1024, "the rows must fit the LDS");

// The cumulative rows of one image, u16[96][kPerCh][kPitch] in global memory and in LDS alike:
// one row per channel (versions 1 and 2) or one per (channel, context) (version 3).
template <bool kContext>
struct Rows {
  static constexpr int kPerCh = kContext ? kCtx : 1;
  static constexpr int kPitch = kContext ? kCtxRow : kCumRow;
  static constexpr int kWords = kContext ? kCtxWords : kCumWords;
  // channel ch's row of context k (k = 0 without contexts)
  __device__ static const uint16_t* row(const uint16_t* rows, int ch, uint32_t k) { return rows + (ch * kPerCh + k) * kPitch; }
};

// the image's rows into LDS as dwords (kWords is even and every image's rows start 4-B aligned; the
// pad of a version-3 row is copied, never read)
template <class R>
__device__ __forceinline__ void load_rows(uint16_t* lds, const uint16_t* __restrict__ src, int tid, int nthreads) {
  const uint32_t* s = (const uint32_t*)src;
  uint32_t* d = (uint32_t*)lds;
  for (int i = tid; i < R::kWords / 2; i += nthreads) d[i] = s[i];
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
// exclusive prefix sum over the 64 lanes
__device__ __forceinline__ uint32_t wave_excl(uint32_t v, int lane) {
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  return inc - v;
}

// ---- encode 1: per-image, per-channel counts ----------------------------------------------
// grid (ceil(npix / 256), 3, n), block 256: thread = pixel, blockIdx.y = a third of the channels
// (32 LDS histograms = 32 KB); each thread reads its pixel's 32 bytes as two 16-B loads.
// T = uint32_t: per-image counts [n][96][256] (img_stride = 96 * 256); T = unsigned long long: the
// prior's one accumulator [96][256] (img_stride = 0), added into with 64-bit integer atomics, so the
// totals do not depend on the order and accumulate across calls.
template <typename T>
__global__ __launch_bounds__(256) void rans_hist(const uint8_t* __restrict__ z, int npix, T* __restrict__ counts,
                                                  size_t img_stride) {
  __shared__ uint32_t h[32 * 256];
  const int tid = threadIdx.x, third = blockIdx.y, img = blockIdx.z;
  for (int i = tid; i < 32 * 256; i += 256) h[i] = 0;
  __syncthreads();
  const int p = blockIdx.x * 256 + tid;
  if (p < npix) {
    const uint4* src = (const uint4*)(z + ((size_t)img * npix + p) * kCh + 32 * third);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const uint4 v = src[q];
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int b = 0; b < 16; ++b) atomicAdd(&h[(16 * q + b) * 256 + ((w[b >> 2] >> (8 * (b & 3))) & 255u)], 1u);
    }
  }
  __syncthreads();
  T* dst = counts + (size_t)img * img_stride + (size_t)(32 * third) * 256;
  for (int i = tid; i < 32 * 256; i += 256)
    if (h[i]) atomicAdd(&dst[i], (T)h[i]);
}

// ---- encode 2: 12-bit tables ---------------------------------------------------------------
// grid (96, n), block 64: one wave per channel, lane l owns symbols 4l..4l+3.
//   f = max(1, floor(c 4096 / N)) for every used symbol; a deficit goes onto the largest entry;
//   a surplus (at most 255, from the floor-to-zero bumps) is taken one at a time from the
//   currently largest entry (lowest symbol on ties), which never takes an entry below 1.
// Writes the channel's cumulative row start[0..256], its file bytes and their count.
// The steps are device functions of the whole wave, shared with rans_tables.

// lane l's four counts -> its four freqs (0 for an unused symbol) and how many it uses
__device__ __forceinline__ void normalise_own(const uint32_t cnt[4], int npix, int lane, uint32_t f[4], uint32_t& used) {
  uint32_t sum = 0;
  used = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[k] = 0;
    if (cnt[k]) {
      const uint32_t q = (uint32_t)(((unsigned long long)cnt[k] << kProbBits) / (unsigned long long)npix);
      f[k] = q ? q : 1u;
      ++used;
    }
    sum += f[k];
  }
  sum = wave_sum(sum);
  int diff = (int)kProbScale - (int)sum;
  // (f << 8) | (255 - s): the largest f, the lowest symbol on ties
  auto best = [&]() {
    uint32_t key = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t kk = (f[k] << 8) | (uint32_t)(255 - (4 * lane + k));
      key = kk > key ? kk : key;
    }
    return wave_max(key);
  };
  if (diff > 0) {
    const int s = 255 - (int)(best() & 255u);
    if ((s >> 2) == lane) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k == (s & 3)) f[k] += (uint32_t)diff;
    }
  }
  for (; diff < 0; ++diff) {  // wave-uniform trip count, at most 255
    const int s = 255 - (int)(best() & 255u);
    if ((s >> 2) == lane) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k == (s & 3)) f[k] -= 1u;
    }
  }
}

// The channel's table as the file stores it (u8 n-1, n x (u8 symbol, u16 freq)) and its length.
__device__ __forceinline__ void write_table(const uint32_t f[4], uint32_t used, int lane, uint8_t* __restrict__ trow,
                                            uint32_t* __restrict__ tablen_row) {
  uint32_t idx = wave_excl(used, lane);
  const uint32_t nsym = wave_sum(used);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (f[k]) {
      uint8_t* e = trow + 1 + 3 * idx;
      e[0] = (uint8_t)(4 * lane + k);
      e[1] = (uint8_t)(f[k] & 255u);
      e[2] = (uint8_t)(f[k] >> 8);
      ++idx;
    }
  if (lane == 0) {
    trow[0] = (uint8_t)(nsym - 1);
    *tablen_row = 1 + 3 * nsym;
  }
}

// The channel's cumulative row start[0..256] from the lanes' freqs.
__device__ __forceinline__ void write_cum(const uint32_t f[4], int lane, uint16_t* __restrict__ crow) {
  uint32_t run = wave_excl(f[0] + f[1] + f[2] + f[3], lane);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    crow[4 * lane + k] = (uint16_t)run;
    run += f[k];
  }
  if (lane == 63) crow[256] = (uint16_t)run;  // 4096
}

__global__ __launch_bounds__(64) void rans_normalise(const uint32_t* __restrict__ counts, int npix, uint16_t* __restrict__ cum,
                                                      uint8_t* __restrict__ tab, uint32_t* __restrict__ tablen) {
  const int lane = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
  const size_t row = (size_t)img * kCh + c;
  const uint4 cv = ((const uint4*)(counts + row * 256))[lane];
  const uint32_t cnt[4] = {cv.x, cv.y, cv.z, cv.w};
  uint32_t f[4], used;
  normalise_own(cnt, npix, lane, f, used);
  write_cum(f, lane, cum + row * kCumRow);
  write_table(f, used, lane, tab + row * kTabRow, tablen + row);
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// ---- encode 2, versions 2 and 3: tables and the per-channel choice.  grid (96, n), block 64 -----
// The prior is 96 x kPerCh x 256 freqs in 1..4096, every row summing to 4096, fitted once over a
// corpus and shared by every file.  A file stores a table only for the channels whose own table
// pays for itself; the others are coded with the prior's row(s).
// counts: the image's [96][kPerCh][256]; their sum over the contexts is version 1's histogram and
// is normalised by version 1's rule.  With cost16[f] = round((12 - log2 f) 2^16):
//   own = sum c cost16[f_own] + (8 (1 + 3 n) << 16),  prior = sum over rows k of c_k cost16[f_prior[k]]   (u64)
// The channel keeps its own table iff own < prior.  Writes the channel's kPerCh cumulative rows (the
// prior's, or its own row in every context), the table's file bytes and their length (0 for a prior
// channel) and keep[].
template <bool kContext>
__global__ __launch_bounds__(64) void rans_tables(const uint32_t* __restrict__ counts, int npix,
                                                   const uint16_t* __restrict__ prior_freq,
                                                   const uint16_t* __restrict__ prior_cum, const uint32_t* __restrict__ cost16,
                                                   uint16_t* __restrict__ cum, uint8_t* __restrict__ tab,
                                                   uint32_t* __restrict__ tablen, uint32_t* __restrict__ keep) {
  using R = Rows<kContext>;
  const int lane = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
  const size_t row = (size_t)img * kCh + c;
  uint32_t cnt[4] = {0, 0, 0, 0};
  unsigned long long pri = 0;
#pragma unroll
  for (int k = 0; k < R::kPerCh; ++k) {
    const uint4 cv = ((const uint4*)(counts + (row * R::kPerCh + k) * 256))[lane];
    const uint32_t ck[4] = {cv.x, cv.y, cv.z, cv.w};
    const uint2 pv = ((const uint2*)(prior_freq + ((size_t)c * R::kPerCh + k) * 256))[lane];  // each in 1..4096 (checked on upload)
    const uint32_t pf[4] = {pv.x & 0xffffu, pv.x >> 16, pv.y & 0xffffu, pv.y >> 16};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cnt[j] += ck[j];
      pri += (unsigned long long)ck[j] * cost16[min(pf[j], kProbScale)];
    }
  }
  uint32_t f[4], used;
  normalise_own(cnt, npix, lane, f, used);
  unsigned long long own = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) own += (unsigned long long)cnt[j] * cost16[f[j]];  // f <= 4096; cost16[0] = 0 (and c = 0 there)
  const uint32_t nsym = wave_sum(used);
  own = wave_sum64(own) + ((unsigned long long)(8u * (1u + 3u * nsym)) << 16);
  pri = wave_sum64(pri);
  uint16_t* crow = cum + (size_t)img * R::kWords + (size_t)c * R::kPerCh * R::kPitch;
  if (own < pri) {  // wave-uniform
#pragma unroll
    for (int k = 0; k < R::kPerCh; ++k) write_cum(f, lane, crow + k * R::kPitch);
    write_table(f, used, lane, tab + row * kTabRow, tablen + row);
    if (lane == 0) keep[row] = 1u;
  } else {
    const uint16_t* prow = prior_cum + (size_t)c * R::kPerCh * R::kPitch;
#pragma unroll
    for (int k = 0; k < R::kPerCh; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) crow[k * R::kPitch + 4 * lane + j] = prow[k * R::kPitch + 4 * lane + j];
      if (lane == 63) crow[k * R::kPitch + 256] = prow[k * R::kPitch + 256];
    }
    if (lane == 0) {
      tablen[row] = 0u;
      keep[row] = 0u;
    }
  }
}

// Version 3's context of a byte: the byte at segment-relative offset j (channel c = j % 96) is coded
// under row (c, k), k = 0 for the segment's first pixel, else min(2, |z[j - 96] - anchor[c]|).  A
// channel that keeps its own table is coded under it in every context, so the segment kernels always
// see three rows per channel.
__device__ __forceinline__ uint32_t ctx_of(uint32_t left, uint32_t anchor) {
  const int d = (int)left - (int)anchor;
  const uint32_t a = (uint32_t)(d < 0 ? -d : d);
  return a < 2u ? a : 2u;
}

// ---- encode 3: segment coding, one lane per segment -----------------------------------------
// grid (ceil(nseg / 64), n), block 64.  The lane's symbols are read pixel by pixel from the
// last to the first as six per-lane-contiguous 16-B loads (a segment starts at a multiple of
// 96 B); bytes are written backwards from the end of the lane's region of `cap` bytes, so the
// finished segment is region[cap - len, cap).
// kContext: the row is chosen per symbol, so beside the 16 bytes of pixel p the lane loads the same
// 16 bytes of pixel p - 1 (its first pixel has none: context 0); the lanes of the wave are at one
// channel, in up to three rows.  anchor is not read without contexts.
template <bool kContext>
__global__ __launch_bounds__(64) void rans_encode_segments(const uint8_t* __restrict__ z, int npix, int seg_pixels, int nseg,
                                                            const uint16_t* __restrict__ cum,
                                                            const uint8_t* __restrict__ anchor, uint8_t* __restrict__ scratch,
                                                            uint32_t cap, uint32_t* __restrict__ seglen) {
  using R = Rows<kContext>;
  __shared__ uint16_t start[R::kWords];
  const int lane = threadIdx.x, img = blockIdx.y;
  load_rows<R>(start, cum + (size_t)img * R::kWords, lane, 64);
  __syncthreads();
  const int seg = blockIdx.x * 64 + lane;
  const bool live = seg < nseg;
  const int p0 = live ? seg * seg_pixels : 0;
  const int mypix = live ? min(seg_pixels, npix - p0) : 0;
  const uint8_t* src = z + ((size_t)img * npix + p0) * kCh;
  uint8_t* region = scratch + ((size_t)img * nseg + (live ? seg : 0)) * cap;
  uint32_t pos = cap, x = kRansL;
  auto emit = [&](uint32_t b) {
    if (pos > 0) region[--pos] = (uint8_t)b;  // pos > 0 always holds: cap is the worst case
  };
  int maxpix = mypix;  // wave-uniform trip count
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) maxpix = max(maxpix, __shfl_xor(maxpix, o, 64));
  for (int p = maxpix - 1; p >= 0; --p) {
    const bool on = p < mypix;
    for (int q = 5; q >= 0; --q) {
      uint4 v = make_uint4(0, 0, 0, 0), u = make_uint4(0, 0, 0, 0);
      if (on) v = *(const uint4*)(src + (size_t)p * kCh + 16 * q);
      if constexpr (kContext)
        if (on && p > 0) u = *(const uint4*)(src + (size_t)(p - 1) * kCh + 16 * q);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w}, l[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int b = 15; b >= 0; --b) {
        const uint32_t s = (w[b >> 2] >> (8 * (b & 3))) & 255u;
        uint32_t k = 0;
        if constexpr (kContext) k = p > 0 ? ctx_of((l[b >> 2] >> (8 * (b & 3))) & 255u, anchor[16 * q + b]) : 0u;
        const uint16_t* row = R::row(start, 16 * q + b, k);
        const uint32_t lo = row[s], freq = row[s + 1] - lo;
        // freq == 4096: the row's only symbol, x is unchanged and nothing is emitted
        if (on && freq != kProbScale) {
          const uint32_t xmax = freq << 19;
          if (x >= xmax) {
            emit(x & 255u);
            x >>= 8;
            if (x >= xmax) {
              emit(x & 255u);
              x >>= 8;
            }
          }
          const uint32_t qd = x / freq;
          x = (qd << kProbBits) + (x - qd * freq) + lo;
        }
      }
    }
  }
  if (live) {
    emit(x & 255u);
    emit((x >> 8) & 255u);
    emit((x >> 16) & 255u);
    emit(x >> 24);
    seglen[(size_t)img * nseg + seg] = cap - pos;
  }
}

// exclusive prefix sums of len[0..count) into off[0..count] (off[count] = total, saturating at
// `limit`) by one block of 256 threads
__device__ void block_offsets(const uint32_t* __restrict__ len, int count, uint32_t* __restrict__ off, uint32_t limit,
                              uint32_t* sh /* 257 words */) {
  const int tid = threadIdx.x;
  uint32_t carry = 0;
  for (int base = 0; base < count; base += 256) {
    const int i = base + tid;
    const uint32_t v = i < count ? min(len[i], limit) : 0u;
    sh[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const uint32_t t = tid >= o ? sh[tid - o] : 0u;
      __syncthreads();
      sh[tid] = (uint32_t)min((unsigned long long)sh[tid] + t, (unsigned long long)limit);
      __syncthreads();
    }
    const uint32_t incl = (uint32_t)min((unsigned long long)sh[tid] + carry, (unsigned long long)limit);
    if (i < count) off[i] = (uint32_t)min((unsigned long long)(incl - min(incl, v)), (unsigned long long)limit);
    const uint32_t total = (uint32_t)min((unsigned long long)sh[255] + carry, (unsigned long long)limit);
    __syncthreads();
    carry = total;
  }
  if (tid == 0) off[count] = carry;
}

// ---- encode 4a: offsets and file sizes.  grid (n), block 256 --------------------------------
// kVer: the container version, 1, 2 or 3 (2 and 3: a 40-byte header; prior channels have tablen 0)
template <int kVer>
__global__ __launch_bounds__(256) void rans_layout(const uint32_t* __restrict__ tablen, uint32_t* __restrict__ taboff,
                                                    const uint32_t* __restrict__ seglen, uint32_t* __restrict__ segoff, int nseg,
                                                    long long* __restrict__ sizes) {
  __shared__ uint32_t sh[257];
  const int img = blockIdx.x;
  block_offsets(tablen + (size_t)img * kCh, kCh, taboff + (size_t)img * (kCh + 1), 0x7fffffffu, sh);
  __syncthreads();
  block_offsets(seglen + (size_t)img * nseg, nseg, segoff + (size_t)img * (nseg + 1), 0x7fffffffu, sh);
  __syncthreads();
  if (threadIdx.x == 0)
    sizes[img] = (long long)(kVer == 1 ? kHeader : kHeader2) + taboff[(size_t)img * (kCh + 1) + kCh] + 4ll * nseg +
                 segoff[(size_t)img * (nseg + 1) + nseg];
}

// ---- encode 4b: the files.  grid (ceil((96 + nseg) / 4), n), block 256: one wave per item ----
// item c < 96: channel c's table (item 0 also the header); item 96 + k: segment k's length and bytes
// Versions 2 and 3: the header also holds (H, W), prior_id and the mask gathered from keep[96]
// (1: the channel stores its own table); a prior channel's tablen is 0, so nothing is copied for it.
template <int kVer>
__global__ __launch_bounds__(256) void rans_assemble(const uint8_t* __restrict__ tab, const uint32_t* __restrict__ tablen,
                                                      const uint32_t* __restrict__ taboff, const uint8_t* __restrict__ scratch,
                                                      uint32_t cap, const uint32_t* __restrict__ seglen,
                                                      const uint32_t* __restrict__ segoff, int nseg, int seg_pixels, int h8, int w8,
                                                      uint8_t* __restrict__ out, long long stride, uint32_t H, uint32_t W,
                                                      uint32_t prior_id, const uint32_t* __restrict__ keep) {
  constexpr int kHdr = kVer == 1 ? kHeader : kHeader2;
  const int lane = threadIdx.x & 63, item = blockIdx.x * 4 + (threadIdx.x >> 6), img = blockIdx.y;
  if (item >= kCh + nseg) return;
  uint8_t* file = out + (size_t)img * (size_t)stride;
  const uint32_t* toff = taboff + (size_t)img * (kCh + 1);
  if (item < kCh) {
    if (item == 0 && lane < kHdr) {
      const uint32_t hw[5] = {(uint32_t)h8, (uint32_t)w8, H, W, prior_id};
      uint8_t b;
      if (lane < 4) b = (uint8_t)("NICR"[lane]);
      else if (lane == 4) b = (uint8_t)kVer;
      else if (lane == 5) b = (uint8_t)kProbBits;
      else if (lane < 8) b = (uint8_t)(((uint32_t)seg_pixels >> (8 * (lane - 6))) & 255u);
      else if (lane < 28) b = (uint8_t)((hw[(lane - 8) >> 2] >> (8 * (lane & 3))) & 255u);
      else {  // versions 2 and 3 only: channel c is bit c & 7 of mask byte c >> 3
        const uint32_t* k8 = keep + (size_t)img * kCh + 8 * (lane - 28);
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) m |= (k8[j] ? 1u : 0u) << j;
        b = (uint8_t)m;
      }
      file[lane] = b;
    }
    const size_t row = (size_t)img * kCh + item;
    const uint8_t* src = tab + row * kTabRow;
    uint8_t* dst = file + kHdr + toff[item];
    for (uint32_t i = lane; i < tablen[row]; i += 64) dst[i] = src[i];  // < 16 + 96 * 769 <= stride
    return;
  }
  const int k = item - kCh;
  const uint32_t len = seglen[(size_t)img * nseg + k];
  uint8_t* segtab = file + kHdr + toff[kCh];
  if (lane < 4) segtab[4 * k + lane] = (uint8_t)((len >> (8 * lane)) & 255u);
  const uint8_t* src = scratch + ((size_t)img * nseg + k) * cap + (cap - len);
  // stride >= nic_rans_bound covers every payload (a file's symbols cost well under 12 bits on
  // average under its own tables); the clamp keeps even a miscounted one inside the image's slot
  const size_t at = (size_t)kHdr + toff[kCh] + 4 * (size_t)nseg + segoff[(size_t)img * (nseg + 1) + k];
  for (uint32_t i = lane; i < len; i += 64)
    if (at + i < (size_t)stride) file[at + i] = src[i];
}

// ---- decode 1: parse, one instantiation per version.  grid (n), block 256 ---------------------
// Every read of a file byte is clamped to [0, size).  meta[img] = {nseg, seg_pixels, payload
// begin, size}.  A header that does not describe an (h8, w8) file of version kVer leaves nseg = 0
// and status 2 (nothing of that image is decoded); versions 2 and 3 (the 40-byte header) must also
// describe an H x W image with h8 = ceil(H / 8), w8 = ceil(W / 8), and their prior_id must be the
// ctx's, else status 8 and nseg = 0 likewise.  A table that breaks the invariants (symbols ascending:
// an entry that does not ascend is never reached, e != nsym; freqs in 1..4096 summing to 4096) sets
// status bit 4 and still yields cumulative rows that resolve every slot (start[0] = 0, non-decreasing,
// start[256] = 4096): the running sum saturates at 4096.  Version 1 stores every channel's table; versions 2 and 3 those of the masked
// channels only, and the other channels' rows are copies of the prior's.  A table is walked once and
// stored into each of the channel's rows (three in version 3).
// wintab (per-file windows, else NULL): row img = (h8, w8, r0, c0) replaces the call's (h8, w8), and
// a row that is no latent of at most maxseg pixels, or whose win_rows x win_cols window at (r0, c0) does not
// lie inside it, is refused like a header of another geometry (status 2, nseg = 0), so what the
// segment kernel reads of a row it acts on has been checked here.
template <int kVer>
__global__ __launch_bounds__(256) void rans_parse(const uint8_t* __restrict__ files, long long stride,
                                                   const long long* __restrict__ sizes, int h8, int w8,
                                                   const int* __restrict__ wintab, int win_rows, int win_cols,
                                                   const uint16_t* __restrict__ prior_cum, uint32_t prior_id,
                                                   uint16_t* __restrict__ cum, uint32_t* __restrict__ seglen,
                                                   uint32_t* __restrict__ segoff, int maxseg, uint32_t* __restrict__ meta,
                                                   int* __restrict__ status) {
  using R = Rows<kVer == 3>;
  constexpr bool kPrior = kVer != 1;
  constexpr uint32_t kHdr = kPrior ? kHeader2 : kHeader;
  __shared__ uint32_t sh[257];
  __shared__ uint32_t choff[kCh + 1];
  __shared__ uint32_t own[kCh];  // versions 2 and 3: the channel stores its table (version 1: all do, own is not used)
  __shared__ int s_bad, s_nseg;
  const int tid = threadIdx.x, img = blockIdx.x;
  const uint8_t* f = files + (size_t)img * (size_t)stride;
  long long sz = sizes[img];
  sz = sz < 0 ? 0 : (sz > stride ? stride : sz);
  sz = sz > 0x7fffffffll ? 0x7fffffffll : sz;
  const uint32_t size = (uint32_t)sz;
  auto rd = [&](uint32_t i) -> uint32_t { return i < size ? (uint32_t)f[i] : 0u; };
  auto rd32 = [&](uint32_t i) -> uint32_t { return rd(i) | (rd(i + 1) << 8) | (rd(i + 2) << 16) | (rd(i + 3) << 24); };
  auto owns = [&](int c) -> bool {
    if constexpr (kPrior) return own[c] != 0u;
    return true;
  };
  bool fits = true;
  if (wintab) {
    const int* t = wintab + 4 * (size_t)img;
    h8 = t[0];
    w8 = t[1];
    fits = h8 > 0 && w8 > 0 && (long long)h8 * w8 <= (long long)maxseg && t[2] >= 0 && t[3] >= 0 &&
           (long long)t[2] + win_rows <= h8 && (long long)t[3] + win_cols <= w8;
  }
  const int npix = fits ? h8 * w8 : 0;
  if (tid == 0) {
    const uint32_t S = rd(6) | (rd(7) << 8), fh = rd32(8), fw = rd32(12);
    bool ok = fits && size >= kHdr && rd(0) == 'N' && rd(1) == 'I' && rd(2) == 'C' && rd(3) == 'R' && rd(4) == (uint32_t)kVer &&
              rd(5) == (uint32_t)kProbBits && S >= 1 && fh == (uint32_t)h8 && fw == (uint32_t)w8;
    bool mine = true;
    if constexpr (kPrior) {
      const uint32_t H = rd32(16), W = rd32(20);
      ok = ok && (H >> 3) + ((H & 7u) != 0u) == fh && (W >> 3) + ((W & 7u) != 0u) == fw;
      mine = rd32(24) == prior_id;
    }
    const int nseg = ok && mine ? (int)(((uint32_t)npix + S - 1) / S) : 0;  // <= npix = maxseg
    uint32_t off = kHdr;
    for (int c = 0; c < kCh; ++c) {
      choff[c] = off;
      if constexpr (kPrior) own[c] = (rd(28 + (c >> 3)) >> (c & 7)) & 1u;
      if (owns(c)) off += 1 + 3 * (rd(off) + 1);  // <= 40 + 96 * 769
    }
    choff[kCh] = off;
    s_nseg = nseg;
    s_bad = !ok ? 2 : (mine ? 0 : 8);
    meta[4 * img + 0] = (uint32_t)nseg;
    meta[4 * img + 1] = ok ? S : 1u;
    meta[4 * img + 2] = min(off + 4u * (uint32_t)nseg, size);
    meta[4 * img + 3] = size;
  }
  __syncthreads();
  const int nseg = s_nseg;
  uint16_t* rows = cum + (size_t)img * R::kWords;
  if (nseg > 0 && tid < kCh && owns(tid)) {
    uint16_t* row = rows + tid * R::kPerCh * R::kPitch;
    const uint32_t base = choff[tid], nsym = rd(base) + 1;
    uint32_t e = 0, run = 0, es = rd(base + 1), ef = rd(base + 2) | (rd(base + 3) << 8);
    bool bad = false;  // a freq outside 1..4096, or a sum past 4096 that the clamp below would hide
    for (uint32_t s = 0; s < 256; ++s) {
#pragma unroll
      for (int k = 0; k < R::kPerCh; ++k) row[k * R::kPitch + s] = (uint16_t)run;
      if (e < nsym && es == s) {
        bad |= ef == 0u || run + ef > kProbScale;  // run <= 4096 and ef < 2^16: no wrap
        run = min(run + ef, kProbScale);
        ++e;
        es = rd(base + 1 + 3 * e);
        ef = rd(base + 2 + 3 * e) | (rd(base + 3 + 3 * e) << 8);
      }
    }
#pragma unroll
    for (int k = 0; k < R::kPerCh; ++k) row[k * R::kPitch + 256] = (uint16_t)kProbScale;
    if (bad || e != nsym || run != kProbScale) atomicOr(&s_bad, 4);
  }
  if constexpr (kPrior) {
    if (nseg > 0)  // the prior's rows (start[0] = 0, non-decreasing, start[256] = 4096 by construction), without a row's pad
      for (int i = tid; i < R::kWords; i += 256)
        if (!own[i / (R::kPerCh * R::kPitch)] && (R::kPitch == kCumRow || i % R::kPitch < kCumRow)) rows[i] = prior_cum[i];
  }
  // the segment table -> clamped lengths -> offsets
  const uint32_t segtab = choff[kCh];
  uint32_t* len = seglen + (size_t)img * maxseg;
  for (int k = tid; k < nseg; k += 256) len[k] = rd32(segtab + 4u * (uint32_t)k);  // < 2^31 + 2^27: no wrap
  __syncthreads();
  block_offsets(len, nseg, segoff + (size_t)img * (maxseg + 1), size, sh);
  __syncthreads();
  if (tid == 0) status[img] = s_bad;
}

// ---- fitting a prior: counts (rans_hist / rans3_hist into one u64 accumulator) -> freqs ---------
// grid (rows), block 64: one wave per row of 256 counts
// (96 channels of the static prior; 96 x 3 (channel, context) rows of the context prior)
// Version 1's rule with all 256 symbols "used": f = max(1, floor(c 4096 / N)); a deficit goes onto
// the largest entry; a surplus (at most 255) is taken one at a time from the currently largest
// entry (lowest symbol on ties).  N = 0: sixteen everywhere.  c 4096 must fit 64 bits: N < 2^52.
__global__ __launch_bounds__(64) void rans_prior_normalise(const unsigned long long* __restrict__ counts,
                                                            uint16_t* __restrict__ freqs) {
  const int lane = threadIdx.x, c = blockIdx.x;
  unsigned long long cnt[4], mine = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cnt[k] = counts[(size_t)c * 256 + 4 * lane + k];
    mine += cnt[k];
  }
  const unsigned long long N = wave_sum64(mine);
  uint32_t f[4], sum = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t q = N ? (uint32_t)((cnt[k] << kProbBits) / N) : 16u;
    f[k] = q ? q : 1u;
    sum += f[k];
  }
  sum = wave_sum(sum);
  int diff = (int)kProbScale - (int)sum;
  auto best = [&]() {  // (f << 8) | (255 - s): the largest f, the lowest symbol on ties
    uint32_t key = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t kk = (f[k] << 8) | (uint32_t)(255 - (4 * lane + k));
      key = kk > key ? kk : key;
    }
    return wave_max(key);
  };
  if (diff > 0) {
    const int s = 255 - (int)(best() & 255u);
    if ((s >> 2) == lane) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k == (s & 3)) f[k] += (uint32_t)diff;
    }
  }
  for (; diff < 0; ++diff) {  // wave-uniform trip count, at most 255; the largest entry stays >= 16
    const int s = 255 - (int)(best() & 255u);
    if ((s >> 2) == lane) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k == (s & 3)) f[k] -= 1u;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) freqs[(size_t)c * 256 + 4 * lane + k] = (uint16_t)f[k];
}

// ---- context counts ---------------------------------------------------------------------------
// grid (ceil(npix / 256), 6, n), block 256: rans_hist's structure with a sixth of the channels per
// block (16 x 3 LDS histograms = 48 KB); a thread reads its pixel's 16 bytes and, unless the pixel
// opens a segment, the 16 bytes of the pixel before it.  T = uint32_t: per-image counts
// [n][96][3][256] (img_stride = 96 * 3 * 256); T = unsigned long long: one corpus accumulator
// (img_stride = 0), integer atomics, so the totals do not depend on the order.
template <typename T>
__global__ __launch_bounds__(256) void rans3_hist(const uint8_t* __restrict__ z, int npix, int seg_pixels,
                                                   const uint8_t* __restrict__ anchor, T* __restrict__ counts,
                                                   size_t img_stride) {
  __shared__ uint32_t h[16 * kCtx * 256];
  const int tid = threadIdx.x, part = blockIdx.y, img = blockIdx.z;
  for (int i = tid; i < 16 * kCtx * 256; i += 256) h[i] = 0;
  __syncthreads();
  const int p = blockIdx.x * 256 + tid;
  if (p < npix) {
    const uint8_t* at = z + ((size_t)img * npix + p) * kCh + 16 * part;
    const bool first = p % seg_pixels == 0;
    const uint4 v = *(const uint4*)at;
    uint4 u = make_uint4(0, 0, 0, 0);
    if (!first) u = *(const uint4*)(at - kCh);  // p >= 1 here
    const uint32_t w[4] = {v.x, v.y, v.z, v.w}, l[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const uint32_t s = (w[b >> 2] >> (8 * (b & 3))) & 255u, left = (l[b >> 2] >> (8 * (b & 3))) & 255u;
      const uint32_t k = first ? 0u : ctx_of(left, anchor[16 * part + b]);
      atomicAdd(&h[(b * kCtx + k) * 256 + s], 1u);
    }
  }
  __syncthreads();
  T* dst = counts + (size_t)img * img_stride + (size_t)(16 * part) * kCtx * 256;
  for (int i = tid; i < 16 * kCtx * 256; i += 256)
    if (h[i]) atomicAdd(&dst[i], (T)h[i]);
}

// ==== window decode: only the segments that hold a pixel of a latent window ("Region
// decode") ====
// The window is the latent pixels (r0 + i, c0 + x), i < rows, x < cols.  Its row i is the run
// [a_i, a_i + cols) of the row-major pixel order, a_i = (r0 + i) w8 + c0, and lies in the segments
// first_i = a_i / S .. last_i = (a_i + cols - 1) / S: at most J = (cols + S - 2) / S + 1 of them.
// Slot (i, j), j < J, stands for segment first_i + j; it is live iff that segment is <= last_i and,
// for i > 0, > last_(i-1) -- a segment that spans several window rows belongs to the first of them.
// A live lane decodes its whole segment (rANS is serial, and the end check needs the last byte) and
// stores only the pixels inside the window, at their place in the compact (n, rows, cols, 96) output.
// (RansWindow: nic_kernels.h)

// Which pixels rans_decode_segments keeps: the whole frame, the call's one window of every file, or a
// window of the call's one shape at each file's own place in its own frame (the table of rans_parse).
enum : int { kFrame = 0, kOneWindow = 1, kFileWindows = 2 };

// the segment of `slot` under segments of S pixels, or -1 for a slot that is not live
__device__ __forceinline__ int window_segment(const RansWindow& w, int S, int slot) {
  const int J = (w.cols + S - 2) / S + 1;
  const int i = slot / J, j = slot - i * J;
  if (i >= w.rows) return -1;
  const int a = (w.r0 + i) * w.w8 + w.c0;  // < h8 w8 <= 2^23
  const int k = a / S + j;
  if (k > (a + w.cols - 1) / S) return -1;
  if (i > 0 && k <= (a - w.w8 + w.cols - 1) / S) return -1;
  return k;
}

// where the pixel at (gy, gx) of the latent goes in image img's window, or nullptr outside it
__device__ __forceinline__ uint8_t* window_pixel(const RansWindow& w, uint8_t* __restrict__ zwin, int img, int gy, int gx) {
  const uint32_t i = (uint32_t)(gy - w.r0), x = (uint32_t)(gx - w.c0);
  if (i >= (uint32_t)w.rows || x >= (uint32_t)w.cols) return nullptr;
  return zwin + (((size_t)img * w.rows + i) * w.cols + x) * kCh;
}

// One lane's reader of its segment's bytes [ptr, end): a read past end gives 0 and still counts, so
// the segment then fails the end check.
struct SegmentReader {
  const uint8_t* __restrict__ f;
  uint32_t ptr, end;
  __device__ __forceinline__ uint32_t next() {
    const uint32_t b = ptr < end ? (uint32_t)f[ptr] : 0u;
    ++ptr;
    return b;
  }
  __device__ __forceinline__ uint32_t state() {  // the segment's leading big-endian final state
    uint32_t x = next() << 24;
    x |= next() << 16;
    x |= next() << 8;
    return x | next();
  }
};

// One symbol of rans_decode_segments: the largest s with row[s] <= slot (row[0] = 0 <= slot < 4096
// = row[256]), then, for a lane that is on, the state update and up to two bytes of renormalisation.
// A lane past its last pixel keeps its final state.
__device__ __forceinline__ uint32_t decode_symbol(const uint16_t* row, uint32_t& x, bool on, SegmentReader& in) {
  const uint32_t slot = x & (kProbScale - 1);
  uint32_t s = 0;
#pragma unroll
  for (uint32_t step = 128; step > 0; step >>= 1)
    if (row[s + step] <= slot) s += step;
  const uint32_t lo = row[s], freq = row[s + 1] - lo;
  if (on) {
    x = freq * (x >> kProbBits) + slot - lo;
    if (x < kRansL) {
      x = (x << 8) | in.next();
      if (x < kRansL) x = (x << 8) | in.next();
    }
  }
  return s;
}

// The lane of rans_decode_segments: its segment (or none), its reader and its pixels [p0, p0 + mypix).
struct SegmentLane {
  bool live;
  int p0, mypix, maxpix;  // maxpix: the wave-uniform trip count
  SegmentReader in;
  uint32_t x;
};

// seg: the lane's segment, or -1 for none.  A live seg is < nseg = ceil(npix / seg_pixels), so
// p0 < npix and off[seg + 1] exists.
__device__ __forceinline__ SegmentLane segment_lane(int seg, int seg_pixels, int npix, const uint8_t* __restrict__ file,
                                                    const uint32_t* __restrict__ off, uint32_t pay, uint32_t size) {
  SegmentLane l;
  l.live = seg >= 0;
  l.p0 = l.live ? seg * seg_pixels : 0;
  l.mypix = l.live ? min(seg_pixels, npix - l.p0) : 0;
  l.in.f = file;
  l.in.ptr = l.live ? min(pay + off[seg], size) : 0u;
  l.in.end = l.live ? min(pay + off[seg + 1], size) : 0u;
  l.x = l.live ? l.in.state() : 0u;
  l.maxpix = l.mypix;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) l.maxpix = max(l.maxpix, __shfl_xor(l.maxpix, o, 64));
  return l;
}

// the block's first slot lies past the window's rows x J slots (block-uniform, before any per-lane work)
__device__ __forceinline__ bool window_block_dead(const RansWindow& w, int S, int first_slot) {
  return first_slot >= w.rows * ((w.cols + S - 2) / S + 1);
}

// ---- decode 2: segments, one lane per segment -----------------------------------------------
// block 64, one wave.  A lane reads only file bytes of its segment [begin, end) (a read past end
// gives 0), looks symbols up in rows that resolve every slot, and writes only its own latent bytes.
// Full frame (kWindow = kFrame): grid (ceil(maxseg / 64), n) covers seg_pixels = 1; lane = segment, blocks
// past the file's own nseg exit; pixel p of the lane goes to z (n, h8, w8, 96) at p0 + p.
// Window (kOneWindow, kFileWindows): grid (ceil(rows cols / 64), n) covers seg_pixels = 1 (J = cols); lane = slot,
// and a block without a live lane (every block of a refused image: nseg = 0) exits; the lane stores
// only the pixels of its segment that window_pixel places inside image img's (rows, cols, 96) of z.
// kFileWindows: win holds the call's rows and cols, and its w8, r0 and c0 -- and npix -- are image
// img's own, from row img = (h8, w8, r0, c0) of wintab (block-uniform; read behind the nseg exit, so
// only from a row the parse accepted: the window lies inside an h8 x w8 latent of that file).
// Either way the rows are staged only behind those exits.
// kContext: the row is chosen per symbol from the pixel decoded before (the context never leaves a
// segment, and a lane decodes its segment from the first pixel).  That pixel's 96 symbols stay in 24
// registers: chunk q of the left pixel is prev[0..3] in every iteration, and the array is rotated by
// one chunk after it, so every index is static and the q loop stays rolled.  anchor is not read
// without contexts, win not without a window, wintab only with per-file windows.
template <bool kContext, int kWindow>
__global__ __launch_bounds__(64) void rans_decode_segments(const uint8_t* __restrict__ files, long long stride, int npix,
                                                            const uint16_t* __restrict__ cum,
                                                            const uint8_t* __restrict__ anchor,
                                                            const uint32_t* __restrict__ segoff, int maxseg,
                                                            const uint32_t* __restrict__ meta, RansWindow win,
                                                            const int* __restrict__ wintab, uint8_t* __restrict__ z,
                                                            int* __restrict__ status) {
  using R = Rows<kContext>;
  __shared__ uint16_t start[R::kWords];
  const int lane = threadIdx.x, img = blockIdx.y;
  const int nseg = (int)meta[4 * img + 0];
  const int seg_pixels = (int)meta[4 * img + 1];
  int seg = (int)blockIdx.x * 64 + lane;
  if constexpr (kWindow) {
    if (nseg == 0) return;  // block-uniform
    if constexpr (kWindow == kFileWindows) {
      const int* t = wintab + 4 * (size_t)img;
      npix = t[0] * t[1];
      win.w8 = t[1];
      win.r0 = t[2];
      win.c0 = t[3];
    }
    if (window_block_dead(win, seg_pixels, (int)blockIdx.x * 64)) return;
    seg = window_segment(win, seg_pixels, seg);
    if (__ballot(seg >= 0) == 0) return;  // block-uniform: the block is this wave
  } else {
    if ((int)blockIdx.x * 64 >= nseg) return;  // block-uniform
    if (seg >= nseg) seg = -1;
  }
  load_rows<R>(start, cum + (size_t)img * R::kWords, lane, 64);
  __syncthreads();
  SegmentLane l = segment_lane(seg, seg_pixels, npix, files + (size_t)img * (size_t)stride,
                               segoff + (size_t)img * (maxseg + 1), meta[4 * img + 2], meta[4 * img + 3]);
  int gy = 0, gx = 0;  // window: the latent position of pixel p
  if constexpr (kWindow) {
    gy = l.p0 / win.w8;
    gx = l.p0 - gy * win.w8;
  }
  uint8_t* mine = z + ((size_t)img * npix + (size_t)l.p0) * kCh;  // full frame: the lane's pixels
  uint32_t prev[24];
#pragma unroll
  for (int i = 0; i < 24; ++i) prev[i] = 0;
  for (int p = 0; p < l.maxpix; ++p) {
    const bool on = p < l.mypix;
    uint8_t* dst = nullptr;
    if constexpr (kWindow) {
      if (on) dst = window_pixel(win, z, img, gy, gx);
    } else {
      if (on) dst = mine + (size_t)p * kCh;
    }
    for (int q = 0; q < 6; ++q) {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        uint32_t k = 0;  // k <= 2: the row is one of the image's
        if constexpr (kContext) k = p > 0 ? ctx_of((prev[b >> 2] >> (8 * (b & 3))) & 255u, anchor[16 * q + b]) : 0u;
        w[b >> 2] |= decode_symbol(R::row(start, 16 * q + b, k), l.x, on, l.in) << (8 * (b & 3));
      }
      if (dst) *(uint4*)(dst + 16 * q) = make_uint4(w[0], w[1], w[2], w[3]);
      if constexpr (kContext) {
#pragma unroll
        for (int i = 0; i < 20; ++i) prev[i] = prev[i + 4];
#pragma unroll
        for (int i = 0; i < 4; ++i) prev[20 + i] = w[i];
      }
    }
    if constexpr (kWindow) {
      if (++gx == win.w8) {
        gx = 0;
        ++gy;
      }
    }
  }
  if (l.live && !(l.x == kRansL && l.in.ptr == l.in.end)) atomicOr(&status[img], 1);
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

bool rans_shape_ok(int h8, int w8) {
  // file offsets, segment offsets and symbol counts are 32-bit: 144 B / pixel worst case
  return h8 > 0 && w8 > 0 && (long long)h8 * w8 <= (1ll << 23);
}

void rans_plan(int n, int h8, int w8, int seg_pixels, bool decode, RansPlan* pl, int ver) {
  const size_t npix = (size_t)h8 * w8, N = (size_t)n;
  const int S = decode ? 1 : seg_pixels;  // decode sizes its offsets for the smallest segments
  pl->nseg = (int)((npix + S - 1) / S);
  // a symbol of freq 1 costs 12 + log2(1 + 2^-11) bits in the worst case (the state may sit at
  // the bottom of its interval): 144 B per pixel, under 1/64 B per pixel of slack, the 4 state bytes
  pl->cap = decode ? 0 : (uint32_t)(144u * (uint32_t)seg_pixels + (uint32_t)seg_pixels / 64u + 8u);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  pl->counts = take(decode ? 0 : N * kCh * 256 * 4 * (ver == 3 ? kCtx : 1));
  pl->cum = take(N * (ver == 3 ? kCtxWords : kCumWords) * 2);
  pl->tab = take(decode ? 0 : N * kCh * kTabRow);
  pl->tablen = take(decode ? 0 : N * kCh * 4);
  pl->taboff = take(decode ? 0 : N * (kCh + 1) * 4);
  pl->keep = take(decode || ver == 1 ? 0 : N * kCh * 4);
  pl->seglen = take(N * pl->nseg * 4);
  pl->segoff = take(N * ((size_t)pl->nseg + 1) * 4);
  pl->meta = take(decode ? N * 16 : 0);
  pl->scratch = take(N * pl->nseg * pl->cap);
  pl->bytes = o;
}

namespace {

// a plan's offsets as typed pointers into the workspace
struct RansBuffers {
  uint32_t* counts;
  uint16_t* cum;
  uint8_t* tab;
  uint32_t *tablen, *taboff, *keep, *seglen, *segoff, *meta;
  uint8_t* scratch;
};

RansBuffers rans_buffers(char* ws, const RansPlan& pl) {
  return {(uint32_t*)(ws + pl.counts), (uint16_t*)(ws + pl.cum),    (uint8_t*)(ws + pl.tab),     (uint32_t*)(ws + pl.tablen),
          (uint32_t*)(ws + pl.taboff), (uint32_t*)(ws + pl.keep),   (uint32_t*)(ws + pl.seglen), (uint32_t*)(ws + pl.segoff),
          (uint32_t*)(ws + pl.meta),   (uint8_t*)(ws + pl.scratch)};
}

template <int kVer>
hipError_t rans_encode(const uint8_t* z, int n, int h8, int w8, int H, int W, int seg_pixels, const RansPrior& pr, char* ws,
                       const RansPlan& pl, uint8_t* out, long long stride, long long* sizes, hipStream_t st) {
  constexpr bool kContext = kVer == 3;
  constexpr size_t kCounts = (size_t)kCh * Rows<kContext>::kPerCh * 256;  // per image
  const int npix = h8 * w8, nseg = pl.nseg;
  const RansBuffers b = rans_buffers(ws, pl);
  hipError_t e = hipMemsetAsync(b.counts, 0, (size_t)n * kCounts * 4, st);
  if (e != hipSuccess) return e;
  if constexpr (kContext)
    rans3_hist<uint32_t><<<dim3((npix + 255) / 256, 6, n), 256, 0, st>>>(z, npix, seg_pixels, pr.anchor, b.counts, kCounts);
  else
    rans_hist<uint32_t><<<dim3((npix + 255) / 256, 3, n), 256, 0, st>>>(z, npix, b.counts, kCounts);
  if constexpr (kVer == 1)
    rans_normalise<<<dim3(kCh, n), 64, 0, st>>>(b.counts, npix, b.cum, b.tab, b.tablen);
  else
    rans_tables<kContext><<<dim3(kCh, n), 64, 0, st>>>(b.counts, npix, pr.freq, pr.cum, pr.cost16, b.cum, b.tab, b.tablen, b.keep);
  rans_encode_segments<kContext><<<dim3((nseg + 63) / 64, n), 64, 0, st>>>(z, npix, seg_pixels, nseg, b.cum, pr.anchor, b.scratch,
                                                                           pl.cap, b.seglen);
  rans_layout<kVer><<<dim3(n), 256, 0, st>>>(b.tablen, b.taboff, b.seglen, b.segoff, nseg, sizes);
  // version 1 writes neither H, W, the id nor the mask: its header ends before them
  rans_assemble<kVer><<<dim3((kCh + nseg + 3) / 4, n), 256, 0, st>>>(b.tab, b.tablen, b.taboff, b.scratch, pl.cap, b.seglen, b.segoff,
                                                                    nseg, seg_pixels, h8, w8, out, stride, (uint32_t)H, (uint32_t)W,
                                                                    pr.id, b.keep);
  return hipGetLastError();
}

// the parse, then every segment (win NULL), the window's slots, or (wintab) the slots of each file's
// own window of win's rows x cols: then h8, w8 and win's other fields are not used, and pl.nseg is the
// call's bound on a file's latent pixels
template <int kVer>
hipError_t rans_decode(const uint8_t* files, long long stride, const long long* sizes, int n, int h8, int w8, const RansWindow* win,
                       const int* wintab, const RansPrior& pr, char* ws, const RansPlan& pl, uint8_t* z, int* status,
                       hipStream_t st) {
  constexpr bool kContext = kVer == 3;
  const int npix = h8 * w8, maxseg = pl.nseg;
  const RansBuffers b = rans_buffers(ws, pl);
  rans_parse<kVer><<<dim3(n), 256, 0, st>>>(files, stride, sizes, h8, w8, wintab, win ? win->rows : 0, win ? win->cols : 0, pr.cum,
                                            pr.id, b.cum, b.seglen, b.segoff, maxseg, b.meta, status);
  if (wintab)
    rans_decode_segments<kContext, kFileWindows><<<dim3((win->rows * win->cols + 63) / 64, n), 64, 0, st>>>(
        files, stride, 0, b.cum, pr.anchor, b.segoff, maxseg, b.meta, *win, wintab, z, status);
  else if (win)
    rans_decode_segments<kContext, kOneWindow><<<dim3((win->rows * win->cols + 63) / 64, n), 64, 0, st>>>(
        files, stride, npix, b.cum, pr.anchor, b.segoff, maxseg, b.meta, *win, nullptr, z, status);
  else
    rans_decode_segments<kContext, kFrame><<<dim3((maxseg + 63) / 64, n), 64, 0, st>>>(
        files, stride, npix, b.cum, pr.anchor, b.segoff, maxseg, b.meta, RansWindow{}, nullptr, z, status);
  return hipGetLastError();
}

// ---- region decode's cut: dst (n, bh, bw, 3) = the bh x bw box at (off[img][0], off[img][1]) of
// image img of src (n, Hs, Ws, 3).  grid (ceil(n bh bw 3 / 1024)), block 256: a thread makes four
// consecutive bytes of dst (4-byte aligned) and stores them as one dword, so a wave writes 256
// contiguous bytes and reads runs of a source row.  A source byte outside its image -- a table row
// the caller did not check -- reads as 0 and nothing outside src is touched.
__global__ __launch_bounds__(256) void cut_boxes(const uint8_t* __restrict__ src, int Hs, int Ws, const int* __restrict__ off,
                                                  int bh, int bw, uint8_t* __restrict__ dst, size_t total) {
  const size_t at = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (at >= total) return;
  const uint32_t row_bytes = 3u * (uint32_t)bw;  // bw <= Ws: 3 Ws fits an int (checked on the host)
  const size_t img_bytes = (size_t)row_bytes * (uint32_t)bh;
  size_t img = at / img_bytes;
  const size_t rem = at - img * img_bytes;
  uint32_t y = (uint32_t)(rem / row_bytes), b = (uint32_t)(rem - (size_t)y * row_bytes);
  uint32_t word = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (at + k < total) {
      const long long sy = (long long)off[2 * img] + y, sb = 3ll * off[2 * img + 1] + b;
      uint32_t v = 0;
      if (sy >= 0 && sy < Hs && sb >= 0 && sb < 3ll * Ws) v = src[((size_t)img * Hs + (size_t)sy) * (3 * (size_t)Ws) + (size_t)sb];
      word |= v << (8 * k);
      if (++b == row_bytes) {
        b = 0;
        if (++y == (uint32_t)bh) {
          y = 0;
          ++img;
        }
      }
    }
  }
  if (at + 4 <= total) {
    *(uint32_t*)(dst + at) = word;
  } else {
    for (size_t k = 0; at + k < total; ++k) dst[at + k] = (uint8_t)(word >> (8 * k));
  }
}

// The device allocation of a prior: freqs | cumulative rows at the segment kernels' pitch | the 96
// anchors (a context prior only) | the cost table.  Every part starts at a multiple of 4.
size_t prior_layout(bool context, size_t* cum_at, size_t* anchor_at, size_t* cost_at) {
  *cum_at = (size_t)kCh * (context ? kCtx : 1) * 256 * 2;
  *anchor_at = *cum_at + (size_t)(context ? kCtxWords : kCumWords) * 2;
  *cost_at = *anchor_at + (context ? kCh : 0);
  return *cost_at + (kProbScale + 1) * 4;
}

}  // namespace

hipError_t launch_rans_encode(int ver, const uint8_t* z, int n, int h8, int w8, int H, int W, int seg_pixels, const RansPrior& pr,
                              char* ws, const RansPlan& pl, uint8_t* out, long long stride, long long* sizes, hipStream_t st) {
  switch (ver) {
    case 1: return rans_encode<1>(z, n, h8, w8, H, W, seg_pixels, pr, ws, pl, out, stride, sizes, st);
    case 2: return rans_encode<2>(z, n, h8, w8, H, W, seg_pixels, pr, ws, pl, out, stride, sizes, st);
    case 3: return rans_encode<3>(z, n, h8, w8, H, W, seg_pixels, pr, ws, pl, out, stride, sizes, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_rans_decode(int ver, const uint8_t* files, long long stride, const long long* sizes, int n, int h8, int w8,
                              const RansWindow* win, const int* wintab, const RansPrior& pr, char* ws, const RansPlan& pl,
                              uint8_t* z, int* status, hipStream_t st) {
  switch (ver) {
    case 1: return rans_decode<1>(files, stride, sizes, n, h8, w8, win, wintab, pr, ws, pl, z, status, st);
    case 2: return rans_decode<2>(files, stride, sizes, n, h8, w8, win, wintab, pr, ws, pl, z, status, st);
    case 3: return rans_decode<3>(files, stride, sizes, n, h8, w8, win, wintab, pr, ws, pl, z, status, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_cut_boxes(const uint8_t* src, int n, int Hs, int Ws, const int* off, int bh, int bw, uint8_t* dst, hipStream_t st) {
  const size_t total = (size_t)n * bh * bw * 3;
  cut_boxes<<<dim3((unsigned)((total + 1023) / 1024)), 256, 0, st>>>(src, Hs, Ws, off, bh, bw, dst, total);
  return hipGetLastError();
}

hipError_t launch_rans_prior_count(const uint8_t* z, int n, int h8, int w8, int seg_pixels, const uint8_t* anchor,
                                   unsigned long long* counts, hipStream_t st) {
  const int npix = h8 * w8;
  if (anchor)
    rans3_hist<unsigned long long><<<dim3((npix + 255) / 256, 6, n), 256, 0, st>>>(z, npix, seg_pixels, anchor, counts, 0);
  else
    rans_hist<unsigned long long><<<dim3((npix + 255) / 256, 3, n), 256, 0, st>>>(z, npix, counts, 0);
  return hipGetLastError();
}

hipError_t launch_rans_prior_build(bool context, const unsigned long long* counts, uint16_t* freqs, hipStream_t st) {
  rans_prior_normalise<<<dim3(kCh * (context ? kCtx : 1)), 64, 0, st>>>(counts, freqs);
  return hipGetLastError();
}

std::vector<char> rans_prior_pack(const uint8_t* anchors, const uint16_t* freqs) {
  const bool context = anchors != nullptr;
  const int rows = kCh * (context ? kCtx : 1), pitch = context ? kCtxRow : kCumRow;
  size_t cum_at, anchor_at, cost_at;
  std::vector<char> host(prior_layout(context, &cum_at, &anchor_at, &cost_at), 0);
  std::memcpy(host.data(), freqs, cum_at);
  uint16_t* cum = (uint16_t*)(host.data() + cum_at);
  for (int row = 0; row < rows; ++row) {
    uint32_t run = 0;
    for (int s = 0; s < 256; ++s) {
      cum[row * pitch + s] = (uint16_t)run;
      run += freqs[row * 256 + s];
    }
    cum[row * pitch + 256] = (uint16_t)run;  // 4096
  }
  if (context) std::memcpy(host.data() + anchor_at, anchors, kCh);
  nic_rans_cost_table((uint32_t*)(host.data() + cost_at));
  return host;
}

RansPrior rans_prior_view(bool context, const char* dev, uint32_t id) {
  size_t cum_at, anchor_at, cost_at;
  prior_layout(context, &cum_at, &anchor_at, &cost_at);
  return {(const uint16_t*)dev, (const uint16_t*)(dev + cum_at), context ? (const uint8_t*)(dev + anchor_at) : nullptr,
          (const uint32_t*)(dev + cost_at), id};
}


}  // namespace nic

// ---- host-only checks and entry points ---------------------------------------------------------

// Every check of a version-`ver` file, for the nic_rans*_inspect named fn: the header (16 bytes in
// version 1; 40 in versions 2 and 3, which also relate H / W to the latent), the tables (all 96 in
// version 1, the masked channels' in versions 2 and 3), the segment table and the size.  Every
// output is nullable; H, W and prior_id are written for versions 2 and 3 only.
static int inspect_file(const char* fn, int ver, const uint8_t* f, int64_t size, int* h8, int* w8, int* seg_pixels, int* H, int* W,
                        uint32_t* prior_id) {
  char msg[200], text[160];
  auto corrupt = [&](const char* what, long long a = 0, long long b = 0) {
    snprintf(text, sizeof(text), what, a, b);
    snprintf(msg, sizeof(msg), "%s: %s", fn, text);
    return nic::set_error(NIC_ECORRUPT, msg);
  };
  if (!f) {
    snprintf(msg, sizeof(msg), "%s: file is NULL", fn);
    return nic::set_error(NIC_EINVAL, msg);
  }
  const int header = ver == 1 ? nic::kHeader : nic::kHeader2;
  if (size < nic::kHeader) return corrupt("%lld bytes are less than the %lld-byte header", size, header);
  if (std::memcmp(f, "NICR", 4) != 0) return corrupt("bad magic");
  if (f[4] != ver) return corrupt("version %lld, expected %lld", f[4], ver);
  if (size < header) return corrupt("%lld bytes are less than the %lld-byte header", size, header);
  if (f[5] != nic::kProbBits) return corrupt("%lld probability bits, expected 12", f[5]);
  auto u32 = [&](int64_t at) { return (uint32_t)f[at] | ((uint32_t)f[at + 1] << 8) | ((uint32_t)f[at + 2] << 16) | ((uint32_t)f[at + 3] << 24); };
  const uint32_t S = (uint32_t)f[6] | ((uint32_t)f[7] << 8), fh = u32(8), fw = u32(12);
  if (S == 0) return corrupt("seg_pixels is 0");
  if (fh == 0 || fw == 0 || fh > (1u << 23) || fw > (1u << 23) || !nic::rans_shape_ok((int)fh, (int)fw))
    return corrupt("latent size %lld x %lld out of range", fh, fw);
  const uint32_t ih = ver == 1 ? 0u : u32(16), iw = ver == 1 ? 0u : u32(20);
  if (ver != 1) {
    if ((ih >> 3) + ((ih & 7u) != 0u) != fh) return corrupt("image height %lld does not give h8 = %lld", ih, fh);
    if ((iw >> 3) + ((iw & 7u) != 0u) != fw) return corrupt("image width %lld does not give w8 = %lld", iw, fw);
  }
  int64_t at = header;
  for (int c = 0; c < nic::kCh; ++c) {
    if (ver != 1 && !((f[28 + (c >> 3)] >> (c & 7)) & 1)) continue;  // the prior's row(s)
    if (at >= size) return corrupt("truncated in the table of channel %lld", c);
    const int nsym = f[at] + 1;
    if (at + 1 + 3 * nsym > size) return corrupt("truncated in the table of channel %lld", c);
    int prev = -1;
    uint32_t sum = 0;
    for (int e = 0; e < nsym; ++e) {
      const int s = f[at + 1 + 3 * e];
      const uint32_t fr = (uint32_t)f[at + 2 + 3 * e] | ((uint32_t)f[at + 3 + 3 * e] << 8);
      if (s <= prev) return corrupt("channel %lld: symbols not strictly ascending", c);
      if (fr < 1 || fr > nic::kProbScale) return corrupt("channel %lld: freq %lld not in 1..4096", c, fr);
      prev = s;
      sum += fr;
    }
    if (sum != nic::kProbScale) return corrupt("channel %lld: freqs sum to %lld, not 4096", c, sum);
    at += 1 + 3 * nsym;
  }
  const int64_t npix = (int64_t)fh * fw, nseg = (npix + S - 1) / S;
  if (at + 4 * nseg > size) return corrupt("truncated in the segment table");
  int64_t pay = 0;
  for (int64_t k = 0; k < nseg; ++k) pay += u32(at + 4 * k);
  if (at + 4 * nseg + pay != size)
    return corrupt("header, tables and segments need %lld bytes, the file has %lld", at + 4 * nseg + pay, size);
  if (h8) *h8 = (int)fh;
  if (w8) *w8 = (int)fw;
  if (seg_pixels) *seg_pixels = (int)S;
  if (ver != 1) {
    if (H) *H = (int)ih;
    if (W) *W = (int)iw;
    if (prior_id) *prior_id = u32(24);
  }
  return NIC_OK;
}

// A prior's freqs, 96 x per_ch rows of 256 (per_ch 1: the static prior; 3: the context prior): each
// in 1..4096, every row summing to 4096.  id: the CRC-32 of the anchors (a context prior only), then
// the freqs as little-endian u16, channel-major, then context, then symbol.
static int check_freq_rows(const char* fn, const uint8_t* anchors, const uint16_t* freqs, int per_ch, uint32_t* id) {
  char msg[160], where[40];
  for (int r = 0; r < nic::kCh * per_ch; ++r) {
    if (per_ch == 1) snprintf(where, sizeof(where), "channel %d", r);
    else snprintf(where, sizeof(where), "channel %d context %d", r / per_ch, r % per_ch);
    uint32_t sum = 0;
    for (int s = 0; s < 256; ++s) {
      const uint32_t fr = freqs[r * 256 + s];
      if (fr < 1 || fr > nic::kProbScale) {
        snprintf(msg, sizeof(msg), "%s: %s: freq %u of symbol %d not in 1..4096", fn, where, fr, s);
        return nic::set_error(NIC_ECORRUPT, msg);
      }
      sum += fr;
    }
    if (sum != nic::kProbScale) {
      snprintf(msg, sizeof(msg), "%s: %s: freqs sum to %u, not 4096", fn, where, sum);
      return nic::set_error(NIC_ECORRUPT, msg);
    }
  }
  if (id) {
    uint8_t le[512];
    uLong crc = crc32(0L, Z_NULL, 0);
    if (anchors) crc = crc32(crc, anchors, nic::kCh);
    for (int r = 0; r < nic::kCh * per_ch; ++r) {
      for (int s = 0; s < 256; ++s) {
        le[2 * s] = (uint8_t)(freqs[r * 256 + s] & 255u);
        le[2 * s + 1] = (uint8_t)(freqs[r * 256 + s] >> 8);
      }
      crc = crc32(crc, le, sizeof(le));
    }
    *id = (uint32_t)crc;
  }
  return NIC_OK;
}

extern "C" {

int nic_rans_bound(int h8, int w8, int seg_pixels, int64_t* bytes) {
  if (!bytes) return nic::set_error(NIC_EINVAL, "nic_rans_bound: bytes is NULL");
  if (!nic::rans_shape_ok(h8, w8)) return nic::set_error(NIC_ESHAPE, "nic_rans_bound: latent size out of range");
  if (seg_pixels < 1 || seg_pixels > 65535) return nic::set_error(NIC_ESHAPE, "nic_rans_bound: seg_pixels not in 1..65535");
  const int64_t npix = (int64_t)h8 * w8, nseg = (npix + seg_pixels - 1) / seg_pixels;
  // header, 96 full tables, the segment table, 12 bits per symbol and 4 state bytes per segment
  *bytes = nic::kHeader + (int64_t)nic::kCh * (1 + 3 * 256) + 4 * nseg + 144 * npix + 4 * nseg;
  return NIC_OK;
}

int nic_rans_inspect(const uint8_t* f, int64_t size, int* h8, int* w8, int* seg_pixels) {
  return inspect_file("nic_rans_inspect", 1, f, size, h8, w8, seg_pixels, nullptr, nullptr, nullptr);
}

int nic_rans2_inspect(const uint8_t* f, int64_t size, int* h8, int* w8, int* seg_pixels, int* H, int* W, uint32_t* prior_id) {
  return inspect_file("nic_rans2_inspect", 2, f, size, h8, w8, seg_pixels, H, W, prior_id);
}

int nic_rans3_inspect(const uint8_t* f, int64_t size, int* h8, int* w8, int* seg_pixels, int* H, int* W, uint32_t* prior_id) {
  return inspect_file("nic_rans3_inspect", 3, f, size, h8, w8, seg_pixels, H, W, prior_id);
}

int nic_rans_cost_table(uint32_t* out4097) {
  if (!out4097) return nic::set_error(NIC_EINVAL, "nic_rans_cost_table: out is NULL");
  out4097[0] = 0;
  for (uint32_t f = 1; f <= nic::kProbScale; ++f)
    out4097[f] = (uint32_t)std::floor((12.0 - std::log2((double)f)) * 65536.0 + 0.5);
  return NIC_OK;
}

int nic_rans_prior_check(const uint16_t* freqs, uint32_t* id) {
  if (!freqs) return nic::set_error(NIC_EINVAL, "nic_rans_prior_check: freqs is NULL");
  return check_freq_rows("nic_rans_prior_check", nullptr, freqs, 1, id);
}

int nic_rans_cprior_check(const uint8_t* anchors, const uint16_t* freqs, uint32_t* id) {
  if (!anchors || !freqs) return nic::set_error(NIC_EINVAL, "nic_rans_cprior_check: anchors or freqs is NULL");
  return check_freq_rows("nic_rans_cprior_check", anchors, freqs, nic::kCtx, id);
}

int nic_rans2_bound(int h8, int w8, int seg_pixels, int64_t* bytes) {
  const int rc = nic_rans_bound(h8, w8, seg_pixels, bytes);
  if (rc == NIC_OK) *bytes += nic::kHeader2 - nic::kHeader;
  return rc;
}

int nic_region_plan(int H, int W, int y, int x, int bh, int bw, int* win4, int* off2) {
  if (!win4 || !off2) return nic::set_error(NIC_EINVAL, "nic_region_plan: win4 or off2 is NULL");
  if (H < 1 || W < 1 || y < 0 || x < 0 || bh < 1 || bw < 1 || (long long)y + bh > H || (long long)x + bw > W) {
    char msg[160];
    snprintf(msg, sizeof(msg), "nic_region_plan: box (y %d, x %d, %d x %d) does not lie inside a %d x %d image", y, x, bh, bw, H, W);
    return nic::set_error(NIC_ESHAPE, msg);
  }
  const int h8 = (H >> 3) + ((H & 7) != 0), w8 = (W >> 3) + ((W & 7) != 0);
  auto axis = [](int at, int len, int n8, int* lo, int* count) {
    const int first = at / 8, last = (at + len - 1) / 8 + 1;  // the latent pixels the box touches: [first, last)
    const int a = first - NIC_DECODE_HALO > 0 ? first - NIC_DECODE_HALO : 0;
    const int b = last + NIC_DECODE_HALO < n8 ? last + NIC_DECODE_HALO : n8;
    *lo = a;
    *count = b - a;
  };
  axis(y, bh, h8, &win4[0], &win4[2]);
  axis(x, bw, w8, &win4[1], &win4[3]);
  off2[0] = y - 8 * win4[0];
  off2[1] = x - 8 * win4[1];
  return NIC_OK;
}

int nic_region_plan_fixed(int H, int W, int y, int x, int bh, int bw, int* win4, int* off2) {
  if (!win4 || !off2) return nic::set_error(NIC_EINVAL, "nic_region_plan_fixed: win4 or off2 is NULL");
  if (H < 1 || W < 1 || y < 0 || x < 0 || bh < 1 || bw < 1 || (long long)y + bh > H || (long long)x + bw > W) {
    char msg[160];
    snprintf(msg, sizeof(msg), "nic_region_plan_fixed: box (y %d, x %d, %d x %d) does not lie inside a %d x %d image", y, x, bh, bw,
             H, W);
    return nic::set_error(NIC_ESHAPE, msg);
  }
  const int h8 = (H >> 3) + ((H & 7) != 0), w8 = (W >> 3) + ((W & 7) != 0);
  auto axis = [](int at, int len, int n8, int* lo, int* count) {
    const int touched = (len + 6) / 8 + 1;  // the most latent pixels that len image pixels touch (len <= H: no overflow)
    const int fixed = touched + 2 * NIC_DECODE_HALO;
    *count = fixed < n8 ? fixed : n8;
    const int want = at / 8 - NIC_DECODE_HALO, last = n8 - *count;
    *lo = want < 0 ? 0 : (want > last ? last : want);
  };
  axis(y, bh, h8, &win4[0], &win4[2]);
  axis(x, bw, w8, &win4[1], &win4[3]);
  off2[0] = y - 8 * win4[0];
  off2[1] = x - 8 * win4[1];
  return NIC_OK;
}

int nic_rans_window_segments(int h8, int w8, int seg_pixels, int r0, int c0, int rows, int cols, int64_t* count) {
  if (!count) return nic::set_error(NIC_EINVAL, "nic_rans_window_segments: count is NULL");
  if (!nic::rans_shape_ok(h8, w8)) return nic::set_error(NIC_ESHAPE, "nic_rans_window_segments: latent size out of range");
  if (seg_pixels < 1 || seg_pixels > 65535)
    return nic::set_error(NIC_ESHAPE, "nic_rans_window_segments: seg_pixels not in 1..65535");
  if (r0 < 0 || c0 < 0 || rows < 1 || cols < 1 || (long long)r0 + rows > h8 || (long long)c0 + cols > w8)
    return nic::set_error(NIC_ESHAPE, "nic_rans_window_segments: the window does not lie inside the latent");
  int64_t total = 0, seen = -1;  // seen: the last segment counted so far
  for (int i = 0; i < rows; ++i) {
    const int64_t a = (int64_t)(r0 + i) * w8 + c0, first = a / seg_pixels, last = (a + cols - 1) / seg_pixels;
    const int64_t from = first > seen ? first : seen + 1;
    if (last >= from) total += last - from + 1;
    seen = last;
  }
  *count = total;
  return NIC_OK;
}

int nic_rans3_bound(int h8, int w8, int seg_pixels, int64_t* bytes) { return nic_rans2_bound(h8, w8, seg_pixels, bytes); }

}  // extern "C"
