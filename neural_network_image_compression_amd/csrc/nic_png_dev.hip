// The device PNG writer: complete PNG files of u8 images, filtered, Huffman-coded and framed on
// the device (format: DESIGN.md "The device PNG writer"; entry points: include/nic.h
// nic_png_device_*).  One file per image:
//   signature | IHDR | one IDAT (zlib header, the deflate blocks, Adler-32) | IEND
// The filtered stream (filter byte + filtered row, Pillow's adaptive choice or a fixed filter) is
// cut into blocks of kBlock bytes.  Every block is coded on its own: one dynamic-Huffman block of
// literals and the end-of-block code, closed by an empty stored block that realigns the stream to
// a byte (so blocks are concatenated as bytes), or a stored block when that is no larger.  No
// LZ77 matching.
//
// png_filter (one wave per row) -> png_codes (one workgroup per block: histogram, Adler sums,
// length-limited code lengths, canonical codes, the block header's bits, the block's size) ->
// png_layout (per image: block offsets, file size, Adler-32) -> png_emit (one workgroup per block:
// the block's bytes assembled in LDS, their CRC-32, word stores into the file) -> png_finish (per
// image: the blocks' CRCs combined, signature, IHDR, IDAT framing, IEND).

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nic.h"
#include "nic_kernels.h"

namespace nic {

namespace {

constexpr int kBlock = 16384;             // bytes of the filtered stream per deflate block
constexpr int kThreads = 256;
constexpr int kRun = kBlock / kThreads;   // symbols one thread of png_emit codes
constexpr int kLit = 257;                 // literals 0..255 and end-of-block
constexpr int kLitBits = 15;              // deflate's limit for the literal/length code
constexpr int kClSyms = 19;               // the code-length alphabet (16, 17, 18 are never used)
constexpr int kClBits = 7;                // deflate's limit for the code-length code
constexpr int kFixedHdrBits = 3 + 14 + 3 * kClSyms;  // BFINAL/BTYPE, HLIT/HDIST/HCLEN, 19 x 3 bits
constexpr int kTabWords = 260;            // per block: 257 (reversed code | length << 16)
constexpr int kHdrWords = 64;             // per block: 74 + 258 * 7 = 1,880 header bits at most
constexpr int kMeta = 8;                  // per block: header bits (0 = stored), bytes, s1, s2, offset, crc
constexpr int kFraming = 8 + 25 + 8 + 2 + 4 + 4 + 12;  // signature, IHDR, IDAT length + type, zlib header, Adler, CRC, IEND
constexpr int kPayloadAt = 8 + 25 + 8 + 2;             // file offset of the first deflate block
constexpr uint32_t kAdlerMod = 65521u;
constexpr uint32_t kCrcPoly = 0xedb88320u;
constexpr int kObufWords = (kBlock + 5) / 4 + 8;  // a block's bytes (never above stored form) and slack

// ---- CRC-32 as polynomial arithmetic (reflected, as zlib's crc32_combine) -----------------------
// a(x) b(x) mod P
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
// x^(8 n) mod P by square and multiply
__host__ __device__ constexpr uint32_t gf_x8n(uint32_t n) {
  uint32_t p = 1u << 31, sq = 1u << 30;  // x^0, x^1
  sq = gf_mul(sq, sq);                   // x^2
  sq = gf_mul(sq, sq);                   // x^4
  sq = gf_mul(sq, sq);                   // x^8
  for (; n; n >>= 1) {
    if (n & 1u) p = gf_mul(sq, p);
    sq = gf_mul(sq, sq);
  }
  return p;
}
__host__ __device__ constexpr uint32_t crc_byte(uint32_t c, uint32_t byte) {  // c: the running (inverted) register
  c ^= byte;
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
  return c;
}

// ---- minimum-redundancy code lengths ---------------------------------------------------------------
// Moffat and Katajainen's in-place calculation: a[0..n) ascending weights -> code lengths
// (non-increasing), n >= 1.
__host__ __device__ inline void min_redundancy(uint32_t* a, int n) {
  if (n == 1) {
    a[0] = 1;
    return;
  }
  a[0] += a[1];
  int root = 0, leaf = 2;
  for (int next = 1; next < n - 1; ++next) {
    if (leaf >= n || a[root] < a[leaf]) {
      a[next] = a[root];
      a[root++] = (uint32_t)next;
    } else {
      a[next] = a[leaf++];
    }
    if (leaf >= n || (root < next && a[root] < a[leaf])) {
      a[next] += a[root];
      a[root++] = (uint32_t)next;
    } else {
      a[next] += a[leaf++];
    }
  }
  a[n - 2] = 0;
  for (int next = n - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
  int avbl = 1, used = 0, dpth = 0, next = n - 1;
  root = n - 2;
  while (avbl > 0) {
    while (root >= 0 && (int)a[root] == dpth) {
      ++used;
      --root;
    }
    while (avbl > used) {
      a[next--] = (uint32_t)dpth;
      --avbl;
    }
    avbl = 2 * used;
    ++dpth;
    used = 0;
  }
}

// The length limit: num[l] = codes of length l (num[maxbits] already holds every longer one).
// While the Kraft sum exceeds 1, one code of length maxbits is dropped, the deepest shorter code
// takes a sibling (its length and the dropped code's become one more): every step lowers the sum
// by 2^-maxbits and keeps the number of codes, so it ends at exactly 1.
__host__ __device__ inline void limit_lengths(uint32_t* num, int maxbits) {
  uint32_t total = 0;
  for (int i = 1; i <= maxbits; ++i) total += num[i] << (maxbits - i);
  while (total > (1u << maxbits)) {
    --num[maxbits];
    for (int i = maxbits - 1; i >= 1; --i)
      if (num[i]) {
        --num[i];
        num[i + 1] += 2;
        break;
      }
    --total;
  }
}

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_xor32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o, 64);
  return v;
}

// exclusive prefix sum of v over the 256 threads (every thread calls); *total = the sum.  sh: 4 words
__device__ uint32_t block_excl(uint32_t v, uint32_t* sh, uint32_t* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();  // sh may still be read from the previous call
  if (lane == 63) sh[wv] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t s = sh[k];
    if (k < wv) base += s;
    tot += s;
  }
  *total = tot;
  return base + inc - v;
}
// sum of v over the 256 threads, in every thread.  sh: 4 words
__device__ uint32_t block_sum(uint32_t v, uint32_t* sh) {
  v = wave_sum32(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}
__device__ uint32_t block_xor(uint32_t v, uint32_t* sh) {
  v = wave_xor32(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] ^ sh[1] ^ sh[2] ^ sh[3];
}
// sum of 64-bit v over the 256 threads modulo 65521 (each v < 2^63 / 256)
__device__ uint32_t block_sum_mod(unsigned long long v, uint32_t* sh) { return block_sum((uint32_t)(v % kAdlerMod), sh) % kAdlerMod; }

// ---- 1: filter.  grid (ceil(h / 4), n), block 256: one wave per row ------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ uint32_t filtered(int f, int x, int a, int b, int c) {
  const int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? ((a + b) >> 1) : paeth(a, b, c);
  return (uint32_t)(x - pred) & 255u;
}
// filter < 0: the filter whose output, read as signed bytes, has the least sum of absolute values
// (None, Sub, Up, Average, Paeth; first on ties; the row above the first is zero)
__global__ __launch_bounds__(256) void png_filter(const uint8_t* __restrict__ img, int h, int wb, int bpp, int filter,
                                                  uint8_t* __restrict__ filt, size_t fstride) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6), im = blockIdx.y;
  if (r >= h) return;  // wave-uniform; the kernel has no barrier
  const uint8_t* x = img + ((size_t)im * h + r) * wb;
  const uint8_t* up = x - wb;  // read only for r > 0
  int best = filter;
  if (filter < 0) {
    uint32_t s[5] = {0, 0, 0, 0, 0};
    for (int i = lane; i < wb; i += 64) {
      const int xi = x[i], a = i >= bpp ? x[i - bpp] : 0, b = r ? up[i] : 0, c = (r && i >= bpp) ? up[i - bpp] : 0;
#pragma unroll
      for (int f = 0; f < 5; ++f) {
        const uint32_t v = filtered(f, xi, a, b, c);
        s[f] += v < 128u ? v : 256u - v;
      }
    }
    best = 0;
    uint32_t least = wave_sum32(s[0]);
#pragma unroll
    for (int f = 1; f < 5; ++f) {
      const uint32_t t = wave_sum32(s[f]);
      if (t < least) {
        least = t;
        best = f;
      }
    }
  }
  uint8_t* dst = filt + (size_t)im * fstride + (size_t)r * (wb + 1);
  if (lane == 0) dst[0] = (uint8_t)best;
  for (int i = lane; i < wb; i += 64) {
    const int xi = x[i], a = i >= bpp ? x[i - bpp] : 0, b = r ? up[i] : 0, c = (r && i >= bpp) ? up[i - bpp] : 0;
    dst[1 + i] = (uint8_t)filtered(best, xi, a, b, c);
  }
}

// ---- 2: counts and codes.  grid (nblocks, n), block 256 -----------------------------------------
// Code lengths of the symbols with cnt > 0 among nsym <= 257 (every thread calls): rank by (count,
// symbol), min_redundancy on the sorted counts, the length limit, then lengths handed out by rank
// (the most frequent symbol takes the shortest code; equal counts: the higher symbol).  num[l]
// becomes the number of codes of length l.
__device__ void build_lengths(const uint32_t* cnt, int nsym, int maxbits, uint32_t* key, uint16_t* order, uint8_t* len,
                              uint32_t* num, int* nused) {
  const int tid = threadIdx.x;
  for (int s = tid; s < nsym; s += kThreads) {
    len[s] = 0;
    const uint32_t c = cnt[s];
    if (c) {
      int r = 0;
      for (int t = 0; t < nsym; ++t) {
        const uint32_t ct = cnt[t];
        r += (ct && (ct < c || (ct == c && t < s))) ? 1 : 0;
      }
      order[r] = (uint16_t)s;
      key[r] = c;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int t = 0; t < nsym; ++t) n += cnt[t] ? 1 : 0;
    *nused = n;
    for (int l = 0; l <= 15; ++l) num[l] = 0;
    if (n > 0) {
      min_redundancy(key, n);
      for (int i = 0; i < n; ++i) num[min((int)key[i], maxbits)] += 1;
      limit_lengths(num, maxbits);
    }
  }
  __syncthreads();
  const int n = *nused;
  for (int j = tid; j < n; j += kThreads) {
    const uint32_t q = (uint32_t)(n - 1 - j);  // 0 = the most frequent
    int l = 1;
    uint32_t acc = num[1];
    while (q >= acc && l < maxbits) acc += num[++l];
    len[order[j]] = (uint8_t)l;
  }
  __syncthreads();
}

// canonical code of symbol s (len[s] > 0), bit-reversed for deflate's LSB-first stream
__device__ __forceinline__ uint32_t canonical(const uint8_t* len, const uint32_t* num, int s) {
  const int l = len[s];
  uint32_t code = 0;
  for (int i = 1; i < l; ++i) code = (code + num[i]) << 1;  // first code of length l
  for (int t = 0; t < s; ++t) code += len[t] == l ? 1u : 0u;
  return __brev(code) >> (32 - l);
}

// deflate's order of the code-length code's own lengths
__constant__ uint8_t kClOrder[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ void or_bits(uint32_t* words, uint32_t pos, uint32_t val, uint32_t nbits) {
  const uint32_t sh = pos & 31u;
  atomicOr(&words[pos >> 5], val << sh);
  if (sh + nbits > 32u) atomicOr(&words[(pos >> 5) + 1], val >> (32u - sh));
}

__global__ __launch_bounds__(256) void png_codes(const uint8_t* __restrict__ filt, size_t fstride, uint32_t total, int nblocks,
                                                 uint32_t* __restrict__ tab, uint32_t* __restrict__ hdr,
                                                 uint32_t* __restrict__ meta) {
  __shared__ uint32_t cnt[kLit + 3], key[kLit + 3], num[16], clcnt[kClSyms], clnum[16], hw[kHdrWords], sh[4];
  __shared__ uint16_t order[kLit + 3];
  __shared__ uint8_t len[kLit + 3], cllen[kClSyms + 1];
  __shared__ uint32_t clcode[kClSyms];
  __shared__ int nused;
  const int tid = threadIdx.x, b = blockIdx.x, img = blockIdx.y;
  const size_t bi = (size_t)img * nblocks + b;
  const uint32_t blen = min((uint32_t)kBlock, total - (uint32_t)b * kBlock);
  const uint8_t* src = filt + (size_t)img * fstride + (size_t)b * kBlock;
  for (int i = tid; i < kLit + 3; i += kThreads) cnt[i] = 0;
  if (tid < kClSyms) clcnt[tid] = 0;
  if (tid < kHdrWords) hw[tid] = 0;
  __syncthreads();
  // histogram and the block's Adler sums: s1 = sum of bytes, s2 = sum of (blen - position) * byte
  uint32_t s1 = 0;
  unsigned long long s2 = 0;
#pragma unroll
  for (int k = 0; k < kBlock / (16 * kThreads); ++k) {
    const uint32_t o = 16u * (uint32_t)(k * kThreads + tid);
    if (o < blen) {  // the 16 bytes lie inside the image's fstride (a multiple of 16 above total)
      const uint4 v = *(const uint4*)(src + o);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (o + j < blen) {
          const uint32_t by = (w[j >> 2] >> (8 * (j & 3))) & 255u;
          atomicAdd(&cnt[by], 1u);
          s1 += by;
          s2 += (unsigned long long)(blen - (o + j)) * by;
        }
    }
  }
  if (tid == 0) cnt[256] = 1;  // end-of-block
  const uint32_t S1 = block_sum(s1, sh) % kAdlerMod;
  const uint32_t S2 = block_sum_mod(s2, sh);
  __syncthreads();
  build_lengths(cnt, kLit, kLitBits, key, order, len, num, &nused);
  // the literal codes and the coded size of the symbols
  uint32_t body = 0;
  for (int s = tid; s < kLit; s += kThreads) {
    uint32_t e = 0;
    if (len[s]) {
      e = canonical(len, num, s) | ((uint32_t)len[s] << 16);
      body += cnt[s] * len[s];
      atomicAdd(&clcnt[len[s]], 1u);
    } else {
      atomicAdd(&clcnt[0], 1u);
    }
    tab[bi * kTabWords + s] = e;
  }
  if (tid == 0) atomicAdd(&clcnt[0], 1u);  // the one distance code, of length 0
  body = block_sum(body, sh);
  __syncthreads();
  // the code-length code over lengths 0..15 (no run codes)
  build_lengths(clcnt, kClSyms, kClBits, key, order, cllen, clnum, &nused);
  if (tid < kClSyms) clcode[tid] = cllen[tid] ? canonical(cllen, clnum, tid) : 0u;
  __syncthreads();
  // header: BFINAL 0, BTYPE 2, HLIT 0 (257 codes), HDIST 0 (1 code), HCLEN 15 (19 lengths), the 19
  // lengths in deflate's order, then the 258 code lengths
  if (tid == 0) {
    or_bits(hw, 0, 4u, 3);
    or_bits(hw, 13, 15u, 4);
  }
  if (tid < kClSyms) or_bits(hw, 17 + 3 * tid, cllen[kClOrder[tid]], 3);
  const uint32_t myl = len[tid], mybits = cllen[myl];
  uint32_t tot = 0;
  const uint32_t ex = block_excl(mybits, sh, &tot);
  or_bits(hw, kFixedHdrBits + ex, clcode[myl], mybits);
  const uint32_t l256 = len[256], b256 = cllen[l256], b257 = cllen[0];
  if (tid == 0) {
    or_bits(hw, kFixedHdrBits + tot, clcode[l256], b256);
    or_bits(hw, kFixedHdrBits + tot + b256, clcode[0], b257);
  }
  __syncthreads();
  if (tid < kHdrWords) hdr[bi * kHdrWords + tid] = hw[tid];
  if (tid == 0) {
    const uint32_t hbits = kFixedHdrBits + tot + b256 + b257;
    const uint32_t dyn = ((hbits + body + 3u + 7u) >> 3) + 4u;  // + the empty stored block that realigns
    const uint32_t stored = blen + 5u;
    uint32_t* m = meta + bi * kMeta;
    m[0] = dyn > stored ? 0u : hbits;
    m[1] = dyn > stored ? stored : dyn;
    m[2] = S1;
    m[3] = S2;
  }
}

// ---- 3: layout.  grid (n), block 256 ------------------------------------------------------------
// block offsets (from the first block's byte), the file size, Adler-32 of the filtered stream
__global__ __launch_bounds__(256) void png_layout(uint32_t* __restrict__ meta, int nblocks, uint32_t total,
                                                  uint32_t* __restrict__ imeta, long long* __restrict__ sizes) {
  __shared__ uint32_t sh[4];
  const int tid = threadIdx.x, img = blockIdx.x;
  uint32_t* m = meta + (size_t)img * nblocks * kMeta;
  uint32_t off = 0, a = 1;  // bytes before this round's blocks; Adler's A before them
  unsigned long long bsum = 0;
  for (int base = 0; base < nblocks; base += kThreads) {
    const int b = base + tid;
    const bool live = b < nblocks;
    const uint32_t sz = live ? m[b * kMeta + 1] : 0u, s1 = live ? m[b * kMeta + 2] : 0u;
    uint32_t tot_sz = 0, tot_s1 = 0;
    const uint32_t ex_sz = block_excl(sz, sh, &tot_sz);
    const uint32_t ex_s1 = block_excl(s1, sh, &tot_s1);
    if (live) {
      m[b * kMeta + 4] = off + ex_sz;
      const uint32_t blen = min((uint32_t)kBlock, total - (uint32_t)b * kBlock);
      const uint32_t before = (a + ex_s1) % kAdlerMod;
      bsum += (m[b * kMeta + 3] + (unsigned long long)blen * before) % kAdlerMod;
    }
    off += tot_sz;
    a = (a + tot_s1) % kAdlerMod;
  }
  const uint32_t bb = block_sum_mod(bsum, sh);
  if (tid == 0) {
    imeta[2 * img + 0] = off;
    imeta[2 * img + 1] = (bb << 16) | a;
    sizes[img] = (long long)kFraming + off;
  }
}

// ---- 4: emit.  grid (nblocks, n), block 256 -----------------------------------------------------
// The block's bytes are put together in LDS: thread t codes symbols [64 t, 64 t + 64) at the bit
// offset a scan of their code lengths gives, ORing whole words into the buffer; then every thread
// takes the CRC-32 of a run of the bytes (combined by multiplying with x^(8 * bytes after it)) and
// the buffer goes to the file as aligned 32-bit words.
__global__ __launch_bounds__(256) void png_emit(const uint8_t* __restrict__ filt, size_t fstride, uint32_t total, int nblocks,
                                                const uint32_t* __restrict__ tab, const uint32_t* __restrict__ hdr,
                                                uint32_t* __restrict__ meta, uint8_t* __restrict__ out, long long stride) {
  __shared__ uint32_t obuf[kObufWords], code[kTabWords], crct[256], sh[4];
  const int tid = threadIdx.x, b = blockIdx.x, img = blockIdx.y;
  const size_t bi = (size_t)img * nblocks + b;
  uint32_t* m = meta + bi * kMeta;
  const uint32_t blen = min((uint32_t)kBlock, total - (uint32_t)b * kBlock);
  const uint8_t* src = filt + (size_t)img * fstride + (size_t)b * kBlock;
  const uint32_t hbits = m[0], nbytes = min(m[1], blen + 5u), last = b == nblocks - 1 ? 1u : 0u;
  uint8_t* ob = (uint8_t*)obuf;
  {
    uint32_t c = (uint32_t)tid;
#pragma unroll
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    crct[tid] = c;
  }
  for (int i = tid; i < kObufWords; i += kThreads) obuf[i] = (hbits && i < kHdrWords) ? hdr[bi * kHdrWords + i] : 0u;
  for (int i = tid; i < kTabWords; i += kThreads) code[i] = (hbits && i < kLit) ? tab[bi * kTabWords + i] : 0u;
  __syncthreads();
  if (hbits == 0) {  // stored (block-uniform)
    if (tid == 0) {
      ob[0] = (uint8_t)last;
      ob[1] = (uint8_t)(blen & 255u);
      ob[2] = (uint8_t)(blen >> 8);
      ob[3] = (uint8_t)(~blen & 255u);
      ob[4] = (uint8_t)((~blen >> 8) & 255u);
    }
    for (uint32_t i = tid; i < blen; i += kThreads) ob[5 + i] = src[i];
  } else {
    const uint32_t s0 = (uint32_t)tid * kRun;
    const uint32_t mine = s0 < blen ? min((uint32_t)kRun, blen - s0) : 0u;
    const bool eob = mine > 0 && s0 + mine == blen;  // the thread of the last symbol appends end-of-block
    uint32_t w[kRun / 4];
#pragma unroll
    for (int q = 0; q < kRun / 16; ++q) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (s0 + 16u * q < blen) v = *(const uint4*)(src + s0 + 16 * q);  // inside fstride, as in png_codes
      w[4 * q + 0] = v.x;
      w[4 * q + 1] = v.y;
      w[4 * q + 2] = v.z;
      w[4 * q + 3] = v.w;
    }
    uint32_t bits = eob ? code[256] >> 16 : 0u;
#pragma unroll
    for (int i = 0; i < kRun; ++i)
      if ((uint32_t)i < mine) bits += code[(w[i >> 2] >> (8 * (i & 3))) & 255u] >> 16;
    uint32_t tot = 0;
    const uint32_t pos = hbits + block_excl(bits, sh, &tot);
    uint32_t wi = pos >> 5, nb = pos & 31u;
    unsigned long long acc = 0;
    auto put = [&](uint32_t e) {
      acc |= (unsigned long long)(e & 0xffffu) << nb;
      nb += e >> 16;
      if (nb >= 32u) {
        if (wi < (uint32_t)kObufWords) atomicOr(&obuf[wi], (uint32_t)acc);
        acc >>= 32;
        nb -= 32u;
        ++wi;
      }
    };
#pragma unroll
    for (int i = 0; i < kRun; ++i)
      if ((uint32_t)i < mine) put(code[(w[i >> 2] >> (8 * (i & 3))) & 255u]);
    if (eob) put(code[256]);
    if (nb > 0 && (uint32_t)acc && wi < (uint32_t)kObufWords) atomicOr(&obuf[wi], (uint32_t)acc);
    if (tid == 0) {
      // the empty stored block after end-of-block: BFINAL, BTYPE 0, zero bits to the byte, 00 00 FF FF
      const uint32_t d = hbits + tot, p = (d + 3u + 7u) >> 3;
      if (last) atomicOr(&obuf[d >> 5], 1u << (d & 31u));
      atomicOr(&obuf[(p + 2) >> 2], 0xffu << (8 * ((p + 2) & 3u)));
      atomicOr(&obuf[(p + 3) >> 2], 0xffu << (8 * ((p + 3) & 3u)));
    }
  }
  __syncthreads();
  // CRC-32 of the block's bytes
  const uint32_t chunk = (nbytes + kThreads - 1) / kThreads;
  const uint32_t beg = min((uint32_t)tid * chunk, nbytes), end = min(beg + chunk, nbytes);
  uint32_t c = 0xffffffffu;
  for (uint32_t i = beg; i < end; ++i) c = crct[(c ^ ob[i]) & 255u] ^ (c >> 8);
  c ^= 0xffffffffu;
  c = c ? gf_mul(c, gf_x8n(nbytes - end)) : 0u;
  c = block_xor(c, sh);
  if (tid == 0) m[5] = c;
  // the bytes into the file: head bytes up to a 4-byte boundary, words, tail bytes
  const size_t at = (size_t)kPayloadAt + m[4];
  if ((long long)(at + nbytes) + 20 > stride) return;  // never: stride >= nic_png_device_bound
  uint8_t* dst = out + (size_t)img * (size_t)stride + at;
  const uint32_t head = min((uint32_t)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u), nbytes);
  if ((uint32_t)tid < head) dst[tid] = ob[tid];
  const uint32_t nw = (nbytes - head) >> 2, shb = 8u * head;
  uint32_t* dw = (uint32_t*)(dst + head);
  for (uint32_t k = tid; k < nw; k += kThreads) dw[k] = shb ? (obuf[k] >> shb) | (obuf[k + 1] << (32u - shb)) : obuf[k];
  for (uint32_t i = head + 4u * nw + tid; i < nbytes; i += kThreads) dst[i] = ob[i];
}

// ---- 5: finish.  grid (n), block 256 --------------------------------------------------------------
__global__ __launch_bounds__(256) void png_finish(const uint32_t* __restrict__ meta, int nblocks, const uint32_t* __restrict__ imeta,
                                                  int h, int w, int channels, uint8_t* __restrict__ out, long long stride) {
  __shared__ uint32_t sh[4];
  const int tid = threadIdx.x, img = blockIdx.x;
  const uint32_t* m = meta + (size_t)img * nblocks * kMeta;
  const uint32_t pay = imeta[2 * img], adler = imeta[2 * img + 1];
  const uint32_t idat = 2u + pay + 4u;  // the IDAT chunk's data bytes
  uint32_t c = 0;
  for (int b = tid; b < nblocks; b += kThreads) {
    const uint32_t after = pay - m[b * kMeta + 4] - m[b * kMeta + 1] + 4u;
    c ^= gf_mul(m[b * kMeta + 5], gf_x8n(after));
  }
  uint8_t ihdr[17] = {'I', 'H', 'D', 'R', (uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w,
                      (uint8_t)(h >> 24), (uint8_t)(h >> 16), (uint8_t)(h >> 8), (uint8_t)h,
                      8, (uint8_t)(channels == 3 ? 2 : 0), 0, 0, 0};
  uint32_t ihdr_crc = 0;
  if (tid == 0) {
    const uint8_t first[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};  // chunk type + zlib header (window 15, FCHECK 1)
    uint32_t r = 0xffffffffu;
    for (int i = 0; i < 6; ++i) r = crc_byte(r, first[i]);
    c ^= gf_mul(r ^ 0xffffffffu, gf_x8n(idat - 2u));
    r = 0xffffffffu;
    for (int i = 0; i < 4; ++i) r = crc_byte(r, (adler >> (24 - 8 * i)) & 255u);
    c ^= r ^ 0xffffffffu;
    r = 0xffffffffu;
    for (int i = 0; i < 17; ++i) r = crc_byte(r, ihdr[i]);
    ihdr_crc = r ^ 0xffffffffu;
  }
  c = block_xor(c, sh);
  if (tid != 0 || (long long)kFraming + pay > stride) return;
  uint8_t* f = out + (size_t)img * (size_t)stride;
  auto be32 = [](uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
  };
  const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  for (int i = 0; i < 8; ++i) f[i] = sig[i];
  be32(f + 8, 13u);
  for (int i = 0; i < 17; ++i) f[12 + i] = ihdr[i];
  be32(f + 29, ihdr_crc);
  be32(f + 33, idat);
  f[37] = 'I';
  f[38] = 'D';
  f[39] = 'A';
  f[40] = 'T';
  f[41] = 0x78;
  f[42] = 0x01;
  uint8_t* t = f + kPayloadAt + pay;
  be32(t, adler);
  be32(t + 4, c);
  be32(t + 8, 0u);
  t[12] = 'I';
  t[13] = 'E';
  t[14] = 'N';
  t[15] = 'D';
  be32(t + 16, 0xae426082u);
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

bool png_dev_shape_ok(int h, int w, int channels) {
  // nic_png_encode's limits: rows of at most 16,384 bytes, images under 1 GB of filtered bytes
  return h >= 1 && w >= 1 && (long long)w * channels <= 16384 && (long long)h * ((long long)w * channels + 1) <= (1ll << 30);
}

void png_dev_plan(int n, int h, int w, int channels, PngDevPlan* pl) {
  const size_t N = (size_t)n;
  pl->total = (uint32_t)((size_t)h * ((size_t)w * channels + 1));
  pl->nblocks = (int)((pl->total + kBlock - 1) / kBlock);
  pl->fstride = align256((size_t)pl->total + 16);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  pl->filt = take(N * pl->fstride);
  pl->tab = take(N * pl->nblocks * kTabWords * 4);
  pl->hdr = take(N * pl->nblocks * kHdrWords * 4);
  pl->meta = take(N * pl->nblocks * kMeta * 4);
  pl->imeta = take(N * 2 * 4);
  pl->bytes = o;
}

hipError_t launch_png_dev_encode(const uint8_t* images, int n, int h, int w, int channels, int filter, char* ws,
                                 const PngDevPlan& pl, uint8_t* out, long long stride, long long* sizes, hipStream_t st) {
  const int wb = w * channels, nb = pl.nblocks;
  uint8_t* filt = (uint8_t*)(ws + pl.filt);
  uint32_t* tab = (uint32_t*)(ws + pl.tab);
  uint32_t* hdr = (uint32_t*)(ws + pl.hdr);
  uint32_t* meta = (uint32_t*)(ws + pl.meta);
  uint32_t* imeta = (uint32_t*)(ws + pl.imeta);
  png_filter<<<dim3((h + 3) / 4, n), 256, 0, st>>>(images, h, wb, channels, filter, filt, pl.fstride);
  png_codes<<<dim3(nb, n), 256, 0, st>>>(filt, pl.fstride, pl.total, nb, tab, hdr, meta);
  png_layout<<<dim3(n), 256, 0, st>>>(meta, nb, pl.total, imeta, sizes);
  png_emit<<<dim3(nb, n), 256, 0, st>>>(filt, pl.fstride, pl.total, nb, tab, hdr, meta, out, stride);
  png_finish<<<dim3(n), 256, 0, st>>>(meta, nb, imeta, h, w, channels, out, stride);
  return hipGetLastError();
}

}  // namespace nic

// ---- host-only entry points ------------------------------------------------------------------

extern "C" {

int nic_png_device_block_bytes(void) { return nic::kBlock; }

int nic_png_device_bound(int h, int w, int channels, int64_t* bytes) {
  if (!bytes) return nic::set_error(NIC_EINVAL, "nic_png_device_bound: bytes is NULL");
  if (channels != 1 && channels != 3) return nic::set_error(NIC_EINVAL, "nic_png_device_bound: channels must be 1 or 3");
  if (!nic::png_dev_shape_ok(h, w, channels))
    return nic::set_error(NIC_ESHAPE, "nic_png_device_bound: bad image shape, rows wider than 16384 bytes or images above 1 GB");
  const int64_t total = (int64_t)h * ((int64_t)w * channels + 1), nblocks = (total + nic::kBlock - 1) / nic::kBlock;
  // the framing and every block stored: a block is coded dynamically only where that is no larger
  *bytes = nic::kFraming + total + 5 * nblocks;
  return NIC_OK;
}

}  // extern "C"
