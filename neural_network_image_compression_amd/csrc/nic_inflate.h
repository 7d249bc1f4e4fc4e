// Inflate (RFC 1950 / 1951) of one zlib stream, written once for the device PNG reader's kernel
// (nic_png_read.hip) and for the CPU (tools/png_read_host_check.cpp): everything that indexes by
// untrusted data lives here -- the bit reader, the code-length decoder, the table builder, the
// symbol decode and the match bounds check -- so the CPU build exercises the kernel's own source.
//
// The caller supplies an Env:
//   int lane(), lanes()            this thread's place among the threads that run the call together
//                                  (the CPU: 0 of 1; the kernel: a wave, every lane running the same
//                                  control flow on the same values)
//   void sync()                    orders the threads' table / window accesses (CPU: nothing)
//   uint32_t in_byte(uint32_t pos) input byte pos; only called with pos < size
//   void put(at, byte)             output byte at; only called with at < T
//   void copy_match(at, dist, len) out[at + i] = out[at - dist + i mod dist] for i < len; only called
//                                  with 1 <= dist <= at and at + len <= T
//   void copy_stored(at, pos, len) out[at + i] = in[pos + i]; only called with pos + len <= size and
//                                  at + len <= T
// Bounds (every loop's trip count is known before it starts):
//   - the block loop and the symbol loop stop as soon as the bits consumed exceed 8 * size, and every
//     iteration consumes at least one bit: at most 8 * size + 1 iterations in all (counted in *iters)
//   - the code-length loop runs at most HLIT + HDIST <= 316 times, the table loops over <= 288 symbols,
//     16 lengths or 1 << kFastBits entries
//   - every input read is clamped to size (bytes past it read as 0 and count as exhaustion), every
//     table index is masked or clamped to its table, every output index is checked against T first
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NIC_HD __host__ __device__ inline
#else
#define NIC_HD inline
#endif

namespace nic {
namespace inflate {

// status bits of nic_png_device_read (include/nic.h)
enum : int { kStHeader = 1, kStData = 2, kStLength = 4, kStAdler = 8, kStFilter = 16 };

constexpr int kFastBits = 10;   // first-level lookup; longer codes walk the canonical counts
constexpr int kFastSize = 1 << kFastBits;
constexpr int kMaxLit = 288;    // symbols of the literal/length code (fixed code: 288)
constexpr int kLensAt = 0;      // lens[]: literal/length + distance lengths (<= 318) ...
constexpr int kClAt = 320;      // ... and the 19 lengths of the code-length code
constexpr int kLensSize = 344;

struct Huff {
  uint16_t count[16];          // codes of each length
  uint16_t first[16];          // first canonical code of each length
  uint16_t start[16];          // index in symbol[] of the first symbol of each length
  uint16_t offs[16];           // running copy of start[] while the symbols are placed
  uint16_t symbol[kMaxLit];    // symbols in canonical order
  uint16_t fast[kFastSize];    // low kFastBits of the stream -> symbol << 4 | length (0: not here)
};

struct Bits {
  uint64_t buf = 0;   // unread bits, LSB first
  uint32_t cnt = 0;   // how many
  uint64_t pos = 0;   // next input byte to load (runs past size: those bytes read as 0)
  uint32_t size = 0;
};

template <class Env>
NIC_HD void refill(Env& env, Bits& b) {  // afterwards cnt >= 32
  if (b.cnt < 32u) {
    uint32_t w = 0;
    for (int k = 0; k < 4; ++k) {
      const uint64_t p = b.pos + (uint64_t)k;
      const uint32_t v = p < (uint64_t)b.size ? (env.in_byte((uint32_t)p) & 255u) : 0u;
      w |= v << (8 * k);
    }
    b.buf |= (uint64_t)w << b.cnt;
    b.cnt += 32u;
    b.pos += 4u;
  }
}
NIC_HD uint32_t peek(const Bits& b, uint32_t n) { return (uint32_t)b.buf & ((1u << n) - 1u); }  // n <= 16 <= cnt
NIC_HD void drop(Bits& b, uint32_t n) {
  n = n < b.cnt ? n : b.cnt;
  b.buf >>= n;
  b.cnt -= n;
}
NIC_HD uint64_t consumed(const Bits& b) { return 8u * b.pos - b.cnt; }
NIC_HD bool exhausted(const Bits& b) { return consumed(b) > 8ull * b.size; }
template <class Env>
NIC_HD uint32_t take(Env& env, Bits& b, uint32_t n) {  // n <= 16
  refill(env, b);
  const uint32_t v = peek(b, n);
  drop(b, n);
  return v;
}

NIC_HD uint32_t bit_reverse(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < 15; ++i)
    if (i < len) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

enum : int { kCodes = 0, kLens = 1, kDists = 2 };

// The decoding tables of the canonical code with lengths lens[0..n), n <= 288.  check: judge the set
// as zlib's inflate_table does -- an over-subscribed set is refused, an incomplete one too unless it
// is a literal/length or distance set whose longest code has one bit; a set without codes is taken
// (a symbol decoded with it has no code).  false: refused.
template <class Env>
NIC_HD bool build_huff(Env& env, Huff& h, const uint8_t* lens, int n, int type, bool check) {
  n = n < 0 ? 0 : (n > kMaxLit ? kMaxLit : n);
  env.sync();
  if (env.lane() == 0) {
    for (int l = 0; l < 16; ++l) h.count[l] = 0;
    for (int s = 0; s < n; ++s) h.count[lens[s] & 15] += 1;
    uint32_t code = 0, idx = 0;
    h.first[0] = h.start[0] = h.offs[0] = 0;
    for (int l = 1; l < 16; ++l) {
      h.first[l] = (uint16_t)code;
      h.start[l] = h.offs[l] = (uint16_t)idx;
      code = (code + h.count[l]) << 1;
      idx += h.count[l];
    }
    for (int s = 0; s < n; ++s) {
      const int l = lens[s] & 15;
      if (l) {
        const uint32_t at = h.offs[l]++;
        h.symbol[at < (uint32_t)kMaxLit ? at : (uint32_t)kMaxLit - 1] = (uint16_t)s;
      }
    }
  }
  for (int e = env.lane(); e < kFastSize; e += env.lanes()) h.fast[e] = 0;
  env.sync();
  int left = 1, maxlen = 0, total = 0;
  bool over = false;
  for (int l = 1; l < 16; ++l) {
    const int c = h.count[l];
    left = (left << 1) - c;
    if (left < 0) {
      over = true;
      left = 0;
    }
    if (c) maxlen = l;
    total += c;
  }
  if (check && maxlen != 0 && (over || (left > 0 && (type == kCodes || maxlen != 1)))) return false;
  if (over) return false;  // never with the fixed code
  for (int j = env.lane(); j < total && j < kMaxLit; j += env.lanes()) {
    int l = 0;
    for (int k = 1; k <= kFastBits; ++k)
      if (j >= (int)h.start[k] && j < (int)h.start[k] + (int)h.count[k]) l = k;
    if (l) {
      const uint32_t rev = bit_reverse((uint32_t)h.first[l] + (uint32_t)(j - (int)h.start[l]), l);
      const uint16_t e = (uint16_t)(((uint32_t)h.symbol[j] << 4) | (uint32_t)l);
      for (uint32_t k = rev; k < (uint32_t)kFastSize; k += 1u << l) h.fast[k & (kFastSize - 1)] = e;
    }
  }
  env.sync();
  return true;
}

// One symbol: consumes its code's 1..15 bits; -1 (nothing consumed): the bits are no code of h.
template <class Env>
NIC_HD int decode_sym(Env& env, Bits& b, const Huff& h) {
  refill(env, b);
  const uint32_t e = h.fast[peek(b, kFastBits) & (kFastSize - 1)];
  if (e) {
    drop(b, e & 15u);
    return (int)(e >> 4);
  }
  const uint32_t v = peek(b, 15);
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)((v >> (l - 1)) & 1u);
    const int c = h.count[l];
    if (code - c < first) {
      drop(b, (uint32_t)l);
      const int at = index + (code - first);
      return h.symbol[at < 0 ? 0 : (at < kMaxLit ? at : kMaxLit - 1)];
    }
    index += c;
    first += c;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

NIC_HD int cl_order(int k) {  // deflate's order of the code-length code's own lengths, k in 0..18
  const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                      10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (int)((k < 12 ? lo >> (5 * k) : hi >> (5 * (k - 12))) & 31u);
}

// The code lengths of a dynamic block's header into lens[0..hlit + hdist) and both tables.  0 or kStData.
template <class Env>
NIC_HD int read_dynamic(Env& env, Bits& b, Huff& lit, Huff& dst, uint8_t* lens) {
  refill(env, b);
  const int hlit = (int)peek(b, 5) + 257, hdist = (int)(peek(b, 10) >> 5) + 1, hclen = (int)(peek(b, 14) >> 10) + 4;
  drop(b, 14);
  if (hlit > 286 || hdist > 30) return kStData;
  env.sync();
  if (env.lane() == 0)
    for (int k = 0; k < 19; ++k) lens[kClAt + k] = 0;
  for (int k = 0; k < hclen; ++k) {  // hclen <= 19
    const uint32_t v = take(env, b, 3);
    if (env.lane() == 0) lens[kClAt + cl_order(k)] = (uint8_t)v;
  }
  if (!build_huff(env, lit, lens + kClAt, 19, kCodes, true)) return kStData;  // lit holds the code-length code for now
  const int total = hlit + hdist;  // <= 316
  int i = 0, last = -1, len256 = 0;
  for (int it = 0; it < total && i < total; ++it) {  // every pass adds at least one length
    const int s = decode_sym(env, b, lit);
    if (s < 0 || s > 18) return kStData;
    int rep = 1, val = s;
    if (s == 16) {
      if (last < 0) return kStData;  // repeat with no previous length
      val = last;
      rep = 3 + (int)take(env, b, 2);
    } else if (s == 17) {
      val = 0;
      rep = 3 + (int)take(env, b, 3);
    } else if (s == 18) {
      val = 0;
      rep = 11 + (int)take(env, b, 7);
    }
    if (i + rep > total) return kStData;
    if (i <= 256 && 256 < i + rep) len256 = val;
    if (env.lane() == 0)
      for (int k = 0; k < rep; ++k) lens[(i + k) < kClAt ? (i + k) : kClAt - 1] = (uint8_t)val;
    i += rep;
    last = val;
    if (exhausted(b)) return kStData;
  }
  if (i != total) return kStData;
  if (len256 == 0) return kStData;  // no end-of-block code
  if (!build_huff(env, lit, lens, hlit, kLens, true)) return kStData;
  if (!build_huff(env, dst, lens + hlit, hdist, kDists, true)) return kStData;
  return 0;
}

template <class Env>
NIC_HD void build_fixed(Env& env, Huff& lit, Huff& dst, uint8_t* lens) {
  env.sync();
  if (env.lane() == 0) {
    for (int s = 0; s < 288; ++s) lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (int s = 0; s < 30; ++s) lens[288 + s] = 5;
  }
  build_huff(env, lit, lens, 288, kLens, false);
  build_huff(env, dst, lens + 288, 30, kDists, false);
}

// A match may be copied iff it starts inside the bytes produced so far and ends inside the output.
NIC_HD int match_check(uint32_t out, uint32_t T, uint32_t dist, uint32_t len) {
  if (dist == 0 || dist > out) return kStData;
  if (len > T - out) return kStLength;
  return 0;
}

// The whole stream in[0..size) -> exactly T output bytes through env; the status bits 1, 2 and 4, and
// for status 0 the stream's Adler-32 field in *adler.  *iters (nullable): block + symbol iterations.
template <class Env>
NIC_HD int inflate_stream(Env& env, Huff& lit, Huff& dst, uint8_t* lens, uint32_t size, uint32_t T, uint32_t* adler,
                          uint64_t* iters) {
  Bits b;
  b.size = size;
  uint64_t it = 0;
  const uint64_t bound = 8ull * size + 1;
  uint32_t out = 0;
  *adler = 0;
  if (iters) *iters = 0;
  const uint32_t cmf = take(env, b, 8), flg = take(env, b, 8);
  if (size < 2 || (cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return kStHeader;
  int status = 0;
  bool final = false;
  while (!final && status == 0) {
    if (++it > bound || exhausted(b)) {
      status = kStData;
      break;
    }
    refill(env, b);
    final = peek(b, 1) != 0;
    const uint32_t type = peek(b, 3) >> 1;
    drop(b, 3);
    if (type == 3) {
      status = kStData;
    } else if (type == 0) {
      drop(b, b.cnt & 7u);  // to the byte boundary
      const uint32_t len = take(env, b, 16), nlen = take(env, b, 16);
      if (exhausted(b) || (len ^ nlen) != 0xffffu) {
        status = kStData;
        break;
      }
      const uint64_t at = consumed(b) >> 3;
      if (at + len > (uint64_t)size) {
        status = kStData;
        break;
      }
      if (len > T - out) {
        status = kStLength;
        break;
      }
      if (len) env.copy_stored(out, (uint32_t)at, len);
      out += len;
      b.buf = 0;
      b.cnt = 0;
      b.pos = at + len;
    } else {
      if (type == 1)
        build_fixed(env, lit, dst, lens);
      else
        status = read_dynamic(env, b, lit, dst, lens);
      while (status == 0) {
        if (++it > bound || exhausted(b)) {
          status = kStData;
          break;
        }
        const int s = decode_sym(env, b, lit);
        if (s < 0) {
          status = kStData;
        } else if (s < 256) {
          if (out >= T) {
            status = kStLength;
          } else {
            env.put(out, (uint32_t)s);
            ++out;
          }
        } else if (s == 256) {
          break;
        } else {
          const int idx = s - 257;
          if (idx > 28) {
            status = kStData;
            break;
          }
          const uint32_t lx = idx < 8 || idx == 28 ? 0u : (uint32_t)(idx - 4) >> 2;
          uint32_t len = idx < 8 ? 3u + idx : idx == 28 ? 258u : 3u + ((4u + (idx & 3u)) << lx);
          len += take(env, b, lx);
          const int d = decode_sym(env, b, dst);
          if (d < 0 || d > 29) {
            status = kStData;
            break;
          }
          const uint32_t dx = d < 4 ? 0u : (uint32_t)(d - 2) >> 1;
          uint32_t dist = d < 4 ? 1u + d : 1u + ((2u + (d & 1u)) << dx);
          dist += take(env, b, dx);
          if (exhausted(b)) {
            status = kStData;
            break;
          }
          status = match_check(out, T, dist, len);
          if (status == 0) {
            env.copy_match(out, dist, len);
            out += len;
          }
        }
      }
    }
  }
  if (iters) *iters = it;
  if (status) return status;
  if (exhausted(b)) return kStData;
  if (out != T) return kStLength;
  drop(b, b.cnt & 7u);
  if ((consumed(b) >> 3) + 4 > (uint64_t)size) return kStLength;  // zlib: the stream ends before its check value
  uint32_t a = 0;
  for (int k = 0; k < 4; ++k) a = (a << 8) | take(env, b, 8);
  *adler = a;
  return 0;
}

// Adler-32 from s1 = sum of bytes and s2 = sum of (T - i) * byte[i], both already modulo 65521
NIC_HD uint32_t adler_from_sums(uint32_t s1, uint32_t s2, uint32_t T) {
  const uint32_t a = (1u + s1) % 65521u, bb = (T % 65521u + s2) % 65521u;
  return (bb << 16) | a;
}

}  // namespace inflate
}  // namespace nic
