// Rate-distortion optimised quantisation against the .nic priors (rule: DESIGN.md §25; entry point:
// include/nic.h nic_rdoq).  Every latent byte has two candidates, the plain code r and its neighbour
// alt on the side of the pre-quant value v = f * 255, and the code kept is the one with the smaller
// D + lam_fix * cost16[freq], all in u64 after two fp32 operations per candidate.
//
// rdoq_static: the static prior (version 2).  Every byte is decided on its own; one thread takes four
//   consecutive bytes (96 = 24 x 4, so the four are of one pixel): one dword of codes, one 16-B load of
//   pre-quant values, one dword stored.
// rdoq_trellis: the context prior (version 3).  The row of a byte is chosen by the code kept for the
//   pixel before it, so a (segment, channel) chain is a two-state Viterbi pass.  One lane walks one
//   chain: lane = chain index = (image, segment) * 96 + channel, so the 64 lanes of a wave read 64
//   consecutive bytes / floats of one pixel at every step (a wave straddles at most two segments).
//   The back-pointers of the two states are one bit each per pixel: two u64 masks per lane, which is
//   why seg_pixels <= 64; two more masks keep the direction of alt, so the write pass needs r alone.
//
// The rows stay in global memory: a wave's lanes are at 64 different channels, so no row is shared
// inside a wave, the context prior's 147 KB of freqs and the 16 KB cost table are L2-resident, and
// the lookups of a channel cluster at its anchor.  No LDS, no atomics, plain vector loads and stores.

#include <hip/hip_runtime.h>

#include "nic_kernels.h"

namespace nic {

namespace {

constexpr int kCh = 96;
constexpr int kCtx = 3;

// One byte's two candidates and their distortions.  v - q is recomputed for alt; the products are
// separately rounded (the __f*_rn forms are never contracted).  alt is kept inside 0..255 whatever f
// holds (a code and its own pre-quant value never leave it), so every table index is in bounds.
struct Cand {
  int q[2];
  unsigned long long d[2];
};

__device__ __forceinline__ unsigned long long rdoq_dist(float e) {
  return (unsigned long long)rintf(__fmul_rn(__fmul_rn(e, e), 65536.0f)) << 16;
}

__device__ __forceinline__ Cand rdoq_cand(int r, float f) {
  const float v = __fmul_rn(f, 255.0f);
  const float e = __fsub_rn(v, (float)r);
  int alt = r + (e > 0.0f ? 1 : 0) - (e < 0.0f ? 1 : 0);
  alt = alt < 0 ? 0 : (alt > 255 ? 255 : alt);
  Cand c;
  c.q[0] = r;
  c.q[1] = alt;
  c.d[0] = rdoq_dist(e);
  c.d[1] = rdoq_dist(__fsub_rn(v, (float)alt));
  return c;
}

// groups: n * h8 * w8 * 24 groups of four bytes
__global__ __launch_bounds__(256) void rdoq_static(const uint8_t* __restrict__ z, const float* __restrict__ f, long long groups,
                                                   unsigned lam_fix, const uint16_t* __restrict__ freq,
                                                   const uint32_t* __restrict__ cost16, uint8_t* __restrict__ out) {
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
    const uint32_t r4 = ((const uint32_t*)z)[g];
    const float4 f4 = ((const float4*)f)[g];
    const float fv[4] = {f4.x, f4.y, f4.z, f4.w};
    const int c0 = (int)(g % (kCh / 4)) * 4;
    uint32_t o4 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const Cand c = rdoq_cand((int)((r4 >> (8 * j)) & 255u), fv[j]);
      const uint16_t* row = freq + (c0 + j) * 256;
      const unsigned long long j0 = c.d[0] + (unsigned long long)lam_fix * cost16[row[c.q[0]]];
      const unsigned long long j1 = c.d[1] + (unsigned long long)lam_fix * cost16[row[c.q[1]]];
      o4 |= (uint32_t)(j1 < j0 ? c.q[1] : c.q[0]) << (8 * j);  // a tie goes to r
    }
    ((uint32_t*)out)[g] = o4;
  }
}

__device__ __forceinline__ int rdoq_ctx(int q, int anchor) {
  const int d = q > anchor ? q - anchor : anchor - q;
  return d < 2 ? d : 2;
}

// chains: n * nseg * 96; freq [96][3][256]
__global__ __launch_bounds__(256) void rdoq_trellis(const uint8_t* __restrict__ z, const float* __restrict__ f, int npix,
                                                    int seg_pixels, int nseg, long long chains, unsigned lam_fix,
                                                    const uint16_t* __restrict__ freq, const uint8_t* __restrict__ anchors,
                                                    const uint32_t* __restrict__ cost16, uint8_t* __restrict__ out) {
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < chains; g += (long long)gridDim.x * 256) {
    const int ch = (int)(g % kCh);
    const long long sg = g / kCh;
    const int seg = (int)(sg % nseg);
    const long long img = sg / nseg;
    const int first = seg * seg_pixels;
    const int len = min(seg_pixels, npix - first);  // 1..64
    const long long at = (img * npix + first) * kCh + ch;  // the chain's first byte; the next is 96 on
    const int anchor = anchors[ch];
    const uint16_t* rows = freq + ch * kCtx * 256;
    auto rate = [&](int k, int q) { return (unsigned long long)lam_fix * cost16[rows[k * 256 + q]]; };

    unsigned long long back0 = 0, back1 = 0;  // bit p: the state before pixel p's state b
    unsigned long long up = 0, down = 0;      // bit p: alt = r + 1 / r - 1 (neither: alt = r)
    unsigned long long best0, best1;
    int prev0, prev1;
    {
      const Cand c = rdoq_cand(z[at], f[at]);
      best0 = c.d[0] + rate(0, c.q[0]);
      best1 = c.d[1] + rate(0, c.q[1]);
      up |= (unsigned long long)(c.q[1] > c.q[0]);
      down |= (unsigned long long)(c.q[1] < c.q[0]);
      prev0 = c.q[0];
      prev1 = c.q[1];
    }
    for (int p = 1; p < len; ++p) {
      const long long i = at + (long long)p * kCh;
      const Cand c = rdoq_cand(z[i], f[i]);
      const int k0 = rdoq_ctx(prev0, anchor), k1 = rdoq_ctx(prev1, anchor);
      const unsigned long long a00 = best0 + rate(k0, c.q[0]), a10 = best1 + rate(k1, c.q[0]);
      const unsigned long long a01 = best0 + rate(k0, c.q[1]), a11 = best1 + rate(k1, c.q[1]);
      const bool t0 = a10 < a00, t1 = a11 < a01;  // a tie goes to the state of r
      best0 = c.d[0] + (t0 ? a10 : a00);
      best1 = c.d[1] + (t1 ? a11 : a01);
      back0 |= (unsigned long long)t0 << p;
      back1 |= (unsigned long long)t1 << p;
      up |= (unsigned long long)(c.q[1] > c.q[0]) << p;
      down |= (unsigned long long)(c.q[1] < c.q[0]) << p;
      prev0 = c.q[0];
      prev1 = c.q[1];
    }
    unsigned long long pick = 0;  // bit p: pixel p keeps alt
    unsigned b = best1 < best0;
    for (int p = len - 1; p >= 0; --p) {
      pick |= (unsigned long long)b << p;
      b = (unsigned)(((b ? back1 : back0) >> p) & 1ull);
    }
    const unsigned long long plus = pick & up, minus = pick & down;
    for (int p = 0; p < len; ++p) {
      const long long i = at + (long long)p * kCh;
      out[i] = (uint8_t)((int)z[i] + (int)((plus >> p) & 1ull) - (int)((minus >> p) & 1ull));
    }
  }
}

constexpr long long kMaxBlocks = 1 << 20;  // the kernels stride over the rest

}  // namespace

hipError_t launch_rdoq(const uint8_t* z, const float* f, int n, int h8, int w8, int seg_pixels, unsigned lam_fix,
                       const RansPrior& pr, uint8_t* out, hipStream_t st) {
  const int npix = h8 * w8;
  if (pr.anchor) {
    const int nseg = (npix + seg_pixels - 1) / seg_pixels;
    const long long chains = (long long)n * nseg * kCh;
    const long long blocks = (chains + 255) / 256;
    rdoq_trellis<<<dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), 256, 0, st>>>(
        z, f, npix, seg_pixels, nseg, chains, lam_fix, pr.freq, pr.anchor, pr.cost16, out);
  } else {
    const long long groups = (long long)n * npix * (kCh / 4);
    const long long blocks = (groups + 255) / 256;
    rdoq_static<<<dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), 256, 0, st>>>(z, f, groups, lam_fix, pr.freq,
                                                                                            pr.cost16, out);
  }
  return hipGetLastError();
}

}  // namespace nic
