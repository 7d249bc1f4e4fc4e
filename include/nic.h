/*
 * nic.h -- C-ABI of the MI355X-native learned-image-codec hot path.
 *
 * Drop-in boundary for the reference's TF2 codec surface
 * (AlexFuster/Neural_network_image_compression, tf2_0/src):
 *
 *   reference                                   replaced by
 *   ------------------------------------------  -----------------------------------------
 *   Encoder()/Decoder() + ProClass.load(path)   nic_create + nic_set_weights
 *     encoder.py:34-36, decoder.py:35-37,
 *     utils.py:15-17, 26-28
 *   Encoder.__call__(x) encoder.py:38-47        nic_encode (device) / nic_encode_host (NumPy)
 *   Decoder.__call__(z) decoder.py:39-48        nic_decode (device) / nic_decode_host (NumPy)
 *   ProClass._feed_batch pack/unpack            nic_pack_latent / nic_unpack_latent
 *     utils.py:35-36, 39-40
 *   disc_entropy tf1_13/src/training.py:66-71   nic_entropy_hist (nic_encode_entropy: fused
 *                                                 into the encoder's conv8)
 *   tf.image.ssim_multiscale(x1, x2, 255)       nic_ms_ssim
 *     tf2_0/tests/calc_ssim.py:13
 *   PSNR (the benchmark's quality figure)       nic_sq_err
 *   Training step convolutions, forward and     nic_conv_gather / nic_conv_wgrad /
 *     backward (tf2_0/src/training.py:74-151,     nic_absmax_scale / nic_gauss_1d
 *     Keras Conv2D / Conv2DTranspose SAME, SSIM)  (training side path)
 *   Training step optimiser (training.py:147-149, nic_adam_keras
 *     tf.keras Adam)
 *
 * Conventions
 *  - Every buffer argument is a DEVICE pointer owned by the caller (e.g. a torch-ROCm
 *    tensor's data_ptr()); inputs are never written.  The library owns only the weights
 *    and a scratch workspace inside the nic_ctx, grown on demand (call nic_reserve to
 *    size it ahead so no allocation happens in a timed or graph-captured call).
 *  - Work is enqueued asynchronously on the caller's hipStream_t (NULL = default
 *    stream).  One nic_ctx must not be used by two threads at once; distinct contexts
 *    are independent.  There is no global mutable state besides the per-thread error.
 *  - One nic_ctx on several streams of one thread: the caller orders the ctx's calls across
 *    streams.  The workspace, the histogram and MS-SSIM scratch and the range-guard word belong
 *    to the ctx, not to a stream, and no call records or waits on an event for another stream
 *    (nic_encode_host / nic_decode_host alone order their own three streams behind `stream`).
 *    A call on stream 2 may follow a call of the same ctx on stream 1 once stream 2 waits for
 *    that call (hipStreamWaitEvent, torch's wait_stream); unordered, the two share scratch and
 *    race.  Calls that take no ctx (nic_sq_err, nic_pack_latent, the training side path) use
 *    only their arguments and need no such order.  tests/test_gpu_stream_contract.py holds
 *    every entry point to "on `stream`, no host synchronisation" (DESIGN.md section 24).
 *  - Layouts are NHWC uint8: images (N, H, W, 3); latents (N, ceil(H/8), ceil(W/8), 96)
 *    with channels Y0..31, Cb0..31, Cr0..31 (encoder.py:45).  Sizes need not be multiples
 *    of 8: like the reference, decode returns (N, 8h, 8w, 3).
 *  - Return 0 on success or a negative NIC_E* code; nic_last_error() describes the most
 *    recent failure on the calling thread.
 */
#ifndef NIC_H_
#define NIC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nic_ctx nic_ctx;

enum {
  NIC_OK = 0,
  NIC_EINVAL = -1,      /* null pointer, bad enum, bad layer name          */
  NIC_ESHAPE = -2,      /* tensor shape does not match the architecture    */
  NIC_ENOWEIGHTS = -3,  /* encode/decode before every tensor was set       */
  NIC_EHIP = -4,        /* HIP runtime error                               */
  NIC_ENOMEM = -5,      /* device allocation failed                        */
  NIC_ERANGE = -6,      /* NIC_RANGE_ERROR: a split-f16 activation left the f16 range */
  NIC_ECORRUPT = -7,    /* nic_rans_inspect: not a well-formed .nic file              */
  NIC_ENOPRIOR = -8,    /* nic_rans2_encode / nic_rans2_decode before nic_rans_prior_set */
  NIC_EUNSUPPORTED = -9 /* nic_png_inspect: a well-formed PNG of a kind the device reader does not take */
};

/* model_id values for nic_set_weights (checkpoint names encoder{Y,CbCr}, decoder{Y,CbCr},
 * training.py:167-172) */
enum {
  NIC_MODEL_ENCODER_Y = 0,
  NIC_MODEL_ENCODER_CBCR = 1,
  NIC_MODEL_DECODER_Y = 2,
  NIC_MODEL_DECODER_CBCR = 3
};

/* Arithmetic of the convolutions:
 *   NIC_PRECISION_FP32  -- exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) for conv2..conv8 and
 *     dconv1..dconv7: an fp32 FMA chain; conv1 and dconv8 as fp32 VALU FMA.
 *   NIC_PRECISION_F16X3 -- split-f16 MFMA (default) for every convolution, conv1 (fused
 *     into conv2's kernel) and dconv8 included: each fp32 operand x = hi + lo with hi, lo
 *     f16 and weights pre-scaled by 2^k; a*w ~ a_hi*w_hi + a_hi*w_lo + a_lo*w_hi on
 *     v_mfma_f32_16x16x32_f16 / v_mfma_f32_32x32x16_f16 with fp32 accumulation.  Error
 *     ~2^-22 relative per product, i.e. at the level of fp32 accumulation-order
 *     differences.  The split format holds |x| < 65504 (the f16 range): see the range guard.
 *     Its kernels use 32-bit offsets inside one plane: images whose 64-channel level
 *     (ceil(h/4) x ceil(w/4), resp. 2*h8 x 2*w8 for decode) exceeds 2^22 pixels (~67 MP per
 *     image) run the NIC_PRECISION_FP32 kernels instead (same results class, no error).
 * Bias, activations, residuals, colour transforms and quantisers are fp32 in both modes. */
enum { NIC_PRECISION_FP32 = 0, NIC_PRECISION_F16X3 = 1 };

/* f16 range guard of NIC_PRECISION_F16X3 (the reference, encoder.py:19-32 / decoder.py:19-32,
 * has no activation bound; trained weights may drive an activation past the f16 range).
 * Every kernel that stores a split activation tracks max |x| and, at |x| >= 65504 or a
 * non-finite x, marks the ctx's range word with the pass's epoch.  Then:
 *   NIC_RANGE_FALLBACK (default) -- every split-f16 encode/decode pass is followed on the
 *     same stream by the exact-fp32 pass (NIC_PRECISION_FP32 kernels) gated on that mark:
 *     its kernels exit at once unless the split pass tripped, in which case they recompute
 *     and overwrite every output.  No host synchronisation; results always fp32-class.
 *   NIC_RANGE_ERROR -- the call synchronises its stream after the split pass and returns
 *     NIC_ERANGE if it tripped (outputs undefined).
 * nic_range_trips (synchronising) counts the passes that tripped since nic_create.
 * A FALLBACK re-run runs as one chained launch whose stages hand their tiles out through
 * device-side queues (no grid barrier): it completes whatever share of the grid is resident,
 * so a tripped FALLBACK call always returns the exact-fp32 outputs.
 * The guard watches the high side only.  The low half of a split activation is an f16
 * subnormal once it falls under 2^-14, i.e. for |x| under about 2^-3, and then carries an
 * absolute error of up to 2^-25 whatever |x| is.  With weights of ordinary size downstream
 * that is below fp32 rounding; a network whose layer runs at 2^-k and whose next kernel is
 * larger by 2^k (leaky-ReLU layers are positively homogeneous, so this is the same function)
 * gets it multiplied back: measured max error 1.8e-5 at k = 8, 3.6e-4 at k = 12, 1.2e-2 at
 * k = 17 against 1.3e-6 for the balanced network, with no trip under either policy.
 * nic_set_weights uploads tensors as given, one at a time, and cannot rebalance them.  The
 * Python Codec.set_weights does it before the upload (weights.lift_low_sites: every split
 * site whose estimated magnitude is under 2^-3 is lifted by an exact power of two, the next
 * kernel lowered by the same; the same function bit for bit in fp32, and a no-op for weights
 * of ordinary scale): with it the cases above measure at most 2.1e-6 at every k.  A caller
 * of this C interface with such weights does the same, or uses NIC_PRECISION_FP32
 * (unaffected at any k).  DESIGN.md section 3. */
enum { NIC_RANGE_FALLBACK = 0, NIC_RANGE_ERROR = 1 };
int nic_set_range_policy(nic_ctx* ctx, int policy);
int nic_range_trips(nic_ctx* ctx, int64_t* passes);
/* How the chained exact-fp32 re-run launches on ctx's device: its resident blocks per CU
 * (occupancy; informational -- the queued stages need no co-residency), the grid (one block
 * per CU) and whether it uses a cooperative launch (always 0: a plain launch). */
int nic_rerun_launch_info(nic_ctx* ctx, int* blocks_per_cu, int* grid, int* cooperative);
/* The grids nic_decode's split-f16 pass launches on ctx's device for n latents of h8 x w8, from
 * the launches' own split functions (nothing runs): blocks[0..1] dconv1's blocks for the Y and
 * for the CbCr planes, blocks[2..3] the same for dconv7, blocks[4] the grid of the fused
 * dconv5+dconv6 pair (0: those planes take two launches).  What a block of these persistent
 * kernels does depends on how many tiles it walks; the tests place their batches by these
 * figures.  NIC_ESHAPE for a batch the split-f16 pass does not take. */
int nic_decode_launch_info(nic_ctx* ctx, int n, int h8, int w8, int* blocks);

/* ABI version: major * 10000 + minor * 100 + patch */
int nic_version(void);

/* Host copies of the fp32 colour constants the device uses: fp32(ycbcr_kernel) (utils.py:7),
 * fp32(inv(ycbcr_kernel)) computed in float64 (utils.py:8), fp32(ycbcr_off) (utils.py:9).
 * Row-major 3x3; any pointer may be NULL. */
int nic_constants(float* ycbcr9, float* ycbcr_inv9, float* off3);

/* Human-readable description of the last error on this thread ("" if none). */
const char* nic_last_error(void);

/* Create a context on HIP device `device`. */
int nic_create(int device, nic_ctx** out);
int nic_destroy(nic_ctx* ctx);

/* Upload one tensor in its Keras layout from HOST memory (fp32, C order).
 *   layer: "conv1".."conv8" (Conv2D kernel (kh,kw,Cin,Cout), encoder.py:10-17) or
 *          "dconv1".."dconv8" (Conv2DTranspose kernel (kh,kw,Cout,Cin), decoder.py:10-17),
 *          followed by "/kernel" or "/bias" (bias shape (Cout,)).
 * The kernel is repacked to the device-native fragment layout.  Synchronous. */
int nic_set_weights(nic_ctx* ctx, int model_id, const char* layer, const float* host, const int64_t* shape,
                    int ndim);

int nic_set_precision(nic_ctx* ctx, int mode);
int nic_get_precision(nic_ctx* ctx, int* mode);

/* 1 when every tensor of the encoder pair (resp. decoder pair) has been set. */
int nic_weights_ready(nic_ctx* ctx, int* encoder_ready, int* decoder_ready);

/* Grow the workspace so encode of (n, h, w) images and decode of their latents allocate
 * nothing.  Synchronous. */
int nic_reserve(nic_ctx* ctx, int n, int h, int w);

/* Latent spatial size for an h x w image: ceil(h/8), ceil(w/8) (TF SAME, three s2 convs). */
int nic_latent_shape(int h, int w, int* h8, int* w8);

/* Encoder.__call__: rgb (n,h,w,3) u8 -> latent (n,h8,w8,96) u8.
 * prequant (nullable): (n,h8,w8,96) fp32, the clipped encoder output before round(x*255). */
int nic_encode(nic_ctx* ctx, const uint8_t* rgb, int n, int h, int w, uint8_t* latent, float* prequant,
               void* stream);

/* Decoder.__call__: latent (n,h8,w8,96) u8 -> rgb (n,8*h8,8*w8,3) u8.
 * rgb_f32 (nullable): the clipped fp32 RGB before round(x*255). */
int nic_decode(nic_ctx* ctx, const uint8_t* latent, int n, int h8, int w8, uint8_t* rgb, float* rgb_f32,
               void* stream);

/* Host-array surface: Encoder.__call__ / Decoder.__call__ on NumPy batches (encoder.py:38-47,
 * decoder.py:39-48 hand host arrays in and out around every call).  rgb / latent are HOST
 * pointers; the call is ordered after the work queued on `stream` and returns with the
 * outputs written (synchronous).  The batch runs as `chunks` (1..16) chunks on the ctx's own
 * streams, chunk k+1's H2D and chunk k-1's D2H overlapping chunk k's device pass; page-locked
 * buffers are DMA'd directly, pageable ones staged through the ctx's pinned buffers. */
int nic_encode_host(nic_ctx* ctx, const uint8_t* rgb, int n, int h, int w, uint8_t* latent, int chunks,
                    void* stream);
int nic_decode_host(nic_ctx* ctx, const uint8_t* latent, int n, int h8, int w8, uint8_t* rgb, int chunks,
                    void* stream);

/* Histogram entropy of each latent plane (tf1_13/src/training.py:66-71).
 * Plane order is the reference's concat along the batch: row p = plane p/n (Y,Cb,Cr) of
 * image p%n.  counts (nullable): (3n, 256) uint32.  bits (nullable): (3n,) fp32
 * bits/symbol.  Needs a ctx only for its scratch. */
int nic_entropy_hist(nic_ctx* ctx, const uint8_t* latent, int n, int h8, int w8, uint32_t* counts, float* bits,
                     void* stream);

/* Encode + histogram entropy of the new latent in one pass (BASELINE config 5: the encoder
 * followed by disc_entropy, tf1_13/src/training.py:66-71): same outputs as nic_encode then
 * nic_entropy_hist -- latent, counts (nullable), bits (nullable) -- with the codes counted in
 * conv8's epilogue as it quantises them (no re-read of the latent).  Shapes where the fold does
 * not apply (exact-fp32 precision, latents too small for one plane per block range) run the
 * two calls. */
int nic_encode_entropy(nic_ctx* ctx, const uint8_t* rgb, int n, int h, int w, uint8_t* latent, uint32_t* counts,
                       float* bits, void* stream);
/* 1 in *folds when nic_encode_entropy on (n, h, w) images (counts or bits requested) takes the
 * folded form on ctx's device and precision, 0 when it runs the two calls.  Shapes the call
 * refuses (NIC_ESHAPE: bad sizes, n > 21845, latent planes over 2^31 / 6 codes) and n = 0 are
 * refused the same way. */
int nic_encode_entropy_fold(nic_ctx* ctx, int n, int h, int w, int* folds);

/* MS-SSIM of tf.image.ssim_multiscale(a, b, max_val=255) (tf2_0/tests/calc_ssim.py:13)
 * per image: a, b u8 (n,h,w,3) -> ms_ssim (n,) fp32.  TF defaults: 11-tap Gaussian
 * (sigma 1.5), k1 0.01, k2 0.03, power factors (0.0448, 0.2856, 0.3001, 0.2363, 0.1333),
 * SYMMETRIC-padded 2x2 average pooling between scales; every scale >= 11 px: h, w >= 161.
 * per_scale (nullable): (n,3,5,2) fp32 mean SSIM and mean cs per channel and scale.
 * fp32 filtering, fp64 reductions.  Needs a ctx only for its scratch. */
int nic_ms_ssim(nic_ctx* ctx, const uint8_t* a, const uint8_t* b, int n, int h, int w, float* ms_ssim,
                float* per_scale, void* stream);

/* Exact per-image sum of squared differences of two u8 tensors of n images of
 * bytes_per_image bytes: sse (n,) uint64.  PSNR = 10 log10(255^2 * bytes / sse). */
int nic_sq_err(const uint8_t* a, const uint8_t* b, int n, int64_t bytes_per_image, uint64_t* sse, void* stream);

/* PNG files of m u8 images (h, w, channels = 1 or 3) in HOST memory, on `threads` host
 * threads (no GPU, no ctx; w * channels <= 16384), in one of two encoders' settings:
 *   NIC_PNG_PILLOW  Pillow with optimize=True, the reference's bitstream writer save_img
 *                   (utils.py:85-87): adaptive per-row filter (least sum of |signed bytes|,
 *                   first on ties), zlib level 9 / window 15 / memLevel 9 / Z_FILTERED,
 *                   65,536-B IDATs -- byte for byte Pillow's file (tests/test_png_encode.py;
 *                   Pillow and this library link the same zlib 1.2.11 here).
 *   NIC_PNG_TF      tf.image.encode_png(compression=-1), what get_bpp sizes
 *                   (training.py:12-21): libpng 1.6 defaults -- the same filter heuristic,
 *                   zlib default level (6) / memLevel 9 (png_io sets MAX_MEM_LEVEL) /
 *                   Z_FILTERED, libpng's window reduction and CMF rewrite for small images and
 *                   its filter pruning for 1-row / 1-column images, 8,192-B IDATs.  TensorFlow is
 *                   not importable here: parity with its own output is UNPINNED.
 * nic_png_encode writes file i at out + i * out_stride (out_stride >= nic_png_bound; out may
 * be NULL for sizes only) and its byte count to sizes[i].  nic_png_sizes = the Pillow sizes
 * (the val_bpp of training.py:157-163 and the RD harness). */
#define NIC_PNG_PILLOW 0
#define NIC_PNG_TF 1
int nic_png_bound(int h, int w, int channels, int mode, int64_t* bytes);
int nic_png_encode(const uint8_t* images, int m, int h, int w, int channels, int mode, uint8_t* out,
                   int64_t out_stride, int64_t* sizes, int threads);
int nic_png_sizes(const uint8_t* images, int m, int h, int w, int channels, int64_t* sizes, int threads);

/* Bitstream image layout of ProClass._feed_batch: (n,h8,w8,96) <-> (n,4*h8,8*w8,3), each
 * plane a raw C-order reshape (utils.py:35-36, 39-40). */
int nic_pack_latent(const uint8_t* latent, int n, int h8, int w8, uint8_t* packed, void* stream);
int nic_unpack_latent(const uint8_t* packed, int n, int h8, int w8, uint8_t* latent, void* stream);

/* ---- The .nic container (version 1): a native bitstream beside the reference's PNG ----------
 * One file per image, a static per-channel byte-wise rANS code of the latent, written and read
 * on the device (format: DESIGN.md, "The .nic container"):
 *   header 16 B: "NICR", u8 version 1, u8 probability bits 12, u16 seg_pixels, u32 h8, u32 w8
 *   96 tables (channel order of the latent): u8 n-1, then n x (u8 symbol, u16 freq), symbols
 *     ascending, freqs in 1..4096 summing to 4096
 *   nseg = ceil(h8 w8 / seg_pixels) u32 segment lengths, then the segments' bytes
 * Segment k codes the latent bytes [k K, min((k+1) K, 96 h8 w8)), K = 96 seg_pixels, in NHWC
 * order.  Little-endian throughout, except each segment's leading 4-byte final state.
 *
 * nic_rans_bound: the largest file of an (h8, w8) latent (every table full, 12 bits per symbol):
 *     the minimum `stride` of nic_rans_encode.  h8 * w8 <= 2^23, seg_pixels in 1..65535.
 * nic_rans_reserve: grow the workspace so nic_rans_encode / nic_rans_decode of (n, h8, w8)
 *     latents allocate nothing.  Synchronous.
 * nic_rans_encode: latent (n,h8,w8,96) u8 (16-byte aligned) -> file i at out + i * stride, its
 *     byte count in sizes[i] (DEVICE int64[n]).  Counting, table normalisation, coding and file
 *     assembly all run on `stream`; no host synchronisation.  An image's file depends on that
 *     image alone.
 * nic_rans_decode: files at files + i * stride of sizes[i] bytes (DEVICE int64[n]), all of one
 *     (h8, w8) (seg_pixels is read per file on the device) -> latent (n,h8,w8,96) and status[i]
 *     (DEVICE int32[n]): 0 ok; bit 0: a segment did not end with its state at 2^23 on its last
 *     byte; bit 1: the header is not a version-1 header of an (h8, w8) latent (that image's
 *     latent is left unwritten); bit 2: a stored table is not "symbols ascending, freqs in 1..4096
 *     summing to 4096" (a freq of 0, a freq or a running sum above 4096 and a sum short of 4096 all
 *     count).  Tables are parsed on the device.  sizes[i] is clamped to [0, stride] and every read
 *     of a file byte to [0, sizes[i]): a byte at or past the size reads as 0, whatever the buffer
 *     holds there, so a file cut short of its header has bit 1 and one cut anywhere behind it has
 *     bit 0 or bit 2.  No input bytes can take the kernels out of bounds: segment offsets saturate
 *     at the size, file reads are clamped to the segment, table lookups resolve inside the 4096
 *     slots (a broken table still yields a row that does), and stores go to the lane's own latent
 *     bytes.  An image with a non-zero status may hold anything inside its own h8 w8 96 bytes.
 *     The size sum is nic_rans_inspect's check alone: bytes behind the last segment, or a last
 *     segment length that runs past the size, have no status bit and the file decodes cleanly.
 * nic_rans_inspect: HOST-only check of one file in host memory (no GPU, no ctx): magic, version,
 *     probability bits, seg_pixels >= 1, h8 w8 in range, every table's invariants, and header +
 *     tables + segment table + sum of segment lengths == size.  NIC_ECORRUPT (nic_last_error
 *     says what) otherwise; h8 / w8 / seg_pixels (each nullable) on success. */
int nic_rans_bound(int h8, int w8, int seg_pixels, int64_t* bytes);
int nic_rans_reserve(nic_ctx* ctx, int n, int h8, int w8, int seg_pixels);
int nic_rans_encode(nic_ctx* ctx, const uint8_t* latent, int n, int h8, int w8, int seg_pixels, uint8_t* out,
                    int64_t stride, int64_t* sizes, void* stream);
int nic_rans_decode(nic_ctx* ctx, const uint8_t* files, int64_t stride, const int64_t* sizes, int n, int h8, int w8,
                    uint8_t* latent, int32_t* status, void* stream);
int nic_rans_inspect(const uint8_t* host_file, int64_t size, int* h8, int* w8, int* seg_pixels);

/* ---- The .nic container, version 2: a codec-level prior, so files need not carry tables ---------
 * The prior is the entropy model shipped with the codec: 96 x 256 freqs (channel order of the
 * latent), each in 1..4096, every channel summing to 4096, fitted once over a corpus.  Its id is
 * the CRC-32 (IEEE) of the 49,152 bytes of the freqs as little-endian u16, channel-major.  Format
 * ("The .nic container, version 2"):
 *   header 40 B: "NICR", u8 version 2, u8 probability bits 12, u16 seg_pixels, u32 h8, u32 w8,
 *     u32 H, u32 W (the image's own size: h8 = ceil(H/8), w8 = ceil(W/8)), u32 prior_id, 12-byte
 *     channel mask (channel c is bit c & 7 of byte c >> 3)
 *   a version-1 table for every channel whose mask bit is 1, in channel order; the others are
 *     coded with the prior's row
 *   the segment table and the segments, exactly as in version 1
 * The encoder keeps a channel's own table iff it pays for itself: with cost16[f] =
 * floor((12 - log2 f) 65536 + 0.5), own = sum c cost16[f_own] + (8 (1 + 3 n) << 16) < prior =
 * sum c cost16[f_prior] (u64; a tie goes to the prior).
 *
 * nic_rans_cost_table: HOST only.  out[0] = 0, out[f] = cost16[f] for f in 1..4096.
 * nic_rans_prior_check: HOST only.  Checks the invariants of 96 x 256 host freqs and returns the
 *     id (nullable); NIC_ECORRUPT naming the channel otherwise.
 * nic_rans_prior_set: checks, then uploads the freqs, their cumulative rows and the cost table.
 *     Synchronous (waits for the device).  NULL freqs clears the prior.  id nullable.
 * nic_rans_prior_count: adds the counts of latent (n,h8,w8,96) u8 (16-byte aligned) into the
 *     caller's DEVICE uint64[96 * 256] accumulator (zeroed by the caller) with 64-bit integer
 *     atomics: deterministic, accumulates across calls.  On `stream`, no host synchronisation.
 * nic_rans_prior_build: accumulated counts -> DEVICE uint16[96 * 256] freqs: for a channel's
 *     counts c[256] of total N, f = max(1, floor(c 4096 / N)) for every symbol; a deficit goes onto
 *     the largest entry; a surplus is taken one at a time from the currently largest entry (lowest
 *     symbol on ties); N = 0 gives sixteen everywhere.  N must stay below 2^52 per channel.
 * nic_rans2_bound = nic_rans_bound + 24.  nic_rans2_reserve: as nic_rans_reserve.
 * nic_rans2_encode: as nic_rans_encode; every image of the call is H x W.  NIC_ENOPRIOR before
 *     nic_rans_prior_set.
 * nic_rans2_decode: as nic_rans_decode; status bit 1: not a version-2 header of an (h8, w8) latent
 *     with a consistent (H, W); bit 3 (value 8): the file's prior_id is not the ctx's (that
 *     image's latent is left unwritten).  NIC_ENOPRIOR before nic_rans_prior_set.
 * nic_rans2_inspect: HOST only: nic_rans_inspect's checks on a version-2 file (tables of the
 *     masked channels only) plus the H / W relation; every output nullable.
 * Arguments are validated before any HIP call: shape, empty batch (OK), NULL, then the prior. */
int nic_rans_cost_table(uint32_t* out4097);
int nic_rans_prior_check(const uint16_t* host_freqs, uint32_t* id);
int nic_rans_prior_set(nic_ctx* ctx, const uint16_t* host_freqs, uint32_t* id);
int nic_rans_prior_count(nic_ctx* ctx, const uint8_t* latent, int n, int h8, int w8, uint64_t* counts_dev, void* stream);
int nic_rans_prior_build(nic_ctx* ctx, const uint64_t* counts_dev, uint16_t* freqs_dev, void* stream);
int nic_rans2_bound(int h8, int w8, int seg_pixels, int64_t* bytes);
int nic_rans2_reserve(nic_ctx* ctx, int n, int h8, int w8, int seg_pixels);
int nic_rans2_encode(nic_ctx* ctx, const uint8_t* latent, int n, int h8, int w8, int H, int W, int seg_pixels,
                     uint8_t* out, int64_t stride, int64_t* sizes, void* stream);
int nic_rans2_decode(nic_ctx* ctx, const uint8_t* files, int64_t stride, const int64_t* sizes, int n, int h8, int w8,
                     uint8_t* latent, int32_t* status, void* stream);
int nic_rans2_inspect(const uint8_t* host_file, int64_t size, int* h8, int* w8, int* seg_pixels, int* H, int* W,
                      uint32_t* prior_id);

/* ---- The .nic container, version 3: a context prior conditioned on the left neighbour -----------
 * The context prior holds, for each of the 96 channels, one anchor symbol a_c (u8) and 3 contexts
 * x 256 freqs (each in 1..4096, every (channel, context) row summing to 4096).  Its id is the
 * CRC-32 (IEEE) of the 96 anchors followed by the 147,456 bytes of the freqs as little-endian u16,
 * channel-major, then context, then symbol.  Format ("The .nic container, version 3"):
 *   the version-2 file with version byte 3 and the context prior's id in prior_id
 *   the byte at segment-relative offset j (channel c = j mod 96, pixel q = j div 96) is coded
 *     under row (c, k): k = 0 if q = 0, else min(2, |z[j - 96] - a_c|) -- the previous pixel in
 *     memory order, never a pixel of another segment
 *   a masked channel stores a version-1 table and is coded under it in every context
 * The per-channel choice is version 2's rule with prior = sum_k sum_s c_k[s] cost16[f[c][k][s]],
 * c_k the image's counts of channel c in context k under the call's seg_pixels.
 *
 * nic_rans_cprior_check: HOST only.  Checks 96 host anchors and 96 x 3 x 256 host freqs and returns
 *     the id (nullable); NIC_ECORRUPT naming the channel and the context otherwise.
 * nic_rans_cprior_set: checks, then uploads the anchors, freqs, cumulative rows and the cost table.
 *     Synchronous.  anchors = freqs = NULL clears the context prior.  id nullable.  The context
 *     prior and nic_rans_prior_set's prior are independent of each other.
 * nic_rans_cprior_count: adds the context counts of latent (n,h8,w8,96) u8 (16-byte aligned), cut
 *     into segments of seg_pixels, under the DEVICE anchors uint8[96] into the caller's DEVICE
 *     uint64[96 * 3 * 256] accumulator (zeroed by the caller) with 64-bit integer atomics:
 *     deterministic, accumulates across calls.  On `stream`, no host synchronisation.
 * nic_rans_cprior_build: accumulated counts -> DEVICE uint16[96 * 3 * 256] freqs, every row by
 *     nic_rans_prior_build's rule (N = 0 gives sixteen everywhere).
 * nic_rans3_bound = nic_rans2_bound.  nic_rans3_reserve / nic_rans3_encode / nic_rans3_decode /
 *     nic_rans3_inspect: as their version-2 namesakes, with the context prior: NIC_ENOPRIOR before
 *     nic_rans_cprior_set; decode status bit 1: not a version-3 header of an (h8, w8) latent with a
 *     consistent (H, W); bit 3 (value 8): the file's prior_id is not the ctx's context prior's
 *     (that image's latent is left unwritten).
 * Arguments are validated before any HIP call: shape, empty batch (OK), NULL, then the prior. */
int nic_rans_cprior_check(const uint8_t* host_anchors, const uint16_t* host_freqs, uint32_t* id);
int nic_rans_cprior_set(nic_ctx* ctx, const uint8_t* host_anchors, const uint16_t* host_freqs, uint32_t* id);
int nic_rans_cprior_count(nic_ctx* ctx, const uint8_t* latent, int n, int h8, int w8, int seg_pixels,
                          const uint8_t* anchors_dev, uint64_t* counts_dev, void* stream);
int nic_rans_cprior_build(nic_ctx* ctx, const uint64_t* counts_dev, uint16_t* freqs_dev, void* stream);
int nic_rans3_bound(int h8, int w8, int seg_pixels, int64_t* bytes);
int nic_rans3_reserve(nic_ctx* ctx, int n, int h8, int w8, int seg_pixels);
int nic_rans3_encode(nic_ctx* ctx, const uint8_t* latent, int n, int h8, int w8, int H, int W, int seg_pixels,
                     uint8_t* out, int64_t stride, int64_t* sizes, void* stream);
int nic_rans3_decode(nic_ctx* ctx, const uint8_t* files, int64_t stride, const int64_t* sizes, int n, int h8, int w8,
                     uint8_t* latent, int32_t* status, void* stream);
int nic_rans3_inspect(const uint8_t* host_file, int64_t size, int* h8, int* w8, int* seg_pixels, int* H, int* W,
                      uint32_t* prior_id);

/* ---- Rate-distortion optimised quantisation against a .nic prior --------------------------------
 * An encoder-side step between nic_encode and nic_rans2_encode / nic_rans3_encode: every latent byte
 * keeps its code or moves one step towards its pre-quant value, whichever costs less in distortion
 * plus lambda times the bits the prior charges.  The file format and the decoder are untouched
 * (DESIGN.md §25).  Per byte, with r the code (nic_encode's latent) and f its pre-quant value
 * (nic_encode's prequant, in [0, 1]):
 *   v = f * 255 and e = v - r, one fp32 multiply and one fp32 subtract, not contracted
 *   alt = r + 1 if e > 0, r - 1 if e < 0, r if e = 0 (held inside 0..255); candidate 0 is r, 1 is alt
 *   D(q) = (u64) rintf((v - q) * (v - q) * 65536) << 16, the same unfused fp32 operations
 *   rate(q | row F) = lam_fix * cost16[F[q]] (nic_rans_cost_table), lam_fix = round(lambda 65536)
 * contexts = 1, the static prior: every byte on its own under its channel's row; the smaller
 *   D + rate, a tie to r.  seg_pixels is checked and otherwise unused.
 * contexts = 3, the context prior: every (segment, channel) chain as a whole, segments and rows
 *   exactly version 3's under the call's seg_pixels, the row of a pixel chosen by the code KEPT for
 *   the pixel before it: best[p][b] = min over b' of best[p-1][b'] + D(p, b) + rate(p, b | ctx(b')),
 *   a tie to b' = 0; the end state is the smaller best, a tie to 0; then the back-pointers are walked.
 * The prior's rows price every channel; whether a channel then keeps its own table in the file is
 * the coder's choice as before, which can only make the file smaller than what was priced.
 * lam_fix = 0 returns latent; the output differs from latent by at most 1 per byte and stays in
 * 0..255.  Deterministic; on `stream`, no host synchronisation, no workspace.
 *
 * nic_rdoq: latent, latent_out (n,h8,w8,96) u8 and prequant (n,h8,w8,96) fp32, all 16-byte aligned
 *     device buffers.  seg_pixels in 1..64 (the back-pointers of a chain are two 64-bit masks;
 *     NIC_ESHAPE otherwise), lam_fix in 0..16 * 65536 and contexts 1 or 3 (NIC_EINVAL otherwise).
 *     latent_out must not overlap latent (NIC_EINVAL).  NIC_ENOPRIOR before nic_rans_prior_set
 *     (contexts 1) or nic_rans_cprior_set (contexts 3).
 * Arguments are validated before any HIP call: shape, empty batch (OK), NULL, then the prior. */
int nic_rdoq(nic_ctx* ctx, const uint8_t* latent, const float* prequant, int n, int h8, int w8, int seg_pixels,
             uint32_t lam_fix, int contexts, uint8_t* latent_out, void* stream);

/* ---- Region decode: a pixel box out of a .nic file (every container version) --------------------
 * A file's segment table is a random-access index: segment k holds the latent pixels [k S, (k+1) S)
 * of the row-major order (S = seg_pixels), so a window of the latent needs only the segments that
 * hold one of its pixels, and the decoder needs only a window of the latent ("Region
 * decode").
 *
 * NIC_DECODE_HALO: the decoder's receptive field, in latent pixels on each side of the latent pixels
 *     a box touches.  Output pixel o of a stride-2 transposed 5x5 layer (dconv1, dconv7, dconv8) reads
 *     its input within floor(o/2) +- 1; dconv5 and dconv6 (3x3, stride 1, at twice the latent's
 *     resolution) read +- 1 each.  So image pixel o reads the 4x level within floor(o/2) +- 1, the 2x
 *     level within floor(o/4) +- 2 behind dconv7 and +- 4 behind dconv6 and dconv5, and the latent
 *     within floor(o/8) +- 3.  With 3 the decode of the window, cut at the box, equals the crop of the
 *     whole decode exactly (a window edge short of 3 is the latent's own edge, with the same zero
 *     padding behind it); with 2 it does not.
 * nic_region_plan: HOST only (no GPU, no ctx).  For the box [y, y + bh) x [x, x + bw) of an H x W
 *     image (0 <= y, bh >= 1, y + bh <= H, likewise x; NIC_ESHAPE otherwise) with h8 = ceil(H/8),
 *     w8 = ceil(W/8):  ry0 = y / 8, ry1 = (y + bh - 1) / 8 + 1, r0 = max(0, ry0 - 3), r1 = min(h8,
 *     ry1 + 3), likewise c0, c1.  win4 = {r0, c0, r1 - r0, c1 - c0}: the latent window with its halo,
 *     clamped to the latent; off2 = {y - 8 r0, x - 8 c0}: where the box starts in the window's
 *     reconstruction (8 rows x 8 cols pixels).  NIC_EINVAL for a NULL output.
 * nic_rans_window_segments: HOST only.  The number of distinct segments that hold a latent pixel of
 *     the window (r0, c0, rows, cols) of an (h8, w8) latent under seg_pixels: the segment state
 *     machines a window decode runs (a segment may cross row ends).  The window must lie inside the
 *     latent (NIC_ESHAPE); count NULL: NIC_EINVAL.
 * nic_rans_decode_window / nic_rans2_decode_window / nic_rans3_decode_window: as nic_rans_decode /
 *     nic_rans2_decode / nic_rans3_decode -- n whole files of one (h8, w8), the same parse on the
 *     device, the same workspace (nic_rans*_reserve of (n, h8, w8) covers it), `stream`, no host
 *     synchronisation -- but only the segments that hold a pixel of the window r0, c0 >= 0, rows,
 *     cols >= 1, r0 + rows <= h8, c0 + cols <= w8 (NIC_ESHAPE otherwise) are decoded, each from its
 *     first pixel to its last, and latent_win (n, rows, cols, 96) u8 (16-byte aligned) receives the
 *     window: latent_win[i][a][b] = latent[i][r0 + a][c0 + b].  status[i]: bits 1, 2 and 3 as in the
 *     full decode (an image refused with bit 1 or bit 3 leaves its latent_win unwritten); bit 0
 *     covers only the segments that were decoded -- damage in a segment outside the window is
 *     neither seen nor reported.  File reads are clamped to the segment, lookups resolve inside the
 *     4096 slots, and a lane stores only its own segment's pixels that lie inside the window.
 * Arguments are validated before any HIP call: shape (the window included), empty batch (OK), NULL,
 * then the prior (NIC_ENOPRIOR, versions 2 and 3). */
#define NIC_DECODE_HALO 3
int nic_region_plan(int H, int W, int y, int x, int bh, int bw, int* win4, int* off2);
int nic_rans_window_segments(int h8, int w8, int seg_pixels, int r0, int c0, int rows, int cols, int64_t* count);
int nic_rans_decode_window(nic_ctx* ctx, const uint8_t* files, int64_t stride, const int64_t* sizes, int n, int h8, int w8,
                           int r0, int c0, int rows, int cols, uint8_t* latent_win, int32_t* status, void* stream);
int nic_rans2_decode_window(nic_ctx* ctx, const uint8_t* files, int64_t stride, const int64_t* sizes, int n, int h8, int w8,
                            int r0, int c0, int rows, int cols, uint8_t* latent_win, int32_t* status, void* stream);
int nic_rans3_decode_window(nic_ctx* ctx, const uint8_t* files, int64_t stride, const int64_t* sizes, int n, int h8, int w8,
                            int r0, int c0, int rows, int cols, uint8_t* latent_win, int32_t* status, void* stream);

/* ---- Batched region decode: a box per file, files of different frame sizes, one call -------------
 * Boxes of one size out of files of any sizes need latent windows of one shape, so the windows of a
 * whole batch decode, and the decoder runs, as one (n, rows, cols, 96) tensor ("Batched
 * region decode").
 *
 * nic_region_plan_fixed: HOST only, beside nic_region_plan (the same boxes are valid, the same error
 *     codes).  The window's shape depends on the box's size and on the latent's only where the latent
 *     is smaller: per axis T = (bh + 6) / 8 + 1 (the most latent rows bh pixel rows touch), R = T +
 *     2 NIC_DECODE_HALO, rows = min(h8, R), r0 = clamp(y / 8 - NIC_DECODE_HALO, 0, h8 - rows);
 *     columns likewise from bw, x and w8.  win4 = {r0, c0, rows, cols}, off2 = {y - 8 r0, x - 8 c0}.
 *     The window holds nic_region_plan's; each of its edges lies on the latent's edge or at least
 *     NIC_DECODE_HALO latent pixels beyond the box's, so the window's reconstruction cut at off2 is the
 *     crop of the whole one, exactly as for nic_region_plan.
 * nic_rans_decode_windows / nic_rans2_decode_windows / nic_rans3_decode_windows: as
 *     nic_rans*_decode_window -- n whole files at one stride, `stream`, no host synchronisation -- but
 *     file i has its own latent size and window place, row i of table, int32[n][4] = {h8, w8, r0, c0}
 *     on the DEVICE (4-byte aligned), and the call has one window shape rows x cols; latent_win
 *     (n, rows, cols, 96) u8, 16-byte aligned: latent_win[i][a][b] = latent_i[r0_i + a][c0_i + b].
 *     max_pixels: the caller's bound on h8 w8 of any row, 1..2^23; it sizes the workspace
 *     (nic_rans*_reserve of n latents of at least max_pixels pixels covers it), because the table is
 *     never read on the host.  The device checks row i before it acts on it: h8, w8 >= 1, h8 w8 <=
 *     max_pixels, r0, c0 >= 0, r0 + rows <= h8, c0 + cols <= w8, and the file's header must describe
 *     an (h8, w8) latent; otherwise status[i] has bit 1 (the header bit), nothing of file i is decoded
 *     or written, and the other files are not affected.  The other status bits mean, per file, what
 *     they mean in nic_rans*_decode_window, and the same bounds hold: clamped file reads, lookups
 *     inside the 4096 slots, stores only inside latent_win[i].
 *     Validated before any HIP call: n in 0..65535, max_pixels, 1 <= rows, cols, rows cols <=
 *     max_pixels (NIC_ESHAPE); empty batch (OK); NULL; alignment; stride; the prior (NIC_ENOPRIOR).
 * nic_cut_boxes: boxes (n, bh, bw, 3) u8 = the bh x bw box at offsets[i] = {oy, ox} of image i of
 *     images (n, Hs, Ws, 3) u8; offsets is int32[n][2] on the DEVICE; boxes and offsets 4-byte aligned;
 *     one launch on `stream`, no host synchronisation.  1 <= bh <= Hs, 1 <= bw <= Ws, Hs Ws <= 2^29,
 *     n bh bw 3 < 2^40 (NIC_ESHAPE).  Whoever fills the table checks 0 <= oy <= Hs - bh, 0 <= ox <=
 *     Ws - bw on the host (Codec.cut_boxes does, before the upload); the kernel does not trust it: a
 *     source byte outside its image reads as 0 and no byte outside images is touched. */
int nic_region_plan_fixed(int H, int W, int y, int x, int bh, int bw, int* win4, int* off2);
int nic_rans_decode_windows(nic_ctx* ctx, const uint8_t* files, int64_t stride, const int64_t* sizes, int n, const int32_t* table,
                            int max_pixels, int rows, int cols, uint8_t* latent_win, int32_t* status, void* stream);
int nic_rans2_decode_windows(nic_ctx* ctx, const uint8_t* files, int64_t stride, const int64_t* sizes, int n, const int32_t* table,
                             int max_pixels, int rows, int cols, uint8_t* latent_win, int32_t* status, void* stream);
int nic_rans3_decode_windows(nic_ctx* ctx, const uint8_t* files, int64_t stride, const int64_t* sizes, int n, const int32_t* table,
                             int max_pixels, int rows, int cols, uint8_t* latent_win, int32_t* status, void* stream);
int nic_cut_boxes(nic_ctx* ctx, const uint8_t* images, int n, int Hs, int Ws, const int32_t* offsets, int bh, int bw, uint8_t* boxes,
                  void* stream);

/* ---- Crops of mixed sizes, resized on the device for training ------------------------------------
 * A training loader draws a box of another size out of every image and resizes it to one output size
 * ("Crops of mixed sizes, resized on the device").  Boxes of different sizes get latent
 * windows of one shape from nic_region_plan_window, so they decode as one batch; nic_resample_boxes
 * turns the windows' reconstructions into the model's input.
 *
 * nic_region_plan_window: HOST only, beside nic_region_plan_fixed (the same boxes are valid, the same
 *     error codes), with the window's shape given: per axis R = (bh + 6) / 8 + 1 + 2 NIC_DECODE_HALO
 *     as in the fixed plan, rows_want >= R and cols_want >= C (NIC_ESHAPE otherwise), rows = min(h8,
 *     rows_want), r0 = clamp(y / 8 - NIC_DECODE_HALO, 0, h8 - rows); columns likewise.  win4 and off2
 *     as in the fixed plan, and at (R, C) the fixed plan's values.  The window holds
 *     nic_region_plan's, and each of its edges lies on the latent's edge or at least NIC_DECODE_HALO
 *     beyond the box's latent pixels, so the cut at off2 is as exact.
 * nic_resample_boxes: images (n, Hs, Ws, 3) u8; table int32[n][6] = {oy, ox, bh, bw, flip, dst} on the
 *     DEVICE (4-byte aligned): the bh x bw box at (oy, ox) of image i, resized to oh x ow, mirrored
 *     left to right where flip is 1, becomes image dst of out (16-byte aligned):
 *       NIC_RESAMPLE_F32  (n_out, 3, oh, ow) fp32,  v scale3[c] + bias3[c] (one fma; v in 0..255)
 *       NIC_RESAMPLE_F16  the same, rounded to f16
 *       NIC_RESAMPLE_U8   (n_out, oh, ow, 3) u8, v rounded half to even and clamped to 0..255; scale3
 *                         and bias3 are not read and may be NULL
 *     scale3 and bias3 are HOST arrays of 3 floats.  One launch on `stream`, no host synchronisation,
 *     no workspace.  The resize is torch.nn.functional.interpolate(mode="bilinear", align_corners=
 *     False, antialias=True) on float input: per axis s = in / out (in = bh or bw), support = max(s,
 *     1), c = s (i + 0.5), taps [max(0, int(c - support + 0.5)), min(int(c + support + 0.5), in)),
 *     tap p weighs max(0, 1 - |p + 0.5 - c| / support) over the taps' sum; separable; taps never
 *     leave the box.  At bh = oh and bw = ow the output is the source pixel.  fp32 arithmetic.
 *     The kernel does not trust the table: a row with bh < 1, bw < 1, oy < 0, ox < 0, oy + bh > Hs,
 *     ox + bw > Ws, flip not 0 or 1, or dst outside [0, n_out) is skipped and stores nothing; no row
 *     reads outside images[i] or writes outside out[dst].  Rows that name one dst race.
 *     Validated before any HIP call: n in 0..65535, Hs, Ws >= 1, Hs Ws <= 2^29, 1 <= oh, ow <= 16384,
 *     n_out >= 1, n_out 3 oh ow < 2^40 (NIC_ESHAPE); out_kind (NIC_EINVAL); empty batch (OK); NULL;
 *     alignment (NIC_EINVAL). */
#define NIC_RESAMPLE_F32 0
#define NIC_RESAMPLE_F16 1
#define NIC_RESAMPLE_U8 2
int nic_region_plan_window(int H, int W, int y, int x, int bh, int bw, int rows_want, int cols_want, int* win4, int* off2);
int nic_resample_boxes(nic_ctx* ctx, const uint8_t* images, int n, int Hs, int Ws, const int32_t* table, int oh, int ow, int n_out,
                       int out_kind, const float* scale3, const float* bias3, void* out, void* stream);

/* ---- Images of mixed sizes, resized in one launch ------------------------------------------------
 * The write side's preparation step: photographs of any sizes go up as one pool and come out at one
 * size, ready for nic_encode ("Images of mixed sizes, resized and encoded in one batch").
 *
 * nic_resample_ragged: nic_resample_boxes with ragged sources.  pool: pool_bytes bytes of u8 on the
 *     DEVICE, 4-byte aligned.  table: int64[n][8] on the DEVICE, 8-byte aligned, row i =
 *       {offset, Hs, Ws, oy, ox, bh, bw, dst | flip << 32}
 *     source i is the tightly packed (Hs, Ws, 3) u8 image whose first byte is pool[offset] (no padding
 *     between its rows; offset a multiple of 4); the bh x bw box at (oy, ox) of it, resized to oh x ow,
 *     mirrored where flip is 1, becomes image dst of out.  dst is the low 32 bits of the last field as
 *     a signed integer, flip the high 32.  Images may overlap or repeat: the pool is only read.
 *     oh, ow, n_out, out_kind, scale3, bias3, out, stream and the arithmetic, bit for bit, are
 *     nic_resample_boxes': the same box of the same pixels gives the same output whichever entry reads it.
 *     The kernel does not trust the table.  A row with offset < 0, offset not a multiple of 4, Hs < 1,
 *     Ws < 1, Hs Ws > 2^29 (nic_resample_boxes' limit on a shape), offset + 3 Hs Ws > pool_bytes
 *     (compared in 64 bits, without overflow for any field values), a box outside its image (bh < 1,
 *     bw < 1, oy < 0, ox < 0, oy + bh > Hs, ox + bw > Ws), flip not 0 or 1, or dst outside [0, n_out)
 *     is skipped by its whole block before anything else is read, and stores nothing; no row reads
 *     outside its own image or writes outside out[dst].  Rows that name one dst race.
 *     Validated before any HIP call: n in 0..65535, pool_bytes >= 0, 1 <= oh, ow <= 16384, n_out >= 1,
 *     n_out 3 oh ow < 2^40 (NIC_ESHAPE); out_kind (NIC_EINVAL); empty batch (OK); NULL; alignment of
 *     pool (4), table (8) and out (16) (NIC_EINVAL). */
int nic_resample_ragged(nic_ctx* ctx, const uint8_t* pool, int64_t pool_bytes, int n, const int64_t* table, int oh, int ow,
                        int n_out, int out_kind, const float* scale3, const float* bias3, void* out, void* stream);

/* ---- The device PNG writer: complete PNG files written on the device --------------------------
 * An optional writer for reconstructions (Pillow's optimize=True file, nic_png_encode, stays the
 * default and the bitstream's format).  Format: DESIGN.md, "The device PNG writer":
 *   signature, IHDR (8-bit, colour type 0 or 2), one IDAT, IEND; no ancillary chunks
 *   IDAT = zlib header 78 01, deflate blocks, Adler-32 of the filtered stream
 *   filtered stream: per row the filter byte and the filtered row; NIC_PNG_FILTER_ADAPTIVE is
 *     nic_png_encode's heuristic (the stream inside Pillow's optimize=True file, byte for byte),
 *     0..4 one fixed filter (None, Sub, Up, Average, Paeth) for every row
 *   the stream is cut into blocks of nic_png_device_block_bytes(); every block is one dynamic-
 *     Huffman block of literals + end-of-block followed by an empty stored block (byte alignment),
 *     or a stored block where that is no larger; no LZ77 matching
 * An image's file depends on that image and the arguments alone.
 *
 * nic_png_device_bound: the largest file of an (h, w, channels) image, the minimum `stride`:
 *     63 + T + 5 * ceil(T / block_bytes), T = h * (w * channels + 1).  w * channels <= 16384,
 *     T <= 2^30, channels 1 or 3.
 * nic_png_device_reserve: grow the workspace so nic_png_device_encode of n such images allocates
 *     nothing.  Synchronous.
 * nic_png_device_encode: images (n,h,w,channels) u8 on the DEVICE -> file i at out + i * stride
 *     (DEVICE), its byte count in sizes[i] (DEVICE int64[n]).  Everything runs on `stream`; no
 *     host synchronisation.  n <= 65535. */
#define NIC_PNG_FILTER_ADAPTIVE (-1)
int nic_png_device_block_bytes(void);
int nic_png_device_bound(int h, int w, int channels, int64_t* bytes);
int nic_png_device_reserve(nic_ctx* ctx, int n, int h, int w, int channels);
int nic_png_device_encode(nic_ctx* ctx, const uint8_t* images, int n, int h, int w, int channels, int filter,
                          uint8_t* out, int64_t stride, int64_t* sizes, void* stream);

/* ---- The device PNG reader: PNG files inflated and unfiltered on the device ---------------------
 * An optional reader for the directory drivers (Pillow stays the default).  The host cuts a file
 * into its one zlib stream and checks the container; the device does the rest ("The device
 * PNG reader"):
 *   host    signature, chunk framing, every chunk's CRC-32, IHDR first, consecutive IDATs, IEND last
 *   device  inflate (stored, fixed and dynamic blocks, LZ77 matches over the 32 KB window), the
 *           Adler-32 of the inflated stream, the five PNG filters undone
 *
 * nic_png_inspect: HOST only (no GPU, no ctx).  One PNG file in host memory -> h, w, channels (each
 *     nullable), the byte count of the concatenated IDAT payloads in *idat_bytes (nullable) and, when
 *     idat is not NULL, those bytes copied to idat[0 .. *idat_bytes) (idat_capacity below that:
 *     NIC_ESHAPE).  NIC_ECORRUPT for a broken file: bad signature, a truncated chunk, a wrong CRC-32,
 *     IHDR missing, repeated or not 13 bytes, zero dimensions, IDATs split by another chunk, no IDAT,
 *     no IEND, bytes after IEND.  NIC_EUNSUPPORTED for a well-formed file the device reader does not
 *     take (nic_last_error says which): anything but 8-bit colour type 0 or 2, non-interlaced, no
 *     tRNS, no unknown critical chunk, w * channels <= 16384 and T = h * (w * channels + 1) <= 2^30.
 *     Ancillary chunks are skipped.  A broken file is NIC_ECORRUPT whatever its kind.
 * nic_png_device_read_reserve: grow the workspace so nic_png_device_read of n such images allocates
 *     nothing.  Synchronous.
 * nic_png_device_read: zlib stream i at streams + i * stride (DEVICE) of sizes[i] bytes (DEVICE
 *     int64[n]; a size outside 0..stride is clamped to it), every stream of an image of one (h, w,
 *     channels) -> images (n,h,w,channels) u8 and status[i] (DEVICE int32[n]): 0 ok, else one of
 *        1  bad zlib header: CM, CINFO, FCHECK, or FDICT set
 *        2  invalid deflate data: block type 3; stored LEN / NLEN mismatch; a code-length set that is
 *           over-subscribed or incomplete as zlib judges it; a repeat code with no previous length;
 *           HLIT / HDIST out of range; no end-of-block code; a symbol with no code; a distance beyond
 *           the bytes produced so far; input exhausted before the final block ends
 *        4  the stream produces more or fewer than T bytes, or ends before its four Adler-32 bytes
 *           (bytes after them are ignored, as zlib's decompress ignores them)
 *        8  Adler-32 mismatch
 *       16  a filter byte above 4 (that row is read as filter 0)
 *     An image with a non-zero status may hold anything, but nothing outside its own h * w * channels
 *     bytes is written; an image's result depends on its stream alone.  Everything runs on `stream`;
 *     no host synchronisation.  No input bytes can take the kernels out of bounds or make them loop:
 *     stream reads are clamped to sizes[i], table and window indices are masked, stores are checked
 *     against the image's own T bytes, and the symbol loop ends once the bits consumed exceed the
 *     stream's.  n <= 65535; stride in 1..2^31-1.
 * Arguments are validated before any HIP call: shape, empty batch (OK), stride, NULL. */
int nic_png_inspect(const uint8_t* host_file, int64_t size, int* h, int* w, int* channels, uint8_t* idat,
                    int64_t idat_capacity, int64_t* idat_bytes);
int nic_png_device_read_reserve(nic_ctx* ctx, int n, int h, int w, int channels);
int nic_png_device_read(nic_ctx* ctx, const uint8_t* streams, int64_t stride, const int64_t* sizes, int n, int h, int w,
                        int channels, uint8_t* images, int32_t* status, void* stream);

/* ---- Training side path (tf2_0/src/training.py:74-151): the step's convolutions ------------
 * NHWC fp32 device tensors, split-f16x3 MFMA (fp32-class), kernels of Keras layouts, no ctx.
 * Every forward and backward convolution of the step is one of two GEMMs:
 *
 * nic_conv_gather: y[b][oy][ox][co] = bias[co] + sum over taps (ky,kx), ci of
 *     x[b][src_y][src_x][ci] * W(ky,kx,ci,co), with
 *       transposed = 0: src = stride * o + k - pad   (Conv2D forward; input grad of Conv2DTranspose)
 *       transposed = 1: src = (o + pad - k) / stride, taps where it divides (Conv2DTranspose
 *                       forward; input grad of Conv2D)
 *     W(ky,kx,ci,co) = wt[((ky*kw+kx)*cin + ci)*cout + co]  (wt_layout 0, Conv2D HWIO)
 *                    = wt[((ky*kw+kx)*cout + co)*cin + ci]  (wt_layout 1, Conv2DTranspose HWOI)
 *     bias nullable; x_scale / w_scale nullable device floats (power-of-two operand scales from
 *     nic_absmax_scale, undone exactly in the epilogue).  work: 16-B aligned device scratch of
 *     nic_conv_gather_work() bytes (the split weights).  cin, cout <= 64.
 * nic_conv_gather_act: the same with act = 1 applying the layers' activation in the epilogue,
 *     y = leaky_relu(bias + sum, 0.2) (Keras Conv2D(..., activation=tf.nn.leaky_relu),
 *     encoder.py:10-17 / decoder.py:10-17); act = 0 is nic_conv_gather.
 * nic_act_bias_grad: the backward of that epilogue over a (rows, cols) NHWC tensor (rows = n h w):
 *     dz = dy * (act && !(y > 0) ? 0.2 : 1) (tf.nn.leaky_relu's gradient, from the layer's output
 *     y), db[c] = sum over rows of dz[row][c] (BiasAddGrad) and dz_scale[0] = nic_absmax_scale
 *     of dz, from one pass; any output may be NULL (not all; act = 0 and dz NULL: dz is dy).
 *     Deterministic (per-block column sums in `work`, added in block order); work must hold
 *     nic_act_bias_grad_work() floats.  cols <= 64.
 * nic_conv_wgrad: dw[ky][kx][a][b'] = sum over b, u of
 *     gat[b][stride*uy+ky-pad_y][stride*ux+kx-pad_x][a] * dir[b][uy][ux][b']
 *     (Conv2D: gat = x, dir = dy, dw HWIO; Conv2DTranspose: gat = dy, dir = x, dw HWOI);
 *     deterministic (per-slice partials in `work`, summed in order); work must hold
 *     nic_conv_wgrad_work() floats.  ca, cb <= 64.
 * nic_absmax_scale: scale[0] = 2^(13 - floor(log2 max|x|)), the exponent held to -126..126, and
 *     1 when the maximum is 0 or infinite, so the split-f16 operands keep every bit of tiny
 *     gradients.  The maximum is fmaxf's, which skips a NaN element: finite elements beside a
 *     NaN keep the scale of their own maximum (the NaN poisons only the sums it enters), and a
 *     tensor of NaNs alone gets 1.  count = 0 gives 1.  work >= 512 floats.
 * nic_gauss_1d: one-channel planes (n,h,w): VALID correlation with ntaps taps along x
 *     (vertical 0) or y, or its adjoint (the input gradient); the SSIM loss's separable
 *     Gaussian (tf.image.ssim, training.py:119-121).
 * The SSIM loss (tf.image.ssim, training.py:119-121) and the MS-SSIM loss (tf.image.ssim_multiscale
 * on one-channel fp32 planes; scale k is the 2x2 mean pool of scale k-1, an odd height or width
 * SYMMETRIC-padded by one on the far side first; the SSIM loss is scale 0 alone):
 * nic_msssim_terms: both means of one scale from its Gaussian-filtered terms in one pass: per pixel
 *     of n planes of hw pixels, from mx = G*x, my = G*y, sxy = G*(x y), sxx = G*(x^2 + y^2):
 *     num0 = (mx my) 2, den0 = mx mx + my my, lum = (num0 + c1)/(den0 + c1),
 *     cs = ((2 sxy - num0) + c2)/((sxx - den0) + c2), every op an fp32 rounding; ssim_mean[i] = mean
 *     of lum cs (tf.image.ssim's value), cs_mean[i] = mean of cs over plane i (deterministic:
 *     per-block partial sums, added in block order; work >= nic_msssim_terms_work() floats).
 * nic_msssim_terms_grad: the gradients of sum_i g_ssim[i] ssim_mean[i] + g_cs[i] cs_mean[i] with
 *     respect to mx, my, sxy, sxx; g_ssim and g_cs each hold n floats (zeros for a mean not used).
 * nic_pool2_prep: the step to the next scale of planes x, y (n,h,w), oh = ceil(h/2), ow = ceil(w/2):
 *     xp = 0.25 ((x[2i][2j] + x[2i][2j+1]) + (x[2i+1][2j] + x[2i+1][2j+1])), each op rounded, row h
 *     / column w of an odd size reading row h-1 / column w-1; yp likewise; and the planes the
 *     Gaussian reads next, pxy = xp yp, pss = xp xp + yp yp; all (n,oh,ow).
 *     mode NIC_POOL2_PREP: all four; NIC_POOL2_POOL: xp, yp only (pxy, pss ignored);
 *     NIC_POOL2_PRODUCTS: no pooling (scale 0): pxy = x y, pss = x x + y y, (n,h,w), and copies
 *     of x, y in xp, yp when those are not NULL.
 * nic_pool2_prep_grad: its adjoint: dx, dy (n,h,w) from the gradients dxp, dyp, dp, dq of the four
 *     outputs (each nullable: zero) and the saved xp, yp (needed with dp or dq); the repeated row
 *     and column of an odd size fold back onto the last real one; every element of dx, dy is
 *     written once, no atomics.  Same modes (NIC_POOL2_POOL ignores dp, dq).
 * The table rate loss (no counterpart in the reference's trainer): the code length of a latent under
 * a learnable per-channel table, the quantity .nic version 2 prices.  L is (groups * channels, 256)
 * fp32, L[r][j] = -log2 p_r(j); y is (m, h, w, channels) NHWC fp32, m % groups == 0; plane i belongs
 * to group i / (m / groups) and its channel c reads row r = group * channels + c.  Per element, every
 * op one fp32 rounding:
 *     v = fminf(fmaxf(255 y, 0), 255) (a NaN becomes 0; no index leaves the row),
 *     k = min((int)floorf(v), 254), t = v - k, bits = L[r][k] + t (L[r][k+1] - L[r][k]).
 * nic_rate_table: plane_bits[i] = sum of bits over plane i's h w channels elements (deterministic:
 *     per-block partial sums of 1,024 elements, added in block order).
 * nic_rate_table_grad: for an upstream g[i] per plane, dy = (255 g[i]) (L[r][k+1] - L[r][k]), every
 *     element written once, and dL[r][j] = sum over row r's elements of g (1 - t) at j = k plus g t at
 *     j = k + 1 (deterministic, no atomics: per-block tables built by one owner per word in pixel
 *     order, added in block order).  dy and dL are each nullable, not both; m = 0 zeroes dL.
 * Both take `work` of nic_rate_table_work() floats: max(m ceil(h w channels / 1024),
 *     groups ceil((m / groups) h w / 128) channels 256); nic_rate_table_grad reads it only with dL.
 *     channels <= 64; m h w channels and groups channels 256 must fit an int.
 * The context rate loss: the same under the row the left neighbour selects, the quantity .nic version
 * 3 prices (one implementation serves both losses: the table rate is its one-context instance).  L is (groups * channels, 3, 256) fp32, L[r][x][j] = -log2 p_{r,x}(j); anchors is
 * groups * channels bytes on the device; yc (m, h, w, channels), NULL meaning y, is the tensor the
 * contexts are read from; seg_pixels >= 1.  Element (i, q, c), q the row-major pixel inside plane i:
 *     x = 0 if q % seg_pixels == 0, otherwise
 *         min(2, |(int)rintf(fminf(fmaxf(255 yc[i][q-1][c], 0), 255)) - anchors[r]|)
 *     (rintf: to nearest, ties to even; "left" is the previous pixel in memory order inside the plane,
 *     across a row end the last pixel of the row above, never a pixel of another plane: q = 0 is
 *     always context 0 and yc[i][-1] is never read), then v, k, t as above and
 *     bits = L[r][x][k] + t (L[r][x][k+1] - L[r][x][k]).
 * nic_rate_ctable: plane_bits[i] as nic_rate_table's, in the same orders: with the three rows of every
 *     channel equal it returns nic_rate_table's bits bit for bit.
 * nic_rate_ctable_grad: dy = (255 g[i]) (L[r][x][k+1] - L[r][x][k]); dL[r][x][j] = sum over row r's
 *     elements in context x of g (1 - t) at j = k plus g t at j = k + 1 (deterministic, no atomics, as
 *     nic_rate_table_grad's, once per context).  Nothing flows to yc or through the left neighbour: the
 *     context is piecewise constant.  dy and dL are each nullable, not both; m = 0 zeroes dL.
 * Both take `work` of nic_rate_ctable_work() floats: max(m ceil(h w channels / 1024),
 *     3 groups ceil((m / groups) h w / 128) channels 256); nic_rate_ctable_grad reads it only with dL.
 *     Argument errors are nic_rate_table's, plus NIC_EINVAL for seg_pixels < 1 and NULL anchors.
 * nic_adam_keras: the step's optimiser update (training.py:147-149, tf.keras Adam = TF's
 *     ResourceApplyAdam) over `count` tensors in one launch; table = device int64 records
 *     {var, m, v, grad, n} (pointers to fp32 device buffers, n elements), max_n their largest n:
 *       m += (g - m)*(1 - beta1);  v += (g*g - v)*(1 - beta2);  var -= (m*alpha)/(sqrt(v) + epsilon)
 *     each op an fp32 rounding; alpha = lr*sqrt(1 - beta2^t)/(1 - beta1^t) from the caller. */
int nic_conv_gather_work(int kh, int kw, int cin, int cout, int64_t* bytes);
int nic_conv_gather(const float* x, int n, int h, int w, int cin, const float* wt, int kh, int kw, int wt_layout,
                    int stride, int pad_y, int pad_x, int transposed, const float* bias, const float* x_scale,
                    const float* w_scale, float* y, int oh, int ow, int cout, void* work, int64_t work_bytes,
                    void* stream);
int nic_conv_gather_act(const float* x, int n, int h, int w, int cin, const float* wt, int kh, int kw, int wt_layout,
                        int stride, int pad_y, int pad_x, int transposed, const float* bias, const float* x_scale,
                        const float* w_scale, float* y, int oh, int ow, int cout, int act, void* work,
                        int64_t work_bytes, void* stream);
int nic_act_bias_grad_work(int64_t rows, int cols, int64_t* floats);
int nic_act_bias_grad(const float* y, const float* dy, int64_t rows, int cols, int act, float* dz, float* db,
                      float* dz_scale, float* work, int64_t work_floats, void* stream);
int nic_conv_wgrad_work(int n, int uh, int uw, int kh, int kw, int ca, int cb, int64_t* floats);
int nic_conv_wgrad(const float* gat, int n, int gh, int gw, int ca, const float* dir, int uh, int uw, int cb, int kh,
                   int kw, int stride, int pad_y, int pad_x, const float* gat_scale, const float* dir_scale, float* dw,
                   float* work, int64_t work_floats, void* stream);
int nic_absmax_scale(const float* x, int64_t count, float* scale, float* work, void* stream);
int nic_gauss_1d(const float* in, int n, int h_in, int w_in, const float* taps, int ntaps, int vertical, int adjoint,
                 float* out, int h_out, int w_out, void* stream);
#define NIC_POOL2_PREP 0
#define NIC_POOL2_PRODUCTS 1
#define NIC_POOL2_POOL 2
int nic_msssim_terms_work(int n, int64_t hw, int64_t* floats);
int nic_msssim_terms(const float* mx, const float* my, const float* sxy, const float* sxx, int n, int64_t hw, float c1,
                     float c2, float* ssim_mean, float* cs_mean, float* work, int64_t work_floats, void* stream);
int nic_msssim_terms_grad(const float* mx, const float* my, const float* sxy, const float* sxx, const float* g_ssim,
                          const float* g_cs, int n, int64_t hw, float c1, float c2, float* gmx, float* gmy, float* gsxy,
                          float* gsxx, void* stream);
int nic_pool2_prep(const float* x, const float* y, int n, int h, int w, int mode, float* xp, float* yp, float* pxy,
                   float* pss, void* stream);
int nic_pool2_prep_grad(const float* dxp, const float* dyp, const float* dp, const float* dq, const float* xp,
                        const float* yp, int n, int h, int w, int mode, float* dx, float* dy, void* stream);
int nic_rate_table_work(int m, int h, int w, int channels, int groups, int64_t* floats);
int nic_rate_table(const float* y, const float* L, int m, int h, int w, int channels, int groups, float* plane_bits,
                   float* work, int64_t work_floats, void* stream);
int nic_rate_table_grad(const float* y, const float* L, const float* g, int m, int h, int w, int channels, int groups,
                        float* dy, float* dL, float* work, int64_t work_floats, void* stream);
int nic_rate_ctable_work(int m, int h, int w, int channels, int groups, int64_t* floats);
int nic_rate_ctable(const float* y, const float* yc, const float* L, const uint8_t* anchors, int m, int h, int w,
                    int channels, int groups, int seg_pixels, float* plane_bits, float* work, int64_t work_floats,
                    void* stream);
int nic_rate_ctable_grad(const float* y, const float* yc, const float* L, const uint8_t* anchors, const float* g, int m,
                         int h, int w, int channels, int groups, int seg_pixels, float* dy, float* dL, float* work,
                         int64_t work_floats, void* stream);
int nic_adam_keras(const int64_t* table, int count, int64_t max_n, float alpha, float beta1, float beta2,
                   float epsilon, void* stream);

/* Per-layer device timing.  With timing on, every kernel launch of encode/decode is
 * bracketed by a hipEvent pair on the caller's stream (the stream the kernel runs on);
 * nic_layer_times returns, per layer in the order conv1, conv2, conv3, conv4, conv8,
 * dconv1, dconv5, dconv6, dconv7, dconv8 (NIC_LAYER_COUNT entries), the summed
 * milliseconds and launch counts since timing was (re)enabled.  Both synchronise on
 * the recorded events. */
#define NIC_LAYER_COUNT 10
int nic_set_timing(nic_ctx* ctx, int enable);
int nic_layer_times(nic_ctx* ctx, double* ms_sum, int64_t* launches);

#ifdef __cplusplus
}
#endif

#endif /* NIC_H_ */
