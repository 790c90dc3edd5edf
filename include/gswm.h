/* gswm.h -- C ABI of the MI355X-native Gaussian-Shading watermark hot path (libgswm.so).
 *
 * Every entry point is what a binding of the reference's hot path would call; the reference
 * (lthero-big/A-watermark-for-Diffusion-Models @ 2024_08_07) is pure Python, so "the interface this
 * replaces" is a Python function body, cited as file:line relative to the reference root.
 *
 * Conventions
 *   - plain C symbols, plain pointers and sizes; no torch / C++ types cross the boundary
 *   - `*_dev` pointers are DEVICE (HBM) pointers owned by the caller; all other pointers are HOST
 *     pointers that are only read during the call (key, nonce, message are copied into the kernel
 *     arguments)
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every call is stream-ordered
 *     and asynchronous, never synchronises, never allocates device memory (exception: gsw_embed with a
 *     message longer than GSW_MSG_INLINE_MAX bytes stages it with hipMallocAsync/hipFreeAsync)
 *   - return value: 0 = GSW_OK, otherwise a gsw_status; no exceptions cross the boundary; no global
 *     mutable state (the in-kernel RNG is fully specified by seed + image index)
 *   - thread-safe for concurrent calls on distinct streams
 *   - per-image lattice is the C-contiguous [4, H/8, W/8] latent, addressed by flat element index
 *     i in [0, n_elems); batches are [B, n_elems] contiguous
 */
#ifndef GSWM_H
#define GSWM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libgswm.so is built with -fvisibility=hidden: only what this header declares is exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define GSW_VERSION 500 /* 0.5.0: every engine launch takes what it needs besides its operands in a caller-owned GswMmExtras (gsw_*_ex; the plain entry points request nothing); the thread-local one-shot side channels of ABI 0.3 (gsw_mm_next_colstats / gsw_mm_last_colstats / gsw_mm_next_rowstats / gsw_mm_last_rowstats / gsw_mm_set_workspace) and the round-1 aliases gsw_linear / gsw_attention_hd64 are gone; gsw_xattn_fused is new */

#define GSW_MSG_INLINE_MAX 256 /* message bytes carried inside the kernel arguments (2048 bit) */

typedef enum gsw_dtype {
    GSW_F32 = 0,
    GSW_F16 = 1,
    GSW_BF16 = 2,
    GSW_F64 = 3
} gsw_dtype;

typedef enum gsw_status {
    GSW_OK = 0,
    GSW_ERR_BAD_ARG = 1,     /* null pointer, bad dtype, non-positive size, n_elems % 4 != 0 ...        */
    GSW_ERR_UNSUPPORTED = 2, /* lattice too large for the LDS-resident vote             */
    GSW_ERR_RAGGED = 3,      /* 8*ceil(n_elems/8) is not a multiple of msg_bits: the reference raises
                                IndexError at extract.py:98                                             */
    GSW_ERR_HIP = 4,         /* a HIP runtime call failed; gsw_last_hip_error() has the hipError_t      */
    GSW_WARN_NO_RECORDS = 5  /* (ABI < 0.5.0: the one-shot record queries reported a dropped request with it; a launch now says what it wrote in
                                GswMmExtras.colstats_rows_per_block / rowstats_slots -- 0 means: take the statistics pass instead) */
} gsw_status;

/* embed flags */
#define GSW_EMBED_EXACT_F64 0u /* Cephes ndtri evaluated in fp64, then rounded (== scipy to <= a few fp64 ulp) */
#define GSW_EMBED_FAST_F32 1u  /* fp32 core on the tail-safe side of the distribution; |dz| <= 1e-5       */

/* per-image flag bits written by gsw_extract */
#define GSW_FLAG_SATURATED 1u /* some z >= 8.292361075813597: norm.cdf == 1.0, y == 2 (extract.py:84-86 raises ValueError) */
#define GSW_FLAG_NAN 2u       /* some z is NaN (int(nan) raises ValueError at extract.py:84)            */

int gsw_version(void);
/* Measurement switches the library was COMPILED with (csrc/gswm_ablate.inc: cycle stamps, ablations of the matmul engine's main loop -- builds that compute
 * wrong results by design).  A shippable library returns 0; tests/test_kernel_metadata.py and the loader (_native.lib) refuse anything else. */
int gsw_build_flags(void);
const char* gsw_strerror(int status);
int gsw_last_hip_error(void); /* thread-local hipError_t of the last GSW_ERR_HIP on this thread */

/* E2 -- gs_insert.py:45-47 / extract.py:77-78,87: the ChaCha20 stream `cryptography` (OpenSSL) produces for
 * Cipher(algorithms.ChaCha20(key, nonce16)): nonce16[0:4] = LE32 initial block counter (carry into the next
 * word), nonce16[4:16] = RFC 8439 nonce.  Writes `nbytes` keystream bytes to out_dev. */
int gsw_keystream(const uint8_t key[32], const uint8_t nonce16[16], uint8_t* out_dev, size_t nbytes, void* stream);

/* E1-E6 -- gs_insert.py:8-66 (and the generalised lattice of ComfyUI_GSWaterMark/nodes.py:51-123), batched.
 *   msg/msg_bytes : the padded watermark k (gs_insert.py:9-20); plaintext = k repeated floor(n_elems/(8*msg_bytes))
 *                   times then zeros (nodes.py:79-87)
 *   u_dev         : optional [B, n_elems] float64 uniforms in [0,1) (the reference's np.random.uniform draws,
 *                   gs_insert.py:62) -- bit-parity mode.  NULL => in-kernel Philox4x32-7 (Random123 philox4x32_R(7)) keyed by `seed`,
 *                   counter = (element index >> 2, image_index0 + b), one 32-bit word per element, u = (w + 1/2) 2^-32:
 *                   results do not depend on batch split
 *                   or GPU count.
 *   out_dev       : [B, n_elems] of out_dtype; z = ndtri((u + y) / 2) (gs_insert.py:64), y = cipher bit,
 *                   MSB-first within each cipher byte (gs_insert.py:49)
 *   n_elems       : 4 * (H/8) * (W/8); must be a multiple of 4 */
int gsw_embed(const uint8_t key[32], const uint8_t nonce16[16], const uint8_t* msg, int msg_bytes,
              const double* u_dev, uint64_t seed, uint64_t image_index0, void* out_dev, int out_dtype, int B,
              int64_t n_elems, uint32_t flags, void* stream);

/* In-kernel RNG only: writes the u the kernel would draw ([B, n_elems] float64) so a CPU oracle can be run on
 * exactly the same inputs. */
int gsw_philox_uniform(uint64_t seed, uint64_t image_index0, double* u_dev, int B, int64_t n_elems, void* stream);

/* X3-X5 -- extract.py:72-101, batched: y = int(norm.cdf(float64(z)) * 2) per element in C order, pack MSB-first,
 * ChaCha20-decrypt, split into msg_bits-wide segments, strict-majority vote per bit (ties -> 0).
 *   z_dev      : [B, n_elems] of z_dtype
 *   bits_dev   : [B, ceil(msg_bits/8)] recovered message, MSB-first (bit t -> byte t>>3, bit 7-(t&7))
 *   counts_dev : optional [B, msg_bits] uint32 number of '1' votes per bit (NULL to skip)
 *   flags_dev  : [B] uint32 GSW_FLAG_* (the reference raises for such images; the host wrapper does too)
 * Returns GSW_ERR_RAGGED when the reference would raise IndexError. */
int gsw_extract(const void* z_dev, int z_dtype, const uint8_t key[32], const uint8_t nonce16[16], int msg_bits,
                uint8_t* bits_dev, uint32_t* counts_dev, uint32_t* flags_dev, int B, int64_t n_elems, void* stream);

/* X6 -- extract.py:103-110 on device: matches_dev[b] = number of equal bits between bits_dev[b] and the
 * reference message over the first min(msg_bits, ref_bits) positions. */
int gsw_bit_matches(const uint8_t* bits_dev, int msg_bits, const uint8_t* ref_msg, int ref_bits,
                    uint32_t* matches_dev, int B, void* stream);

/* X2 / G1 -- the elementwise update of the DDIM (eta = 0) sampling / inversion loop
 * (inverse_stable_diffusion_gs.pyc `backward_ddim`; diffusers DDIMScheduler/DDIMInverseScheduler.step):
 *   out = a * x + b * model_out            (a, b precomputed per step on the host in fp64)
 * computed in fp32, one rounding to `dtype`.  out_dev may alias x_dev. */
int gsw_ddim_step(const void* x_dev, const void* model_out_dev, void* out_dev, float a, float b, int dtype,
                  int64_t n, void* stream);

/* G1 with classifier-free guidance fused (modified_stable_diffusion_gs.pyc: uncond + g * (text - uncond), then the
 * scheduler step): out = a * x + b * (e_uncond + g * (e_text - e_uncond)). */
int gsw_ddim_step_cfg(const void* x_dev, const void* e_uncond_dev, const void* e_text_dev, void* out_dev, float a,
                      float b, float guidance, int dtype, int64_t n, void* stream);

/* G1 / X2 -- one whole DPM-Solver++ multistep (2M, data prediction, midpoint) scheduler step, sampling or inversion:
 *   e  = e_text ? e_uncond + g * (e_text - e_uncond) : e_uncond
 *   m0 = P * x + Q * e                     (the x0 prediction, rounded to `dtype` exactly as gsw_ddim_step[_cfg] rounds it)
 *   x' = A * x + B * m0 + C * m_prev       (m0 as stored; the C term only when m_prev is given and C != 0)
 * fp32 math, coefficients precomputed per step on the host in fp64; x' -> x_out_dev, m0 -> m_out_dev.  x_out_dev may alias x_dev,
 * m_out_dev may alias m_prev_dev.  m_prev_dev is not read when C == 0.  GSW_ERR_BAD_ARG for m_prev_dev == NULL with C != 0. */
int gsw_dpm_step(const void* x_dev, const void* e_uncond_dev, const void* e_text_dev /* NULL: no guidance */,
                 const void* m_prev_dev /* NULL: first order */, void* x_out_dev, void* m_out_dev, float P, float Q, float A,
                 float B, float C, float guidance, int dtype, int64_t n, void* stream);

/* Last inversion step fused with the extract tail: z = a * x + b * model_out is voted on directly (and stored to
 * z_out_dev when non-NULL, in `dtype`, after the same rounding an unfused gsw_ddim_step would apply). */
int gsw_ddim_step_extract(const void* x_dev, const void* model_out_dev, void* z_out_dev, float a, float b, int dtype,
                          const uint8_t key[32], const uint8_t nonce16[16], int msg_bits, uint8_t* bits_dev,
                          uint32_t* counts_dev, uint32_t* flags_dev, int B, int64_t n_elems, void* stream);

/* X2 / G1 -- elementwise fusions inside the eps model (the UNet the DDIM loops call; in the reference this is diffusers'
 * ResnetBlock2D / GEGLU running as separate torch kernels):
 *   gsw_groupnorm_silu: out = act(GroupNorm_groups(x + pre_bias[b, c]) * gamma[c] + beta[c]); x, out: [B, C, HW] (NCHW), HW % 8 == 0;
 *                       pre_bias: optional [B, C] (the time-embedding projection added before norm2); act: 0 none, 1 SiLU
 *   gsw_geglu:          out[r, i] = in[r, i] * gelu(in[r, inner + i]); in: [rows, 2*inner], out: [rows, inner], inner % 8 == 0 */
int gsw_groupnorm_silu(const void* x_dev, const void* pre_bias_dev, const void* gamma_dev, const void* beta_dev, void* out_dev, int B, int C,
                       int HW, int groups, float eps, int act, int dtype, void* stream);
int gsw_geglu(const void* in_dev, void* out_dev, int64_t rows, int inner, int dtype, void* stream);

/* X2 / G1 -- convolution of the eps model as an MFMA implicit GEMM on "padded-flat NHWC" (PF) activations
 * (replaces diffusers' Conv2d -> MIOpen in ResnetBlock2D / Downsample2D / conv_shortcut):
 *   PF tensor: [B*(H+2)*(W+2)] rows x C channels, row (b, y, x) = b*(H+2)*(W+2) + y*(W+2) + x, zero border, plus (W+3) zero guard
 *              rows before row 0 and after the last row (x_dev points at row 0).
 *   y[m, n] = sum_taps sum_c x[row(m) + off_tap, c] * w[n, tap*C + c] + bias[n] + rowbias[b(m), n] + resid[m, n]; border rows = 0
 *   w_dev: [N][ksize*ksize*C] (tap-major, channel-minor), ksize 1 or 3, stride 1 or 2 (3x3 only); H, W = OUTPUT size;
 *   ldx: row stride of x in elements; C % 64 == 0; N % 8 == 0 from 128 channels up (the matmul engine, csrc/gswm_mm.hip; a partial last 160-column
 *   tile costs a full one), N % 64 == 0 below that (the 64-column kernel of round 1: the 4-channel edges padded to one tile);
 *   dtype GSW_F16 / GSW_BF16; bias / rowbias / resid optional.  rowbias: [B] rows, ld_rowbias elements apart (0 = N; else >= N and a
 *   multiple of 8): the time-embedding projections of ALL resnets come out of one GEMM, each convolution reads its column slice. */
int gsw_conv_pf(const void* x_dev, const void* w_dev, const void* bias_dev, const void* rowbias_dev, int ld_rowbias, const void* resid_dev, void* y_dev,
                int B, int H, int W, int C, int N, int ksize, int stride, int ldx, int dtype, void* stream);

/* GroupNorm (+SiLU) on a PF tensor: out = act(GroupNorm(x) * gamma + beta); out is a PF tensor (zero border) or, with out_tokens = 1,
 * dense tokens [B, H*W, C] (the transformer's input).  workspace_dev: >= B * 64 * groups * 2 floats.  C % 8 == 0, groups <= 64. */
int gsw_groupnorm_pf(const void* x_dev, const void* gamma_dev, const void* beta_dev, void* out_dev, float* workspace_dev, int B, int H, int W,
                     int C, int groups, float eps, int act, int out_tokens, int dtype, void* stream);

/* Same with two sources: GroupNorm over the channel concatenation [x (Ca channels) | x2 (C - Ca channels)] read in place (the UNet's
 * skip connections are never materialised as a torch.cat). */
int gsw_groupnorm_pf2(const void* x_dev, const void* x2_dev, int Ca, const void* gamma_dev, const void* beta_dev, void* out_dev, float* workspace_dev,
                      int B, int H, int W, int C, int groups, float eps, int act, int out_tokens, int dtype, void* stream);

/* ---- Extras of a matmul-engine launch (ABI 0.4.0; the only form since 0.5.0).  Everything a launch needs besides its operands travels in ONE caller-owned
 * struct: no thread-local "arm, then launch" state, nothing shared between two streams of one thread, and what the launch actually did comes back in the
 * same struct.  NULL in place of a GswMmExtras* means "no records, no split-K".
 *   colstats_dev / colstats_capacity : in  -- GroupNorm statistics without a pass over the tensor: a convolution / token-scatter launch (gsw_conv_pf_ex,
 *                          gsw_conv3x3_res_pf_ex, gsw_conv_up2x_pf_ex, gsw_gemm_ex with GSW_GEMM_TOK2PF) also writes, per block of 32 or 64 consecutive output pixels and per
 *                          PAIR of output columns (2c, 2c + 1), the sum and the sum of squares of the values it stores: [npar][blocks][2 planes: sums | sums of squares][N / 2]
 *                          floats, npar = 1 (4 for gsw_conv_up2x_pf_ex: one quarter of the buffer per parity launch, records over the low-resolution pixels);
 *                          capacity >= npar * ceil(M / 128) * 4 * N floats covers either tile height (M = output pixels of ONE launch); 16-byte aligned (NULL: none)
 *   rowstats_dev / rowstats_capacity : in  -- LayerNorm statistics likewise: a plain gsw_gemm_ex (+ residual) also writes, per output row and 80-column half tile, the
 *                          (sum, sum of squares) of what it stores: [M][slots][2] floats, capacity >= M * 2 ceil(N / 160) * 2 (NULL: none)
 *   workspace_dev / workspace_bytes / max_splits : in -- split-K scratch (caller-owned device memory, 16-byte aligned, on the device of the launch's stream) and policy.
 *                          Small-batch launches of the eps model -- one image's 8 x 8 level is a single 64-row tile against 180-360 K stages (the reference's own use:
 *                          extract.py:112-117 inverts ONE latent per call) -- cannot fill 256 CUs with output tiles.  With a workspace, a launch whose 128- or 256-row
 *                          tiling has <= 128 tiles lets up to 32 workgroups share a tile's K stages (at most 256 workgroups in all) whenever the engine's cost model
 *                          (fitted to tools/splitk_tile_sweep.py) predicts a gain of 5 % or more: each workgroup dumps its fp32 accumulators into a slab and a second
 *                          kernel adds the slabs in split order (deterministic) and runs the epilogue of the launch's mode.  40 MiB covers every launch (256 slabs of
 *                          160 KiB: 256-row tiles; 128-row tiles need half).  The workspace is scratch between a launch and its reduce kernel, both on the launch's
 *                          stream: launches on ONE stream may share it, launches on different streams need different workspaces.  max_splits: 0 = automatic, 1 = never
 *                          split, k > 1 = split every launch min(k, stages, 256 / tiles) ways (parity tests).  (NULL / 0 bytes: the launch runs unsplit)
 *   colstats_rows_per_block, colstats_blocks : out -- 0 / 0 when the launch wrote no column records (it split K, enumerated whole tensors, ...)
 *   rowstats_slots : out -- records per row written (0: none)
 *   splits         : out -- K splits of the launch (1: unsplit)
 *   flags          : in  -- 0, or GSW_MM_GN_ONLY (ABI 0.4.1; the word sits in what was tail padding: zero-initialise the struct): the PF output of this convolution
 *                           is read by nothing but a GroupNorm that takes its statistics from the column records requested here.  The launch then leaves the
 *                           one-pixel border of the output UNWRITTEN when (and only when) it wrote those records: the GroupNorm kernels never read it (the apply
 *                           kernel writes zeros to its own output's border whatever the input's holds) -- one small launch less per resnet. */
#define GSW_MM_GN_ONLY 1
typedef struct GswMmExtras {
    float* colstats_dev;
    int64_t colstats_capacity;
    float* rowstats_dev;
    int64_t rowstats_capacity;
    void* workspace_dev;
    int64_t workspace_bytes;
    int max_splits;
    int colstats_rows_per_block, colstats_blocks, rowstats_slots, splits;
    int flags;
} GswMmExtras;

/* gsw_gemm_strided / gsw_gemm_ln / gsw_conv_pf / gsw_conv3x3_res_pf / gsw_conv_up2x_pf with extras (ex may be NULL; the plain entry points ARE ex = NULL). */
int gsw_gemm_ex(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* bias_dev, const void* resid_dev, int64_t ldr, void* y_dev, int64_t ldy,
                int64_t M, int K, int N, int mode, int S, int Wimg, int dtype, GswMmExtras* ex, void* stream);
/* Dense GEMM whose A operand lies in TWO column blocks (additive: the version stays 500): Y = [x0 | x1] W^T (+ bias + resid), x0 [M][ld0] with K0 columns,
 * x1 [M][ld1] with K1 columns, W [N][K0 + K1] (the columns that multiply x1 start at K0).  The engine walks the two blocks as K segments with their own row
 * strides, like the three-segment convolution of the resnet tail, so a product of two linear maps folded into one weight -- Transformer2DModel's
 * proj_out(x + ff.net[2](h)) = [h | x] [Wp W2 | Wp]^T + (Wp b2 + bp) -- runs as ONE launch and the intermediate tensor is never written.
 *   mode GSW_GEMM_TOK2PF : as the one-operand entry (in-place resid == y, column records through ex); every tiling of the PF-row epilogue, the 256 x 320 tile included.
 *        GSW_GEMM_PLAIN  : dense rows (+ resid), on the 128- / 256-row tiles only: the wide tile's dense-row producer addresses ONE dense operand, so a two-block
 *                          launch never takes it by itself, and where the caller forces it (gsw_mm_config tile_rows = 512) on a shape it is legal for
 *                          (M % 256 == 0, N % 320 == 0) the call returns GSW_ERR_UNSUPPORTED without launching -- unless the plan splits the launch
 *                          along K (a workspace in ex and few output tiles): a split launch runs the narrow split kernels whatever the tile knob
 *                          says, with one block or two, and succeeds.
 *        GSW_GEMM_GEGLU / GSW_GEMM_TRANS : GSW_ERR_UNSUPPORTED.
 * Validation as the one-operand entry, per block: K0 % 64, K1 % 64, ld_i >= K_i, ld_i % 8, ldw >= K0 + K1 (else GSW_ERR_UNSUPPORTED); x1_dev NULL: GSW_ERR_BAD_ARG. */
int gsw_gemm2_ex(const void* x0_dev, int64_t ld0, int K0, const void* x1_dev, int64_t ld1, int K1, const void* w_dev, int64_t ldw, const void* bias_dev,
                 const void* resid_dev, int64_t ldr, void* y_dev, int64_t ldy, int64_t M, int N, int mode, int S, int Wimg, int dtype, GswMmExtras* ex, void* stream);
int gsw_gemm_ln_ex(const void* x_dev, const float* ln_stat_dev, const void* w_dev, const float* u_dev, const float* v_dev, void* y_dev, int64_t M, int K, int N,
                   int mode, int S, int dtype, GswMmExtras* ex, void* stream);
int gsw_conv_pf_ex(const void* x_dev, const void* w_dev, const void* bias_dev, const void* rowbias_dev, int ld_rowbias, const void* resid_dev, void* y_dev,
                   int B, int H, int W, int C, int N, int ksize, int stride, int ldx, int dtype, GswMmExtras* ex, void* stream);
int gsw_conv3x3_res_pf_ex(const void* x_dev, const void* w_dev, const void* bias_dev, const void* rowbias_dev, int ld_rowbias, const void* resid_dev, void* y_dev,
                          int B, int H, int W, int C, int N, const void* x1_dev, int C1, const void* x2_dev, int C2, int dtype, GswMmExtras* ex, void* stream);
int gsw_conv_up2x_pf_ex(const void* x_dev, const void* w4_dev, const void* bias_dev, void* y_dev, int B, int H, int W, int C, int N, int dtype, GswMmExtras* ex,
                        void* stream);

/* gsw_groupnorm_pf2 with the statistics folded from the column records of the producing launches (GswMmExtras.colstats_*; cs*_rows = rows per block the launch
 * reported, cs*_blocks = blocks per parity buffer, i.e. the buffer's stride): pixels per image must be a multiple of the block rows and the groups an even number
 * of channels wide; workspace_dev >= max(B * 64 * groups * 2, B * C) floats. */
int gsw_groupnorm_pf_cs(const void* x_dev, const void* x2_dev, int Ca, const float* cs1_dev, int cs1_rows, int cs1_npar, int cs1_blocks,
                        const float* cs2_dev, int cs2_rows, int cs2_npar, int cs2_blocks, const void* gamma_dev, const void* beta_dev, void* out_dev,
                        float* workspace_dev, int B, int H, int W, int C, int groups, float eps, int act, int out_tokens, int dtype, void* stream);

/* ResnetBlock2D tail in ONE GEMM: y = conv3x3(x) + conv1x1([x1 | x2]) + bias + rowbias + resid on PF tensors.
 * w_dev: [N][9*C + C1 + C2] (3x3 taps first, then the shortcut's columns), x1 / x2 optional (x2 requires x1). */
int gsw_conv3x3_res_pf(const void* x_dev, const void* w_dev, const void* bias_dev, const void* rowbias_dev, int ld_rowbias, const void* resid_dev, void* y_dev,
                       int B, int H, int W, int C, int N, const void* x1_dev, int C1, const void* x2_dev, int C2, int dtype, void* stream);

/* Transformer blocks of the eps model: xnew = x + delta (skipped when delta_dev is NULL), y = LayerNorm(xnew) * gamma + beta;
 * x, delta, xnew, y: [rows, C]; C % 8 == 0, C <= 1536; GSW_F16 / GSW_BF16. */
int gsw_add_layernorm(const void* x_dev, const void* delta_dev, const void* gamma_dev, const void* beta_dev, void* xnew_dev, void* y_dev,
                      int64_t rows, int C, float eps, int dtype, void* stream);

/* Round-1 name of the dense linear layer: gsw_gemm(mode = geglu ? GSW_GEMM_GEGLU : GSW_GEMM_PLAIN). */

/* X2 / G1 -- every dense linear layer of the eps model (diffusers BasicTransformerBlock / Transformer2DModel / TimestepEmbedding /
 * ResnetBlock2D.time_emb_proj, which the reference reaches through `pipe(...)` at extract.py:66-69) on the hand-written matmul engine
 * (csrc/gswm_mm.hip: persistent 256 x 160 tiles, 8 waves in lockstep, three-stage LDS-DMA ring of 64-wide K slices):
 *   x: [M, K] row-major, w: [N, K] (nn.Linear layout), bias: [N] or NULL (PLAIN / GEGLU: 16-byte aligned -- the epilogue fetches it by LDS-DMA;
 *   GSW_ERR_BAD_ARG otherwise); K % 64 == 0, N % 8 == 0 (N % 160 == 0 for GEGLU; a partial last 160-column tile costs a full one); GSW_F16 / GSW_BF16.
 *   mode GSW_GEMM_PLAIN : y[M, N] = x w^T + bias (+ resid[M, N])
 *        GSW_GEMM_GEGLU : rows of w / bias interleaved per 16-ROW BLOCK as [8 value | 8 gate]: with I = N / 2 outputs, packed row
 *                         16 j + r holds value row 8 j + r for r < 8 and gate row I + 8 j + (r - 8) for r >= 8 of diffusers' [2 I, K]
 *                         projection (pf.pack_geglu_weight; bias packed the same way).  y[M, N/2] = value * gelu(gate) -- diffusers'
 *                         GEGLU without the [M, N] intermediate.  (ABI 0.1.x documented a per-160-row-tile [80 | 80] packing that the
 *                         engine never implemented since 0.2.0: GSW_VERSION >= 200 means the 16-row packing.)
 *        GSW_GEMM_TRANS : y[M/S][N][S] = per-image transpose of x w^T + bias (the attention kernel's V^T operand); S % 8 == 0
 *        GSW_GEMM_TOK2PF: rows are tokens (b, y, x) of S = H*W-token images of width Wimg; y_dev is row 0 of a padded-flat NHWC tensor
 *                         [B, H+2, W+2, N] and token rows land on its interior rows: y[pf(m)] = x w^T + bias (+ resid[pf(m)], which may
 *                         alias y: Transformer2DModel's `proj_out(...) + residual` in place) */
#define GSW_GEMM_PLAIN 0
#define GSW_GEMM_GEGLU 1
#define GSW_GEMM_TRANS 2
#define GSW_GEMM_TOK2PF 3
int gsw_gemm(const void* x_dev, const void* w_dev, const void* bias_dev, const void* resid_dev, void* y_dev, int64_t M, int K, int N,
             int mode, int S, int Wimg, int dtype, void* stream);
/* Self-attention's q | k | v projections from ONE pass over the tokens (diffusers Attention.to_q / to_k / to_v behind extract.py:66-69): w = the three
 * weights row-concatenated [N][K]; columns [0, N_rows) of x w^T (+ bias) -> rows_dev [M, N_rows] (q | k, read by gsw_attention as column slices),
 * columns [N_rows, N) -> trans_dev [M / S][N - N_rows][S] (V transposed).  N_rows % 160 == 0 (a column tile is either kind); K % 64, N % 8, S % 8 == 0. */
int gsw_gemm_qkv(const void* x_dev, const void* w_dev, const void* bias_dev, void* rows_dev, void* trans_dev, int64_t M, int K, int N_rows, int N,
                 int S, int dtype, void* stream);

/* LayerNorm folded into the GEMM that consumes it (diffusers BasicTransformerBlock: norm1 -> to_q | to_k | to_v, norm2 -> to_q, norm3 -> the GEGLU
 * projection): LN(x) W^T + b = rstd_m (x W'^T)_mn - rstd_m mean_m u_n + v_n with W' = W diag(gamma), u = W' 1, v = W beta + b -- the normalised tensor
 * is never written or read.
 *   row records          : GswMmExtras.rowstats_* of the launch that PRODUCES x (rowstats_slots records per row come back)
 *   gsw_ln_rowstats_finish: records -> stat_dev float2 [M] = (rstd, -rstd * mean) over the C columns.
 *   gsw_gemm_ln          : the consuming GEMM; w_dev = W' (GEGLU: packed like gsw_gemm), u_dev / v_dev fp32 [N] in the same row order, 16-byte aligned;
 *                          mode GSW_GEMM_PLAIN / GSW_GEMM_GEGLU / GSW_GEMM_TRANS; M % 8 == 0. */
int gsw_ln_rowstats_finish(const float* records_dev, int slots, int64_t M, int C, float eps, float* stat_dev, void* stream);
int gsw_gemm_ln(const void* x_dev, const float* ln_stat_dev, const void* w_dev, const float* u_dev, const float* v_dev, void* y_dev, int64_t M, int K, int N,
                int mode, int S, int dtype, void* stream);

/* The same with explicit row strides (elements, multiples of 8): x rows ldx >= K, w rows ldw >= K, resid rows ldr, y rows ldy -- operands may be
 * column slices of wider matrices (the per-image Q K^T and P V products of the VAE's single-head attention). */
int gsw_gemm_strided(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* bias_dev, const void* resid_dev, int64_t ldr,
                     void* y_dev, int64_t ldy, int64_t M, int K, int N, int mode, int S, int Wimg, int dtype, void* stream);

/* Process-wide tuning knobs of the matmul engine, for parity tests and A/B measurements only (production leaves both on "auto"; this is the
 * one piece of global state behind the ABI, also settable through the environment as GSW_MM_BM / GSW_MM_SPLIT before the first launch):
 *   tile_rows  : 0 = automatic (the 256 x 320 tile for long-K launches with several rounds of such tiles -- GSW_MM_WIDE is its per-epilogue bit mask --, else
 *                256 x 160 tiles unless they would leave CUs without one, then 128 x 160), 128 or 256 = forced narrow tiles, 512 = the 256 x 320 tile
 *                wherever it is legal (N % 320 == 0, dense rows / PF rows / GEGLU epilogues, operands below 4 GiB); -1 = keep
 *   split_mask : bit e set = epilogue kind e (0 dense rows -- 128-row tiles only: the 256-row dense-row tile has no 12-wave form --, 1 PF / convolution, 2 GEGLU, 3 transposed) runs the 12-wave variant whose
 *                waves 8-11 own the LDS-DMA; -1 = keep (default 10: convolutions and the transposed projection) */
int gsw_mm_config(int tile_rows, int split_mask);
int gsw_mm_get_config(int* tile_rows, int* split_mask); /* the current values (either pointer may be NULL): what a captured launch sequence depends on */

/* X1 / G1 tail -- diffusers AutoencoderKL mid-block attention (one head as wide as the block, 512): softmax over the rows of the score matrix
 * between the two engine products.  In place: x[r, 0:cols] <- softmax(scale * x[r, 0:cols]); rows `ld` elements apart; cols % 8 == 0; a scale that is not
 * finite and > 0 returns GSW_ERR_BAD_ARG. */
int gsw_softmax_rows(void* x_dev, int64_t rows, int cols, int64_t ld, float scale, int dtype, void* stream);

/* ---- The small-batch regime of the eps model (csrc/gswm_small.hip).  The reference inverts ONE latent per call (extract.py:112-117: 50 UNet
 * evaluations of one 4x64x64 latent), BASELINE configs[1] is batch 8: a forward is then a chain of ~500 dependent launches of 5-20 us, each paying
 * the ~4.7 us floor of a kernel boundary plus its own fill and drain, so what counts is FEWER and SHORTER launches.
 *
 * gsw_groupnorm_pf_fused: gsw_groupnorm_pf2 in ONE launch (no workspace): one workgroup per (image, group) holds the group's values in registers
 *   between the statistics and the normalisation (exact two-pass variance).  Groups an even number of channels wide; returns GSW_ERR_UNSUPPORTED
 *   when a group does not fit one workgroup's registers (more than 32 image rows per row lane, or an image row of the group wider than 1024 threads: use gsw_groupnorm_pf2 then) -- meant for B * groups
 *   up to a few hundred workgroups.
 * gsw_gather_rows: out[b] = table[clamp(index[b * index_stride], 0, nrows - 1)] (index_stride 0: one index for all rows): the time-embedding chain
 *   of diffusers' UNet2DConditionModel (sinusoid -> linear -> SiLU -> linear -> SiLU -> every resnet's time_emb_proj) depends on the timestep only,
 *   so it is tabulated once over the num_train_timesteps integer timesteps and a forward gathers its rows.  16-byte aligned rows.
 * gsw_nchw_to_pf: latent [B, Cin, H, W] -> PF rows [B, H+2, W+2, Cp]: zero border, channels >= Cin zero (conv_in reads one 64-wide K block).
 * gsw_conv3x3_pf_nchw: 3x3 stride-1 convolution of a PF tensor with Nout <= 16 output channels, written as NCHW [B, Nout, H, W] (+ bias): the
 *   UNet's conv_out (320 -> 4; diffusers UNet2DConditionModel.conv_out behind extract.py:66-69).  w: [Nout][9 * C] tap-major, channel-minor; C % 32 == 0. */
int gsw_groupnorm_pf_fused(const void* x_dev, const void* x2_dev, int Ca, const void* gamma_dev, const void* beta_dev, void* out_dev, int B, int H, int W,
                           int C, int groups, float eps, int act, int out_tokens, int dtype, void* stream);
int gsw_gather_rows(const void* table_dev, int64_t ld_bytes, int64_t nrows, const int64_t* index_dev, int index_stride, void* out_dev, int64_t out_ld_bytes,
                    int B, int64_t row_bytes, void* stream);
int gsw_nchw_to_pf(const void* x_dev, void* y_dev, int B, int Cin, int H, int W, int Cp, int dtype, void* stream);
int gsw_conv3x3_pf_nchw(const void* x_dev, const void* w_dev, const void* bias_dev, void* y_dev, int B, int H, int W, int C, int Nout, int dtype, void* stream);

/* Dense linears of the transformer blocks at SMALL M (one or two images: 64 ... 16384 token rows), where the engine's 128 x 160 tiles leave most CUs
 * without one: a four-wave workgroup owns a 64 x 64 / 32 x 64 / 16 x 64 / 16 x 32 output tile (config 0 .. 3; -1 = gsw_gemm_small_config's choice),
 * splits K four ways INSIDE the workgroup (fragments straight from global memory, partial tiles added in wave order through LDS: deterministic, no
 * second launch) and runs the epilogue of `mode` (GSW_GEMM_PLAIN / GEGLU / TRANS / TOK2PF, operands as for gsw_gemm_strided) with the engine's
 * rounding points.  K % 32 == 0, K >= 128, M % 16 == 0, N % 16 == 0 (GEGLU: N % 32 == 0), M <= 16384; 32-bit element offsets.
 *   ln_records_dev : LayerNorm fold (see gsw_gemm_ln) straight from the RAW row records [M][ln_slots][2] the producer of x left -- no finishing launch;
 *                    then w_dev = W diag(gamma), ln_u_dev / ln_v_dev fp32 [N] (16-byte aligned), bias_dev must be NULL; NULL = plain bias epilogue
 *   rowstats_dev   : GSW_GEMM_PLAIN only, optional: per output row and column tile the (sum, sum of squares) of the stored values,
 *                    [M][*rowstats_slots][2] floats, *rowstats_slots = ceil(N / tile columns) (0 when none were written);
 *                    capacity >= M * ceil(N / 32) * 2 covers every configuration.
 * gsw_gemm_small_config: the configuration the kernel would pick for a shape, or -1 when the shape is not this kernel's. */
int gsw_gemm_small_config(int64_t M, int K, int N, int mode);
int gsw_gemm_small(const void* x_dev, int64_t ldx, const void* w_dev, int64_t ldw, const void* bias_dev, const void* resid_dev, int64_t ldr, void* y_dev, int64_t ldy,
                   int64_t M, int K, int N, int mode, int S, int Wimg, const float* ln_records_dev, int ln_slots, float ln_eps, const float* ln_u_dev,
                   const float* ln_v_dev, float* rowstats_dev, int64_t rowstats_capacity, int* rowstats_slots, int config, int dtype, void* stream);

/* diffusers Upsample2D (nearest 2x + 3x3 convolution) from the low-resolution PF input, by sub-pixel decomposition: w4 =
 * [4 output parities (dy*2+dx)][N][4 taps (a*2+b)][C], the 3x3 weights pre-summed over the taps that read the same source pixel
 * (pf.pack_upsample_weight).  y: PF [B, 2H, 2W, N] (interior rows from the four parity launches, border rows zeroed here). */
int gsw_conv_up2x_pf(const void* x_dev, const void* w4_dev, const void* bias_dev, void* y_dev, int B, int H, int W, int C, int N, int dtype,
                     void* stream);

/* Attention of the eps-model (diffusers BasicTransformerBlock.attn1 / attn2 inside the UNet the reference runs at extract.py:66-69):
 * out = softmax(q k^T * scale) v per (batch, head), fp16 / bf16, fp32 accumulation -- a flash-attention forward.
 *   head_dim : 64 (SD 2.x), 40 / 80 / 160 (SD 1.x levels with 8 heads); other widths return GSW_ERR_UNSUPPORTED
 *   q   : [B, Sq, >= H*head_dim] row stride ldq elements, head h in columns [h*head_dim, (h+1)*head_dim)
 *   k   : [B, Sk, >= H*head_dim] row stride ldk
 *   vt  : [B, H*head_dim, Sk] contiguous -- the value projection TRANSPOSED (compute it as W_v x^T)
 *   out : [B, Sq, >= H*head_dim] row stride ldo
 *   Sk_valid : keys in [Sk_valid, Sk) are padding and get zero weight (cross-attention: 77 context tokens padded to 128)
 * Any Sq; Sk % 8 == 0; strides % 8 == 0; else GSW_ERR_UNSUPPORTED (sequences off the 128-query / 64-key tiles run a variant with clamped
 * loads and masked keys).  A scale that is not finite and > 0 returns GSW_ERR_BAD_ARG. */
int gsw_attention(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev, int B, int H, int head_dim, int Sq, int Sk,
                  int Sk_valid, int ldq, int ldk, int ldo, float scale, int dtype, void* stream);
/* The same with a caller-owned scratch buffer (16-byte aligned device memory, free again when the launch's stream has run it): few query tiles against many
 * key tiles -- one image's self-attention at 64 x 64 is 160 workgroups for 256 CUs, each walking 64 key tiles -- are then run as up to 8 workgroups per query
 * tile (at most 256 query tiles, at least 2048 keys), each over its own range of keys, and a second small kernel merges their partial results (deterministic).  4 MiB per 100 query tiles x splits is
 * enough (bytes = query tiles x splits x 4 x (16 ceil(head_dim / 32) + 2) x 256); a smaller buffer, or none, runs the unsplit kernel.  The split-K scratch of
 * GswMmExtras may be shared: both are free between launches of one stream. */
int gsw_attention_ws(const void* q_dev, const void* k_dev, const void* vt_dev, void* out_dev, int B, int H, int head_dim, int Sq, int Sk,
                     int Sk_valid, int ldq, int ldk, int ldo, float scale, int dtype, void* workspace_dev, int64_t workspace_bytes, void* stream);
/* The whole cross-attention sublayer of a transformer block as ONE launch (csrc/gswm_xattn.hip) -- diffusers' BasicTransformerBlock.attn2 with norm2 in front
 * and the residual behind, which extract.py:66-69 / the generation loop run at every latent level:
 *     out = x + to_out(softmax(to_q(LayerNorm(x)) K^T / sqrt(d)) V) + b_out,        K, V = to_k(ctx), to_v(ctx)
 * The context side is precomputed by the host ONCE per (context, layer) as a stream of MFMA fragments (xattn.py: context_operands; per head 112 640 bytes:
 * A' = K_h Wq_h diag(gamma) scale log2(e), rows centred, and B = Wo_h V_h^T (+ b_out as key slot 79 of the last head) in consumption order) plus 96 floats v per head
 * (the LayerNorm fold's constant term; -inf for padding keys).  x [x_images * tokens, 320] is the RAW residual stream, ln_stat float2 per row (rstd, -rstd mean:
 * gsw_ln_rowstats_finish); output image i reads x image i % x_images (classifier-free guidance: one x, two contexts) and context ctx_index[i] (NULL: context 0).
 * out_stat (nullable): (rstd, -rstd mean) of the OUTPUT rows with out_eps, what the next LayerNorm's fold reads.  C == 320, tokens % 128 == 0, <= 79 keys, else
 * GSW_ERR_UNSUPPORTED. */
int gsw_xattn_fused(const void* x_dev, const float* ln_stat_dev, const void* blob_dev, int64_t blob_stride_bytes, const float* v_dev, int64_t v_stride_floats,
                    const int32_t* ctx_index_dev, void* out_dev, float* out_stat_dev, float out_eps, int x_images, int out_images, int tokens, int C, int heads,
                    int dtype, void* stream);
/* The same launch, starting one operation earlier in the block: it first MAKES x from the self-attention in front of the sublayer (BasicTransformerBlock.attn1's
 * output projection, bias and residual) -- x = resid + o Wo^T + b with o [x_images * tokens, 320] that attention's output and w_frag Wo and b as 21 chunks of
 * MFMA fragments (xattn.py: pack_out_projection) -- rounds it to the storage dtype as the separate launch would, takes norm2's statistics (epsilon ln_eps) from
 * the rounded rows, and continues as gsw_xattn_fused.  x is never written: the projection's own launch, its 2 x rows x 640 bytes of traffic and
 * gsw_ln_rowstats_finish all disappear.  Same shape limits. */
int gsw_xattn_fused_pre(const void* resid_dev, const void* o_dev, const void* w_frag_dev, float ln_eps, const void* blob_dev, int64_t blob_stride_bytes,
                        const float* v_dev, int64_t v_stride_floats, const int32_t* ctx_index_dev, void* out_dev, float* out_stat_dev, float out_eps, int x_images,
                        int out_images, int tokens, int C, int heads, int dtype, void* stream);

/* GroupNorm + proj_in of a transformer (diffusers' Transformer2DModel.forward: `self.norm(hidden_states)`, NHWC flatten, `self.proj_in`; behind extract.py:66-69) at the
 * 320-channel level as ONE launch: tokens[b, y W + x, :] = GroupNorm(x)[b, y, x, :] Wp^T + b, x a padded-flat NHWC tensor (gsw_conv_pf's layout), the rows normalised in
 * registers on their way into the matrix pipe -- the normalised tensor is never stored.  pairsum: per-image, per-column-PAIR (sum, sum of squares) of x's interior,
 * [B][C / 2][2] floats, from the producing launch's column records (gsw_gn_colstats_pairs: the first half of gsw_groupnorm_pf_cs on its own).  w_frag: Wp and b as 21
 * chunks of MFMA fragments (xattn.py: pack_out_projection).  out_stat (nullable): (rstd, -rstd mean) of the output rows with out_eps, for the LayerNorm that follows.
 * C == 320, W % 32 == 0, H W % 128 == 0, an even number of channels per group, else GSW_ERR_UNSUPPORTED. */
int gsw_gn_colstats_pairs(const float* cs_dev, int cs_rows, int cs_npar, int cs_blocks, float* pairsum_dev, int B, int H, int W, int C, void* stream);
int gsw_gn_proj_tokens(const void* x_pf_dev, const float* pairsum_dev, const void* gamma_dev, const void* beta_dev, float gn_eps, int groups, const void* w_frag_dev,
                       void* out_dev, float* out_stat_dev, float out_eps, int B, int H, int W, int C, int dtype, void* stream);

/* E4, bit-parity mode -- gs_insert.py:62 `np.random.uniform(0, 1)` / nodes.py:52-53,114-117 `RandomState(seed).uniform(0, 1)`:
 * NumPy's legacy MT19937 `random_sample` stream continued on the device.  key/pos: the generator state as
 * np.random.get_state()[1:3] gives it (pos == 624: block exhausted).  Writes n float64 uniforms to u_dev and, when
 * state_out_dev != NULL, the advanced state ([624] key words + [1] pos) so that the host generator can be moved past the draws.
 * gsw_mt19937_seed: NumPy's legacy integer seeding (init_genrand); use pos = 624 with it. */
void gsw_mt19937_seed(uint32_t seed, uint32_t key[624]);
int gsw_mt19937_uniform(const uint32_t key[624], int pos, double* u_dev, int64_t n, uint32_t* state_out_dev, void* stream);

/* =====================================================================================================================
 * Image-side stages either side of the latent loops.  Images are uint8 [B, H, W, 3]
 * (what np.asarray(PIL image) gives); every function restates, bit for bit, what Pillow / libjpeg compute for the call the
 * reference makes.
 * ===================================================================================================================== */
typedef enum gsw_image_mode {
    GSW_IMG_U8_HWC = 0,  /* uint8 [B, H, W, 3]: a PIL image                                                           */
    GSW_IMG_F16_CHW = 1, /* fp16 [B, 3, H, W] = fp16(2 * fp16(v / 255) - 1): extract.py:37,48,40 (ToTensor -> .to(float16)
                            -> img_to_latents' 2.*x - 1.), i.e. exactly what the VAE encoder is fed                     */
    GSW_IMG_F32_CHW = 2  /* fp32 [B, 3, H, W] = v / 255: torchvision ToTensor (extract.py:37)                          */
} gsw_image_mode;

/* extract.py:35-36 / distortions:229-230 `pil_img.resize(size, Image.Resampling.LANCZOS)`: Pillow's Resample.c
 * precompute_coeffs + normalize_coeffs_8bpc (double precision, host libm) for one axis.  Fills bounds[out_size*2] (first source
 * index, count) and kk[out_size*ksize] (22-bit fixed point); returns ksize > 0, or -gsw_status.  bounds == kk == NULL: returns
 * ksize only.  Pure host function (a "plan": upload both arrays once per (in_size, out_size)). */
int gsw_lanczos_plan(int in_size, int out_size, int32_t* bounds, int32_t* kk, int kk_capacity);

/* The two resampling passes of ImagingResample on device (horizontal first, uint8 in between; a pass whose size is unchanged is
 * skipped like Pillow does), with the conversion to `out_mode` fused into the last pass.  tmp_dev: [B, Hin, Wout, 3] uint8 scratch,
 * needed when a horizontal pass is followed by anything (may be NULL otherwise).  *_dev plan arrays: gsw_lanczos_plan output for
 * (Win -> Wout) and (Hin -> Hout); NULL for a skipped pass. */
int gsw_resize_lanczos(const uint8_t* in_dev, int B, int Hin, int Win, void* out_dev, int Hout, int Wout, int out_mode, uint8_t* tmp_dev,
                       const int32_t* hbounds_dev, const int32_t* hkk_dev, int hksize, const int32_t* vbounds_dev, const int32_t* vkk_dev,
                       int vksize, void* stream);

/* `decode_image` tail + diffusers numpy_to_pil (modified_stable_diffusion_gs.pyc src :207-220): [B, 3, H, W] float tensor ->
 * uint8 [B, H, W, 3] = (x * 255).round(); denormalise != 0 first applies (x / 2 + 0.5).clamp(0, 1) in the tensor's dtype. */
int gsw_tensor_to_image(const void* in_dev, int dtype, int B, int H, int W, int denormalise, uint8_t* out_dev, void* stream);

/* distortions:175-184 "compression": `image.save(buf, format="JPEG", quality=q)` then `Image.open(buf)`, minus the (lossless)
 * entropy coding: RGB -> YCbCr 4:2:0, islow FDCT, IJG quality-scaled tables (force_baseline), dequantise, islow IDCT, fancy h2v2
 * upsampling, YCbCr -> RGB.  workspace_dev: gsw_jpeg_workspace_bytes(B, H, W) bytes. */
int gsw_jpeg_quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]);
size_t gsw_jpeg_workspace_bytes(int B, int H, int W);
int gsw_jpeg_roundtrip(const uint8_t* rgb_dev, int B, int H, int W, int quality, void* out_dev, int out_mode, uint8_t* workspace_dev,
                       void* stream);

/* distortions:157-164 "blurring": `image.filter(ImageFilter.GaussianBlur(radius))` = Pillow's three extended-box passes per axis
 * (BoxBlur.c), bit-exact.  tmp_dev: uint8 scratch of the image batch's size.  gsw_gaussian_blur_params exposes the integer box
 * radius and the two 8.24 weights Pillow derives from `radius` (pure host). */
int gsw_gaussian_blur_params(float radius, int passes, int* box_radius, uint32_t* ww, uint32_t* fw);
int gsw_gaussian_blur(const uint8_t* rgb_dev, int B, int H, int W, float radius, uint8_t* out_dev, uint8_t* tmp_dev, void* stream);

/* Point-wise attacks of distortions:131-224. */
typedef enum gsw_pointwise_op {
    GSW_PW_BRIGHTNESS = 0, /* ImageEnhance.Brightness(image).enhance(strength)  (distortions:131-139)                  */
    GSW_PW_CONTRAST = 1,   /* ImageEnhance.Contrast(image).enhance(strength)    (distortions:141-148); workspace: [B] uint64 */
    GSW_PW_INVERT = 2,     /* F.invert                                          (distortions:222-223)                  */
    GSW_PW_GRAY = 3,       /* F.rgb_to_grayscale, replicated to 3 channels      (distortions:201-202)                  */
    GSW_PW_HFLIP = 4,      /* F.hflip                                           (distortions:203-204)                  */
    GSW_PW_VFLIP = 5,      /* F.vflip                                           (distortions:205-206)                  */
    GSW_PW_NOISE = 6       /* (x + strength * N(0,1)).clamp(0,1); Philox keyed by (seed; pixel, image_index0 + b) -- the
                              reference draws torch.randn on the host (distortions:166-173): statistical parity only      */
} gsw_pointwise_op;
int gsw_image_pointwise(const uint8_t* rgb_dev, int B, int H, int W, int op, float strength, uint64_t seed, uint64_t image_index0,
                        void* out_dev, int out_mode, uint64_t* workspace_dev, void* stream);

/* Geometric attacks of distortions:107-137,207-222 (rotation, resizedcrop, erasing, randomcrop).  One launch per batch (two for the
 * crop and resize); the per-image tables are device arrays, so nothing here synchronises with the host. */

/* Pillow's resampling filters, numbered as PIL.Image.Resampling numbers them. */
typedef enum gsw_resample_filter {
    GSW_RESAMPLE_LANCZOS = 1,
    GSW_RESAMPLE_BILINEAR = 2
} gsw_resample_filter;

/* gsw_lanczos_plan for any filter of gsw_resample_filter (Resample.c precompute_coeffs + normalize_coeffs_8bpc); for LANCZOS the
 * same arrays as gsw_lanczos_plan.  Pure host function. */
int gsw_resample_plan(int filter, int in_size, int out_size, int32_t* bounds, int32_t* kk, int kk_capacity);

/* distortions:107-113 "rotation": `img.rotate(angle, NEAREST, expand=False, fillcolor=0)` = Geometry.c affine_fixed.
 * coeffs_dev: int32 [B, 6] = (a0, a1, a2, a3, a4, a5) in 16.16 fixed point per image; output pixel (x, y) reads source
 * ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16) in wrapping 32-bit arithmetic, black outside the image.  The transpose fast
 * paths (0, 90, 180, 270 degrees) are integer coefficient rows too.  out_dev must not alias in_dev. */
int gsw_affine_nearest(const uint8_t* in_dev, int B, int H, int W, const int32_t* coeffs_dev, void* out_dev, int out_mode, void* stream);

/* distortions:126-137 "erasing" (keep_inside = 0: the rectangle becomes 0) and :207-222 "randomcrop" (keep_inside != 0: the rectangle
 * is kept, everything else becomes 0).  boxes_dev: int32 [B, 4] = (top, left, height, width) per image, inside the image (the
 * caller checks; an empty box is allowed). */
int gsw_box_mask(const uint8_t* in_dev, int B, int H, int W, const int32_t* boxes_dev, int keep_inside, void* out_dev, int out_mode, void* stream);

/* distortions:115-124 "resizedcrop": `img.crop((left, top, left + crop_w, top + crop_h)).resize((Wout, Hout), filter)` per image, a
 * shared crop size and per-image origins_dev int32 [B, 2] = (top, left) inside the image (the caller checks).  Pillow's two passes,
 * horizontal first, uint8 in between, a pass skipped when its size is kept.  tmp_dev: [B, crop_h, Wout, 3] uint8 scratch.  Plans:
 * gsw_resample_plan for (crop_w -> Wout) and (crop_h -> Hout); NULL for a skipped pass. */
int gsw_crop_resize(const uint8_t* in_dev, int B, int H, int W, const int32_t* origins_dev, int crop_h, int crop_w, void* out_dev, int Hout,
                    int Wout, int out_mode, uint8_t* tmp_dev, const int32_t* hbounds_dev, const int32_t* hkk_dev, int hksize,
                    const int32_t* vbounds_dev, const int32_t* vkk_dev, int vksize, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Tracing: which registered message does an extracted watermark belong to (additive entry points: nothing above changes and
 * gsw_version() stays 500).
 *
 *   counts_dev   : uint32 [B, msg_bits], the counts output of gsw_extract ('1' votes per bit); copies = votes per bit
 *                  (padded lattice bits / msg_bits, one number per call since gsw_extract refuses ragged lattices)
 *   registry_dev : uint8 [n_users, msg_bits / 8], one issued message per row, packed as the codec packs messages
 *                  (bit t -> byte t >> 3, bit 7 - (t & 7))
 *   weights      : GSW_TRACE_SOFT  w = 2 c - copies (the vote margin);  GSW_TRACE_HARD  w = +1 if c > copies / 2 else -1 (the
 *                  reference's strict majority, ties -> 0), in which case score = 2 agree - msg_bits
 *   score[b, u]  = sum_t (2 r[u, t] - 1) w[b, t], an exact int32
 *   idx_dev / score_dev : int32 [B, k], the k best users per image by score, descending, ties towards the lower index; past
 *                  n_users (n_users < k): idx = -1, score = INT32_MIN
 *   workspace_dev: gsw_trace_workspace_bytes(B, n_users, k) bytes owned by the caller (partial lists; no state is kept between calls
 *                  and the result does not depend on the launch geometry)
 *
 * The scores go through the int8 matrix pipe with the registry bits expanded in registers; the [B, n_users] score matrix is never
 * written and the registry is read packed, once per tile of up to 64 images (fewer when copies > 127 or msg_bits > 1024).  Exact for
 * every copies up to 2 000 000 (int8 planes in base 128).  Registries of 2^19 rows and more are searched twice inside the call (a
 * leading sample first, whose k-th best score bounds the full search from below); the answer is the same.
 * GSW_ERR_BAD_ARG: null pointer, B < 1, msg_bits outside 8..2048 or not a multiple of 8, copies < 1, k outside 1..8, n_users outside
 * 1..2^31-1, unknown mode.  GSW_ERR_UNSUPPORTED: msg_bits * copies >= 2^31, soft mode with copies > 2 000 000, B > 1 048 560.
 * gsw_trace_workspace_bytes returns 0 for arguments gsw_trace_topk refuses. */
#define GSW_TRACE_SOFT 0
#define GSW_TRACE_HARD 1
size_t gsw_trace_workspace_bytes(int B, int64_t n_users, int k);
int gsw_trace_topk(const uint32_t* counts_dev, int B, int msg_bits, int copies, int mode, const uint8_t* registry_dev, int64_t n_users, int k,
                   int32_t* idx_dev, int32_t* score_dev, void* workspace_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Tracing against a registry whose records carry their own ChaCha20 key and nonce (what gs_insert logs when key and nonce are
 * left blank).  Additive: gsw_version() stays 500.
 *
 * X3 alone: y = int(norm.cdf(float64(z)) * 2) per element, packed MSB first (bit i -> byte i >> 3, bit 7 - (i & 7)); the quantiser and the
 * flags are gsw_extract's own (same thresholds, same GSW_FLAG_*; a saturated element packs as 1, a NaN as 0).  signs_dev [B, n_elems / 8].
 * n_elems % 8 != 0 (or n_elems > 0x7FFFFFF0) -> GSW_ERR_UNSUPPORTED; null pointer, unknown dtype, B < 0, n_elems < 1 -> GSW_ERR_BAD_ARG. */
int gsw_sign_pack(const void* z_dev, int z_dtype, uint8_t* signs_dev, uint32_t* flags_dev, int B, int64_t n_elems, void* stream);

/* records_dev: uint8 [n_records, record_stride], 16-byte aligned; a row is key[32] | nonce16[16] | msg[msg_bytes]; record_stride >= 48 + msg_bytes, % 16 == 0.
 * codeword of a record = the cipher bits gsw_embed plants for it over n_bits lattice bits (keystream of its key and nonce16, initial counter
 *                        and carry as gsw_keystream, XOR its message repeated), generated in registers: no codeword is ever stored.
 * score = n_bits - 2 popcount(signs[b] ^ codeword[u]), an exact int32; for records that share one key and nonce it is gsw_trace_topk's
 *         GSW_TRACE_SOFT score of the same messages on gsw_extract's counts.
 * out: the k best records per image by (score descending, index ascending), idx = -1 / score = INT32_MIN past the end -- gsw_trace_topk's
 *      conventions; workspace_dev: gsw_trace_keyed_workspace_bytes(B, n_records, k) bytes owned by the caller; the result does not depend on
 *      the launch geometry.
 * GSW_ERR_BAD_ARG: null pointer, B < 1, k outside 1..8, msg_bytes outside 1..256, n_bits < 1, n_records outside 1..2^31-1, a bad stride or
 * alignment of records_dev.  GSW_ERR_RAGGED: n_bits is not a multiple of 8 msg_bytes (the reference's vote raises IndexError there).
 * GSW_ERR_UNSUPPORTED: n_bits > 1 048 576 (one image's sign row is staged in 128 KiB of LDS), B > 65535.
 * gsw_trace_keyed_workspace_bytes returns 0 for B, n_records, k that gsw_trace_keyed_topk refuses. */
size_t gsw_trace_keyed_workspace_bytes(int B, int64_t n_records, int k);
int gsw_trace_keyed_topk(const uint8_t* signs_dev, int B, int64_t n_bits, const uint8_t* records_dev, int64_t record_stride, int msg_bytes,
                         int64_t n_records, int k, int32_t* idx_dev, int32_t* score_dev, void* workspace_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Multi-bit windows: extract.py's --l ("the size of slide windows for m"; gs_insert.py:52-53 "can be a value other than 1").  The
 * reference's own l > 1 path does not run (gs_insert.py:23,58-66 fills 1/l of the lattice; extract.py:84-86 parses decimal digits as
 * base 2), so the semantics are this library's ("Multi-bit windows").  Additive: gsw_version() stays 500.
 *
 *   l       : 1, 2 or 4 (windows that never straddle a byte).  l == 1 IS the entry point without _l, argument for argument.  Any other
 *             l, and for l > 1 a lattice with (n_elems * l) % 8 != 0 or n_elems * l > 0x7FFFFFF0: GSW_ERR_UNSUPPORTED.
 *   Nb      = n_elems * l cipher bits per image = the keystream of gsw_keystream XOR the message repeated floor(Nb / (8 msg_bytes)) times
 *             then zeros, MSB-first within each byte; element i takes bits [i l, i l + l), the first one is the MSB of y_i
 *   embed   : z_i = ndtri((u_i + y_i) / 2^l), one u per element (u_dev, or the Philox stream of gsw_embed, same addressing); the stored
 *             value is the representable value of out_dtype nearest to z_i that still quantises to y_i (bin-safe rounding), so a noiseless
 *             gsw_extract_l returns every count as 0 or copies in every dtype.  u = 0, y = 0 gives -inf.  GSW_EMBED_FAST_F32: |dz| <= 1e-5,
 *             same y; arguments below the fp32 core's domain take the exact core.
 *   quantise: y = int(norm.cdf(float64(z)) * 2^l), exactly, for fp16 / bf16 / fp32 / fp64 inputs (2^l - 1 thresholds, csrc/quant_thresholds.inc);
 *             z >= 8.292361075813597 packs as all ones and sets GSW_FLAG_SATURATED, NaN packs as zeros and sets GSW_FLAG_NAN
 *   extract : the y of an image written as l bits each, XOR keystream, strict-majority vote in msg_bits-wide segments (ties -> 0);
 *             counts are exact '1' votes out of copies = Nb / msg_bits; GSW_ERR_RAGGED when that is not whole.  GSW_ERR_UNSUPPORTED when
 *             keystream + decrypted bits + vote (about Nb / 4 bytes) exceed the LDS of a CU.
 *   gsw_quant_pack: the l-bit gsw_sign_pack: packed_dev [B, Nb / 8], the operand of gsw_trace_keyed_topk with n_bits = Nb.
 * Pointers, dtypes, B and stream as in the l = 1 entry points; the same GSW_ERR_BAD_ARG conditions. */
int gsw_embed_l(const uint8_t key[32], const uint8_t nonce16[16], const uint8_t* msg, int msg_bytes, const double* u_dev, uint64_t seed,
                uint64_t image_index0, void* out_dev, int out_dtype, int B, int64_t n_elems, uint32_t flags, int l, void* stream);
int gsw_extract_l(const void* z_dev, int z_dtype, const uint8_t key[32], const uint8_t nonce16[16], int msg_bits, uint8_t* bits_dev,
                  uint32_t* counts_dev, uint32_t* flags_dev, int B, int64_t n_elems, int l, void* stream);
int gsw_quant_pack(const void* z_dev, int z_dtype, uint8_t* packed_dev, uint32_t* flags_dev, int B, int64_t n_elems, int l, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Localising edits: where an image still agrees with a codeword, and a vote weighted by tile.
 * Additive: gsw_version() stays 500.
 *
 *   packed_dev : [B, Nb / 8], the rows gsw_sign_pack / gsw_quant_pack write for the [C, h, w] lattice, Nb = C h w l; element i = (c, y, x)
 *                in C order owns bits [i l, i l + l), MSB first; 4-byte aligned
 *   keys_dev   : [B, 48], key[32] | nonce16[16] PER IMAGE (4-byte aligned); the keystream is gsw_keystream's (initial counter, carry), generated
 *                in registers: no keystream and no codeword is stored
 *   tile       : T in {8, 16, 32}; tile (ty, tx) holds the elements of ALL C channels with y / T == ty and x / T == tx: n_t = C T T l bits
 *   gsw_tile_agree : agree[b, ty, tx] = number of bits j of the tile with q_j == cw_j, cw_j = ks_j ^ msg[b][j mod msg_bits] (the cipher bits
 *                gsw_embed[_l] plants for that message); msg_dev [B, msg_bits / 8], MSB first.  For a tile whose content is independent of the key
 *                and a message fixed independently of the image, agree ~ Bin(n_t, 1/2) exactly.
 *   gsw_vote_tiled : with p_j = q_j ^ ks_j and uint16 weights [B, h / T, w / T],
 *                score[b, t] = sum over j = t (mod msg_bits) of wgt[tile(j / l)] (2 p_j - 1),  wsum[b, t] = the same sum of wgt alone,
 *                bits MSB first with bit t = (score > 0): a tie or no weight at all gives 0, gsw_extract's tie rule.  With every weight 1,
 *                score = 2 counts - copies of gsw_extract[_l] and the bits are its bits.
 * Every output element is written; the results are exact integers and do not depend on the launch geometry.
 * GSW_ERR_BAD_ARG: null pointer, misaligned packed_dev / keys_dev / weights_dev, B < 1, non-positive C, h, w or msg_bits, l outside {1, 2, 4}.
 * GSW_ERR_UNSUPPORTED: tile outside {8, 16, 32}, h or w not a multiple of tile, msg_bits % 8 != 0, Nb > 1 048 576 (one image's row is staged in
 * 128 KiB of LDS); gsw_vote_tiled also when (Nb / msg_bits) * 65535 does not fit int32.  GSW_ERR_RAGGED: Nb % msg_bits != 0. */
int gsw_tile_agree(const uint8_t* packed_dev, int B, int C, int h, int w, int l, int tile, const uint8_t* keys_dev, const uint8_t* msg_dev,
                   int msg_bits, int32_t* agree_dev, void* stream);
int gsw_vote_tiled(const uint8_t* packed_dev, int B, int C, int h, int w, int l, int tile, const uint8_t* keys_dev, const uint16_t* weights_dev,
                   int msg_bits, uint8_t* bits_dev, int32_t* score_dev, int32_t* wsum_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Per-image records: embed and verify a batch in which every image has its own key, nonce and message.
 * Additive: gsw_version() stays 500.
 *
 *   records_dev : uint8 [B, record_stride], 16-byte aligned, gsw_trace_keyed_topk's rows: key[32] | nonce16[16] | msg[msg_bytes], with
 *                 record_stride >= 48 + msg_bytes and record_stride % 16 == 0; row b belongs to image b.  msg_bytes is 1..256.
 *   gsw_embed_keyed   : row b of out_dev is bit for bit what gsw_embed (l == 1) or gsw_embed_l (l == 2, 4) writes when called with record
 *                 b's key, nonce16 and message, B = 1, image_index0 + b, row b of u_dev (or NULL: Philox, addressed by that global image
 *                 index) and the same seed, flags (GSW_EMBED_*) and out_dtype.  n_elems % 4 == 0; for l > 1 the rule of gsw_embed_l.
 *   gsw_extract_keyed : bits_dev [B, msg_bytes], counts_dev [B, 8 msg_bytes] (NULL ok) and flags_dev [B] of row b are exactly those of
 *                 gsw_extract / gsw_extract_l for that image under record b's key and nonce16 with msg_bits = 8 msg_bytes;
 *                 matches_dev [B] (NULL ok) = how many of those recovered bits equal record b's message.
 *                 (That includes the votes of a NaN element in an image flagged GSW_FLAG_NAN: as gsw_extract[_l] counts them for the same geometry.)
 * One launch each; the keystreams are generated inside it and never stored.  Every output element is written, no atomics, no workspace;
 * the results do not depend on the launch geometry.
 * GSW_ERR_BAD_ARG: null pointer (u_dev, counts_dev, matches_dev excepted), B < 1, msg_bytes outside 1..256, a bad stride or alignment of
 * records_dev, out_dev / u_dev / z_dev not 16-byte aligned, unknown dtype, n_elems < 1 (embed: n_elems % 4 != 0).
 * GSW_ERR_UNSUPPORTED: l outside {1, 2, 4}; embed: as gsw_embed_l; extract: Nb = n_elems * l not a multiple of 8 or above 1 048 576 (one
 * image's row is staged in 128 KiB of LDS).  GSW_ERR_RAGGED (extract): Nb % (8 msg_bytes) != 0. */
int gsw_embed_keyed(const uint8_t* records_dev, int64_t record_stride, int msg_bytes, const double* u_dev, uint64_t seed,
                    uint64_t image_index0, void* out_dev, int out_dtype, int B, int64_t n_elems, uint32_t flags, int l, void* stream);
int gsw_extract_keyed(const void* z_dev, int z_dtype, const uint8_t* records_dev, int64_t record_stride, int msg_bytes,
                      uint8_t* bits_dev, uint32_t* counts_dev /* NULL ok */, uint32_t* flags_dev, uint32_t* matches_dev /* NULL ok */,
                      int B, int64_t n_elems, int l, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Soft-decision vote: every lattice element votes with an integer reliability level taken from its magnitude.
 * Additive: gsw_version() stays 500.
 *
 *   records_dev : gsw_extract_keyed's rows, uint8 [B, record_stride], 16-byte aligned: key[32] | nonce16[16] | msg[msg_bytes]; the keystream of
 *                 image b is record b's (gsw_keystream's counter and carry), generated inside the launch and never stored.  M = 8 msg_bytes,
 *                 one cipher bit per element (l = 1).
 *   thr_dev     : float [B, thr_stride] (thr_stride >= levels, in floats) or, with thr_stride == 0, one row of `levels` floats for all images;
 *                 levels is 1..15.
 *   p_j         = q_j ^ ks_j, q_j the quantiser of gsw_extract.
 *   level_j     = #{ i < levels : |z_j| >= thr[b][i] }.  fp16, bf16 and fp32 inputs are widened exactly to fp32 and compared there, fp64
 *                 inputs are compared in fp64 against the thresholds widened to fp64: an exact function of the stored bits in every dtype.
 *                 NaN gives level 0, +-inf gives `levels` (finite thresholds), -0.0 counts as 0.0.
 *   score_dev   : int32 [B, M] (NULL ok), score[b, t] = sum over j = t (mod M) of level_j (2 p_j - 1)
 *   wsum_dev    : int32 [B, M] (NULL ok), the same sum of level_j alone
 *   wsq_dev     : int32 [B] (NULL ok), sum over the image of level_j^2
 *   bits_dev    : uint8 [B, msg_bytes], MSB first, bit t = (score > 0): a tie or no weight at all gives 0, gsw_extract's tie rule
 *   matches_dev : uint32 [B] (NULL ok), how many recovered bits equal record b's message, as gsw_extract_keyed
 *   flags_dev   : uint32 [B], gsw_extract's GSW_FLAG_*; a flagged element still votes with its level, a NaN with level 0
 * With levels = 1 and thr = {0} every non-NaN element has level 1: on NaN-free images score = 2 counts - copies of gsw_extract_keyed and
 * the bits are its bits.
 * One launch.  Every output element is written, no atomics, no workspace, nothing to zero first; the results are exact integers and do
 * not depend on the launch geometry.
 * GSW_ERR_BAD_ARG: null pointer (score_dev, wsum_dev, wsq_dev, matches_dev excepted), B < 1, msg_bytes outside 1..256, a bad stride or
 * alignment of records_dev, z_dev not 16-byte aligned, thr_dev not 4-byte aligned, thr_stride neither 0 nor >= levels, levels outside
 * 1..15, unknown dtype, n_elems < 1.
 * GSW_ERR_UNSUPPORTED: n_elems % 8 != 0 or n_elems > 1 048 576 (one image's keystream is staged in 128 KiB of LDS).
 * GSW_ERR_RAGGED: n_elems % (8 msg_bytes) != 0. */
int gsw_extract_soft(const void* z_dev, int z_dtype, const uint8_t* records_dev, int64_t record_stride, int msg_bytes,
                     const float* thr_dev, int64_t thr_stride /* floats; 0: one table for all images */, int levels,
                     uint8_t* bits_dev, int32_t* score_dev /* NULL ok */, int32_t* wsum_dev /* NULL ok */, int32_t* wsq_dev /* NULL ok */,
                     uint32_t* flags_dev, uint32_t* matches_dev /* NULL ok */, int B, int64_t n_elems, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Keyed registry search ranked by reliability-weighted margins: gsw_trace_keyed_topk with every lattice
 * element weighted by gsw_extract_soft's level.  One cipher bit per element (l = 1).  Additive: gsw_version() stays 500.
 *
 * gsw_level_pack, one launch per batch: z_dev [B, n_elems] (16-byte aligned), thr_dev / thr_stride / levels as gsw_extract_soft;
 * P = bit length of levels (1 .. 4).
 *   signs_dev  : uint8 [B, n_elems / 8], bit for bit gsw_sign_pack's row
 *   planes_dev : uint8 [B, P, n_elems / 8], plane k = bit k of level_j (gsw_extract_soft's level, same widening rules), packed MSB first
 *   wsum_dev   : int32 [B], sum over the image of level_j          wsq_dev : int32 [B], sum of level_j^2
 *   flags_dev  : uint32 [B], as gsw_sign_pack
 * Every output element is written, no atomics, no workspace, nothing to zero first.
 * GSW_ERR_BAD_ARG: null pointer, B < 1, n_elems < 1, unknown dtype, z_dev not 16-byte aligned, thr_dev not 4-byte aligned, thr_stride neither
 * 0 nor >= levels, levels outside 1..15.  GSW_ERR_UNSUPPORTED: n_elems % 8 != 0 or n_elems > 1 048 576.
 *
 * gsw_trace_keyed_soft_topk: records_dev, record_stride, msg_bytes, n_records, k, idx_dev, score_dev and workspace_dev
 * (gsw_trace_keyed_workspace_bytes(B, n_records, k) bytes) as gsw_trace_keyed_topk; signs_dev, planes_dev, wsum_dev as gsw_level_pack
 * writes them for n_elems = n_bits and the same `levels`.
 *   score = sum_j level_j (1 - 2 (signs_j ^ codeword[u]_j)) = wsum[b] - 2 sum_{k < P} 2^k popcount(plane_k[b] & (signs[b] ^ codeword[u])),
 *           an exact int32; for records that share one key and nonce it is sum_t (2 r_t - 1) score[b, t] of gsw_extract_soft, r the
 *           record's message.  With levels = 1 and thr = {0} on NaN-free images it is gsw_trace_keyed_topk's score.
 *   out   : the k best records per image by (score descending, index ascending), idx = -1 / score = INT32_MIN past the end; the result
 *           does not depend on the launch geometry.
 * GSW_ERR_BAD_ARG: as gsw_trace_keyed_topk, plus levels outside 1..15 and wsum_dev not 4-byte aligned.  GSW_ERR_RAGGED: n_bits is not a
 * multiple of 8 msg_bytes.  GSW_ERR_UNSUPPORTED: n_bits * (1 + P) > 1 048 576 (the sign row and the P plane rows of an image are staged in
 * 128 KiB of LDS), B > 65535. */
int gsw_level_pack(const void* z_dev, int z_dtype, const float* thr_dev, int64_t thr_stride /* floats; 0: one table for all images */, int levels,
                   uint8_t* signs_dev, uint8_t* planes_dev, int32_t* wsum_dev, int32_t* wsq_dev, uint32_t* flags_dev, int B, int64_t n_elems,
                   void* stream);
int gsw_trace_keyed_soft_topk(const uint8_t* signs_dev, const uint8_t* planes_dev, const int32_t* wsum_dev, int levels, int B, int64_t n_bits,
                              const uint8_t* records_dev, int64_t record_stride, int msg_bytes, int64_t n_records, int k, int32_t* idx_dev,
                              int32_t* score_dev, void* workspace_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Soft-decision vote for multi-bit windows, l = 2 or 4: every CIPHER BIT of a lattice element votes with an
 * integer reliability level, its distance from the nearest quantiser boundary at which that bit would have come out differently.
 * Additive: gsw_version() stays 500.
 *
 *   Element e of image b holds z (Z = z widened exactly to fp64) and y = #{ j : z >= T_j }, gsw_extract_l's window (T_1 .. T_(2^l - 1)
 *   the quantiser's fp64 thresholds; NaN: 0 + GSW_FLAG_NAN, z >= the saturation point: all ones + GSW_FLAG_SATURATED).  Window bit w
 *   (0 = first = MSB of y, cipher position e l + w) has the value s = 2^(l-1-w) in y and flips exactly at the boundaries T_i with s | i.
 *   a = (y / s) s is the nearest flip boundary at or below z (none if a == 0), c = a + s the nearest above (none if c == 2^l).
 *   thr_dev     : float [B, thr_stride] (thr_stride >= l levels, in floats) or, with thr_stride == 0, one table for all images; a table is
 *                 [l][levels], row w for window bit w; levels is 1..15.  With t_i = (double)thr[b][w][i]:
 *   level(e, w) = #{ i < levels : (a == 0 or Z >= fl64(T_a + t_i)) and (c == 2^l or Z <= fl64(T_c - t_i)) }, sums and differences formed
 *                 in fp64 (round to nearest), compares in fp64: an exact function of the stored bits in every dtype.  NaN z gives level
 *                 0, a NaN threshold never counts, +-inf gives `levels` for finite thresholds; the order of a row does not matter.
 *   p           = (bit w of y) ^ keystream bit (e l + w) of record b (gsw_extract_keyed's rows and keystream), t = (e l + w) mod M, M = 8 msg_bytes
 *   score_dev   : int32 [B, M] (NULL ok), score[b, t] = sum of level (2 p - 1)         wsum_dev : int32 [B, M] (NULL ok), the same sum of level
 *   wsq_dev     : int32 [B] (NULL ok), sum of level^2 over all n_elems l bits
 *   bits_dev, matches_dev, flags_dev : as gsw_extract_soft (MSB first, bit t = (score > 0), a tie or no weight gives 0)
 * With levels = 1 and thr = 0 every bit of a non-NaN element has level 1: on NaN-free images score = 2 counts - copies of
 * gsw_extract_keyed at that l and the bits are its bits.
 *
 * gsw_level_pack_l: the same levels without a key, the operands of gsw_trace_keyed_soft_topk and gsw_key_search_soft_topk with
 * n_bits = Nb = n_elems l.  P = bit length of levels (1 .. 4).
 *   signs_dev  : uint8 [B, Nb / 8], bit for bit gsw_quant_pack's row
 *   planes_dev : uint8 [B, P, Nb / 8], bit e l + w of plane k = bit k of level(e, w), packed MSB first
 *   wsum_dev   : int32 [B], sum of the levels over the image's Nb bits          wsq_dev : int32 [B], sum of their squares
 *   flags_dev  : uint32 [B], as gsw_quant_pack
 * Both: one launch, one workgroup per image; every output element is written, no atomics, no workspace, nothing to zero first; the results
 * are exact integers and do not depend on the launch geometry.
 * GSW_ERR_BAD_ARG: l other than 2 or 4, null pointer (score_dev, wsum_dev, wsq_dev, matches_dev of gsw_extract_soft_l excepted), B < 1,
 * msg_bytes outside 1..256, a bad stride or alignment of records_dev, z_dev not 16-byte aligned, thr_dev not 4-byte aligned, thr_stride
 * neither 0 nor >= l levels, levels outside 1..15, unknown dtype, n_elems < 1.
 * GSW_ERR_UNSUPPORTED: n_elems % 8 != 0 or n_elems l > 1 048 576 (one image's keystream is staged in 128 KiB of LDS).
 * GSW_ERR_RAGGED (gsw_extract_soft_l): n_elems l % (8 msg_bytes) != 0. */
int gsw_extract_soft_l(const void* z_dev, int z_dtype, const uint8_t* records_dev, int64_t record_stride, int msg_bytes,
                       const float* thr_dev, int64_t thr_stride /* floats; 0: one table for all images */, int levels, int l,
                       uint8_t* bits_dev, int32_t* score_dev /* NULL ok */, int32_t* wsum_dev /* NULL ok */, int32_t* wsq_dev /* NULL ok */,
                       uint32_t* flags_dev, uint32_t* matches_dev /* NULL ok */, int B, int64_t n_elems, void* stream);
int gsw_level_pack_l(const void* z_dev, int z_dtype, const float* thr_dev, int64_t thr_stride /* floats; 0: one table for all images */, int levels,
                     int l, uint8_t* signs_dev, uint8_t* planes_dev, int32_t* wsum_dev, int32_t* wsq_dev, uint32_t* flags_dev, int B,
                     int64_t n_elems, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Blind key search: which keys of a keyring does an image carry a watermark under, whatever the message.
 * Additive: gsw_version() stays 500.
 *
 *   signs_dev : uint8 [B, n_bits / 8], the row gsw_sign_pack or gsw_quant_pack writes (any alignment)
 *   keys_dev  : uint8 [n_keys, key_stride], 16-byte aligned; a row is key[32] | nonce16[16], bytes past 48 are ignored (the record rows of
 *               gsw_trace_keyed_topk can be passed as they are); key_stride >= 48, % 16 == 0
 *   M = 8 msg_bytes message positions, V = n_bits / M copies of each
 *   d         = signs[b] ^ keystream(key_u, nonce16_u) over n_bits bits (initial counter and carry as gsw_keystream), generated inside the
 *               launch and never stored
 *   c_t       = #{ j < n_bits : j mod M == t, d_j = 1 }
 *   stat[b,u] = sum_t |2 c_t - V|, an exact int32: the score gsw_trace_keyed_topk gives the image's own majority-voted message under key u
 *               (a tie adds 0 whichever way it is broken), i.e. the maximum of that score over all 2^M messages.  For an image that is
 *               independent of the key the c_t are independent Bin(V, 1/2).
 *   out       : the k best keys per image by (stat descending, index ascending), idx = -1 / stat = INT32_MIN past the end of the keyring;
 *               workspace_dev: gsw_key_search_workspace_bytes(B, n_keys, k) bytes owned by the caller.  Every output element is written,
 *               no atomics; the result depends on neither the launch geometry nor the arrival order.
 * GSW_ERR_BAD_ARG: null pointer, B < 1, k outside 1..8, msg_bytes outside 1..256, n_bits < 1, n_keys outside 1..2^31-1, a bad stride or
 * alignment of keys_dev.  GSW_ERR_RAGGED: n_bits is not a multiple of 8 msg_bytes.  GSW_ERR_UNSUPPORTED: n_bits > 1 048 576, B > 65535.
 * Every refusal happens before any launch.  gsw_key_search_workspace_bytes returns 0 for B, n_keys, k that gsw_key_search_topk refuses. */
size_t gsw_key_search_workspace_bytes(int B, int64_t n_keys, int k);
int gsw_key_search_topk(const uint8_t* signs_dev, int B, int64_t n_bits, const uint8_t* keys_dev, int64_t key_stride, int msg_bytes, int64_t n_keys,
                        int k, int32_t* idx_dev, int32_t* stat_dev, void* workspace_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Alignment search: every candidate alignment of a packed quantised row, written in one launch; the rows are the
 * operand of gsw_key_search_topk (or any search over packed rows).  Additive: gsw_version() stays 500.
 *
 *   rows_dev   : uint8 [B, C H W l / 8], the row gsw_sign_pack (l = 1) or gsw_quant_pack writes (any alignment): element e = (c H + y) W + x
 *                owns bits [e l, e l + l), MSB first, byte j holds bits 8 j .. 8 j + 7
 *   aligns_dev : int32 [A, 3] rows (d, dy, dx), 4-byte aligned.  The alignment acts on the [H, W] planes of the lattice: mirror the last axis if
 *                d & 4, then d & 3 quarter turns counterclockwise (torch.rot90 over the last two axes), then a cyclic roll by (dy, dx) (any
 *                integers, taken modulo H and W)
 *   out_dev    : uint8 [B, A, C H W l / 8] (any alignment); row (b, a) is bit for bit what gsw_quant_pack writes for that transform of image
 *                b's latent: the l-bit groups are permuted, no value is touched, so the result does not depend on the latent's dtype
 * The list is device memory and is not read on the host: an entry with d outside 0..7, or an odd d when H != W, writes a row of zeros (the
 * callers of this package refuse such a list before it is uploaded).  Every output byte is written, no atomics, no workspace, integer
 * arithmetic only.  Rows of up to 65 536 bytes are staged in LDS once per workgroup, longer ones are read in place.
 * GSW_ERR_BAD_ARG: null pointer, aligns_dev not 4-byte aligned, B, C, H, W or A < 1, l outside {1, 2, 4}.  GSW_ERR_UNSUPPORTED: C H W l >
 * 1 048 576 bits, B > 65535.  GSW_ERR_RAGGED: C H W l is not a multiple of 8.  Every refusal happens before any launch. */
int gsw_rows_align(const uint8_t* rows_dev, int B, int C, int H, int W, int l, const int32_t* aligns_dev, int A, uint8_t* out_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Blind key search ranked by reliability levels: gsw_key_search_topk with every lattice element weighted by
 * gsw_level_pack's level.  One cipher bit per element (l = 1).  Additive: gsw_version() stays 500.
 *
 *   signs_dev  : uint8 [B, n_bits / 8], gsw_level_pack's sign row (any alignment)
 *   planes_dev : uint8 [B, P, n_bits / 8], gsw_level_pack's plane rows, plane k = bit k of the levels (any alignment); P in 1 .. 4,
 *                w_j = sum_k 2^k plane_k[j] in 0 .. 2^P - 1
 *   keys_dev   : as gsw_key_search_topk
 *   d          = signs[b] ^ keystream(key_u, nonce16_u), M = 8 msg_bytes, V = n_bits / M
 *   X_t        = sum_{j mod M == t} w_j (2 d_j - 1)
 *   stat[b,u]  = sum_t |X_t|, an exact int32 (at most 15 n_bits): sum_t |score[t]| of gsw_extract_soft under key u; with one plane of all
 *                ones it is gsw_key_search_topk's stat bit for bit
 *   out        : as gsw_key_search_topk; workspace_dev: gsw_key_search_soft_workspace_bytes(B, n_keys, k) bytes owned by the caller.  Every
 *                output element is written, no atomics; the result depends on neither the launch geometry nor the arrival order.
 * GSW_ERR_BAD_ARG: as gsw_key_search_topk, plus planes_dev null and P outside 1..4.  GSW_ERR_RAGGED: n_bits is not a multiple of 8 msg_bytes.
 * GSW_ERR_UNSUPPORTED: n_bits (1 + P) > 1 048 576 (gsw_trace_keyed_soft_topk's domain), B > 65535.  Every refusal happens before any launch.
 * gsw_key_search_soft_workspace_bytes returns 0 for B, n_keys, k that gsw_key_search_soft_topk refuses. */
size_t gsw_key_search_soft_workspace_bytes(int B, int64_t n_keys, int k);
int gsw_key_search_soft_topk(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int64_t n_bits, const uint8_t* keys_dev,
                             int64_t key_stride, int msg_bytes, int64_t n_keys, int k, int32_t* idx_dev, int32_t* stat_dev, void* workspace_dev,
                             void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Alignment search ranked by reliability levels: every candidate alignment of gsw_level_pack's sign row AND of its
 * P level planes, written in one launch; the outputs, viewed as [B A, ...], are the operands of gsw_key_search_soft_topk without a copy.
 * One cipher bit per element (l = 1).  Additive: gsw_version() stays 500.
 *
 *   signs_dev      : uint8 [B, n / 8], n = C H W, gsw_level_pack's sign row (any alignment)
 *   planes_dev     : uint8 [B, P, n / 8], gsw_level_pack's plane rows (any alignment); P in 1 .. 4
 *   aligns_dev     : int32 [A, 3] rows (d, dy, dx), 4-byte aligned, as gsw_rows_align
 *   out_signs_dev  : uint8 [B, A, n / 8] (any alignment)
 *   out_planes_dev : uint8 [B, A, P, n / 8] (any alignment)
 * Row (b, a) of out_signs and row (b, a, p) of out_planes are bit for bit what gsw_rows_align writes for that input row at l = 1: a
 * permutation of bits, so the levels travel with their elements and their sums do not change.  The source position of an element is computed
 * once for all 1 + P rows.  An entry with d outside 0..7, or an odd d when H != W, writes zeros to all its 1 + P rows (the callers of this
 * package refuse such a list before it is uploaded).  Every output byte is written, no atomics, no workspace, integer arithmetic only.  The
 * 1 + P rows of an image are staged in LDS once per workgroup while they total at most 65 536 bytes (each padded to 16), else read in place.
 * GSW_ERR_BAD_ARG: null pointer, aligns_dev not 4-byte aligned, P outside 1..4, B, C, H, W or A < 1.  GSW_ERR_UNSUPPORTED:
 * C H W (1 + P) > 1 048 576 bits (gsw_key_search_soft_topk's domain), B > 65535.  GSW_ERR_RAGGED: C H W is not a multiple of 8.  Every
 * refusal happens before any launch. */
int gsw_level_rows_align(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int C, int H, int W, const int32_t* aligns_dev, int A,
                         uint8_t* out_signs_dev, uint8_t* out_planes_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Aligned registry search under one key: the vote counts of every candidate alignment of a packed quantised row,
 * in one launch; viewed as [B A, msg_bits] they are the operand of gsw_trace_topk.  Additive: gsw_version() stays 500.
 *
 *   rows_dev    : uint8 [B, C H W l / 8], gsw_sign_pack's / gsw_quant_pack's row (any alignment), as gsw_rows_align
 *   aligns_dev  : int32 [A, 3] rows (d, dy, dx), 4-byte aligned, as gsw_rows_align
 *   key, nonce16: host bytes, as gsw_extract; the keystream is the first n_bits = C H W l bits of ChaCha20 under them
 *   counts_dev  : int32 [B, A, msg_bits], 4-byte aligned; with M = msg_bits
 *                 counts[b, a, t] = #{ p < n_bits : p mod M == t and (bit p of gsw_rows_align's row (b, a)) ^ (keystream bit p) == 1 }
 *                 bit for bit the counts gsw_extract / gsw_extract_l write for that transform of image b's latent, whatever its dtype
 * The aligned rows are never written.  An entry with d outside 0..7, or an odd d when H != W, writes a row of zero counts (the callers of
 * this package refuse such a list before it is uploaded).  Every output element is written, no atomics, no workspace, integer arithmetic
 * only.  The row and its keystream are both staged in LDS once per workgroup (64 KiB each at most); there is no read-in-place form.
 * GSW_ERR_BAD_ARG: null pointer, aligns_dev or counts_dev not 4-byte aligned, B, C, H, W or A < 1, l outside {1, 2, 4}, msg_bits outside
 * 8..2048 or not a multiple of 8.  GSW_ERR_RAGGED: n_bits is not a multiple of 8 or of msg_bits.  GSW_ERR_UNSUPPORTED: n_bits > 524 288,
 * B > 65535.  In that order; every refusal happens before any launch. */
int gsw_counts_align(const uint8_t* rows_dev, int B, int C, int H, int W, int l, const int32_t* aligns_dev, int A, const uint8_t key[32],
                     const uint8_t nonce16[16], int msg_bits, int32_t* counts_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Aligned registry search ranked by reliability levels: gsw_counts_align for gsw_level_pack's rows.  The
 * level-weighted vote of every candidate alignment under one key, in one launch; viewed as [B A, msg_bits] the scores are the operand of
 * gsw_trace_topk.  One cipher bit per element (l = 1).  Additive: gsw_version() stays 500.
 *
 *   signs_dev, planes_dev : gsw_level_pack's sign row uint8 [B, n / 8] and plane rows uint8 [B, P, n / 8], n = C H W (any alignment); P in 1 .. 4
 *   aligns_dev  : int32 [A, 3] rows (d, dy, dx), 4-byte aligned, as gsw_rows_align
 *   key, nonce16: host bytes, as gsw_extract; the keystream is the first n bits of ChaCha20 under them
 *   bias        : added to every score (a caller that feeds gsw_trace_topk passes levels * n / msg_bits: the scores are then its counts)
 *   score_dev   : int32 [B, A, msg_bits], 4-byte aligned;  wsum_dev : the same shape, or null (then it is not written).  With M = msg_bits,
 *                 d_p = (bit p of gsw_rows_align's row (b, a) of the sign row) ^ (keystream bit p), level_p = sum_k 2^k (bit p of the aligned plane k):
 *                 score[b, a, t] = bias + sum over p = t (mod M) of level_p (2 d_p - 1),  wsum[b, a, t] = sum over p = t (mod M) of level_p
 *                 bit for bit gsw_extract_soft's score (plus bias) and wsum of that transform of image b's latent under the table the rows were packed with
 * The aligned rows are never written.  An entry with d outside 0..7, or an odd d when H != W, writes `bias` to its scores and zeros to its wsum
 * (the callers of this package refuse such a list before it is uploaded).  Every element of a present output is written, no atomics, no
 * workspace, integer arithmetic only.  The 1 + P rows (each padded to 16 bytes), the keystream and a reduction region (64 KiB at most) are staged
 * in LDS; there is no read-in-place form.
 * GSW_ERR_BAD_ARG: null pointer (wsum_dev apart), aligns_dev, score_dev or wsum_dev not 4-byte aligned, B, C, H, W or A < 1, P outside 1..4,
 * msg_bits outside 8..2048 or not a multiple of 8.  GSW_ERR_RAGGED: n is not a multiple of 8 or of msg_bits.  GSW_ERR_UNSUPPORTED:
 * n (1 + P) > 1 048 576, B > 65535, the staged regions beyond 128 KiB (a 4 x 128 x 128 lattice at P = 4 takes 80 KiB, 4 x 256 x 256 at P = 1 the
 * whole of it), |bias| + 15 n / msg_bits beyond int32.  In that order; every refusal happens before any launch. */
int gsw_level_counts_align(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int C, int H, int W, const int32_t* aligns_dev, int A,
                           const uint8_t key[32], const uint8_t nonce16[16], int msg_bits, int bias, int32_t* score_dev, int32_t* wsum_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Reliability levels through the alignment searches at l = 2, 4: gsw_level_rows_align and gsw_level_counts_align
 * for gsw_level_pack_l's rows.  Element e of the [C, H, W] lattice owns bits [e l, e l + l), MSB first, of the quantised row and of every
 * level plane; an alignment moves the l-bit group of an element in all 1 + P rows after ONE computation of where the element comes from.
 * Additive: gsw_version() stays 500.
 *
 *   signs_dev, planes_dev : gsw_level_pack_l's row uint8 [B, n l / 8] and plane rows uint8 [B, P, n l / 8], n = C H W (any alignment); P in 1 .. 4
 *   l           : 1, 2 or 4.  At l = 1 both entry points write byte for byte what gsw_level_rows_align / gsw_level_counts_align write
 *   aligns_dev  : int32 [A, 3] rows (d, dy, dx), 4-byte aligned, as gsw_rows_align
 * gsw_level_rows_align_l: out_signs_dev uint8 [B, A, n l / 8], out_planes_dev uint8 [B, A, P, n l / 8] (any alignment); row (b, a) of each is
 * bit for bit gsw_rows_align's row at that l.  Viewed as [B A, ...] they are the operands of gsw_key_search_soft_topk and
 * gsw_trace_keyed_soft_topk with n_bits = n l.  Staged in LDS while the 1 + P padded rows total at most 65 536 bytes, else read in place.
 * GSW_ERR_BAD_ARG: null pointer, aligns_dev not 4-byte aligned, l outside {1, 2, 4}, P outside 1..4, B, C, H, W or A < 1.
 * GSW_ERR_UNSUPPORTED: n l (1 + P) > 1 048 576, B > 65535.  GSW_ERR_RAGGED: n l is not a multiple of 8.
 * gsw_level_counts_align_l: key, nonce16, bias, score_dev, wsum_dev as gsw_level_counts_align, over the n l cipher positions p:
 *                 score[b, a, t] = bias + sum over p = t (mod M) of level_p (2 d_p - 1),  wsum[b, a, t] = sum over p = t (mod M) of level_p
 *                 bit for bit gsw_extract_soft_l's score (plus bias) and wsum of that transform of image b's latent under the table the rows were packed with
 * GSW_ERR_BAD_ARG: as gsw_level_counts_align, and l outside {1, 2, 4}.  GSW_ERR_RAGGED: n l is not a multiple of 8 or of msg_bits.
 * GSW_ERR_UNSUPPORTED: n l (1 + P) > 1 048 576, B > 65535, the staged regions beyond 128 KiB, |bias| + 15 n l / msg_bits beyond int32.  In that
 * order.  An entry without a map (d outside 0..7, or an odd d when H != W) writes zero rows, or `bias` and zeros.  Every output byte is
 * written, no atomics, no workspace, integer arithmetic only; every refusal happens before any launch. */
int gsw_level_rows_align_l(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int l, int B, int C, int H, int W, const int32_t* aligns_dev, int A,
                           uint8_t* out_signs_dev, uint8_t* out_planes_dev, void* stream);
int gsw_level_counts_align_l(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int l, int B, int C, int H, int W, const int32_t* aligns_dev, int A,
                             const uint8_t key[32], const uint8_t nonce16[16], int msg_bits, int bias, int32_t* score_dev, int32_t* wsum_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Robust decode in one launch, tile weights times reliability levels: the rounds of the tile-weighted vote
 * (gsw_vote_tiled, gsw_tile_agree and the weight rule between them) with every cipher bit voting at its reliability level.
 * Additive: gsw_version() stays 500.
 *
 *   signs_dev  : [B, Nb / 8], gsw_quant_pack's / gsw_level_pack[_l]'s row for the [C, h, w] lattice at window l, Nb = C h w l; 4-byte aligned
 *   planes_dev : [B, P, Nb / 8], gsw_level_pack[_l]'s planes over the same Nb bits, plane k = bit k of the level; 4-byte aligned; P in 0 .. 4,
 *                with P = 0 the pointer is not read and every level is 1
 *   keys_dev   : [B, 48], key[32] | nonce16[16] PER IMAGE, 4-byte aligned, as gsw_vote_tiled
 *   iters      : I in 0 .. 8, the rounds after the first;  sign_rounds : W in {0, 1}, the rounds that vote at unit levels before the levels count
 * With p_j = q_j ^ ks_j, lev_j = sum_k 2^k plane_k[j], L_j = 1 in round r < W and lev_j after, wgt = 1 in round 0, for r = 0 .. I:
 *   score[t]    = sum over j = t (mod msg_bits) of L_j wgt[tile(j / l)] (2 p_j - 1),  wsum[t] = the same sum without the sign,
 *   bit_t       = score[t] > 0 (a tie or no weight at all gives 0),
 *   excess[tau] = sum over j in tile tau of L_j (1 - 2 (p_j ^ bit_(j mod msg_bits))),  wsq[tau] = sum over j in tau of L_j^2,
 *   wgt[tau]   <- max(0, excess[tau] - isqrt(wsq[tau])), isqrt the exact floor square root.
 * Outputs of round I: bits_dev uint8 [B, msg_bits / 8] MSB first, score_dev and wsum_dev int32 [B, msg_bits], excess_dev, wsq_dev and weights_dev
 * int32 [B, h / T, w / T]; weights is what the last vote used (ones when I = 0).  Every element of every output is written; the results are exact
 * integers and do not depend on the launch geometry.  One workgroup per image; nothing visits global memory between the rounds.
 * With P = 0, bits / score / wsum are those of I rounds of gsw_vote_tiled under max(0, 2 agree - n_t - isqrt(n_t)) and (excess + n_t) / 2 is
 * gsw_tile_agree's count against the returned bits; with I = 0, W = 0 they are gsw_extract_soft[_l]'s; with I = 0, W = 1 the plain vote's.
 * GSW_ERR_BAD_ARG: as gsw_vote_tiled, and P outside 0..4, iters outside 0..8, sign_rounds outside {0, 1}, planes_dev null or misaligned with P > 0.
 * GSW_ERR_UNSUPPORTED: as gsw_vote_tiled's lattice checks, and Nb (1 + P) > 1 048 576, (Nb / msg_bits) Lmax^2 n_t > INT32_MAX with
 * Lmax = max(1, 2^P - 1) and n_t = C T T l (a bit's vote is at most Lmax times a weight of at most Lmax n_t), or an LDS footprint
 * 64 ceil(Nb / 512) + P Nb / 8 + 4 tiles (1 or 3) + msg_bits / 8 above 131 072 bytes.  GSW_ERR_RAGGED: Nb % msg_bits != 0.  Every refusal
 * happens before any launch. */
int gsw_decode_robust(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int C, int h, int w, int l, int tile, const uint8_t* keys_dev,
                      int msg_bits, int iters, int sign_rounds, uint8_t* bits_dev, int32_t* score_dev, int32_t* wsum_dev, int32_t* excess_dev,
                      int32_t* wsq_dev, int32_t* weights_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Pooled evidence across the images of a set: every score of the keyed searches is linear in the image, so the
 * sum of a record's scores over a set of images is its score against ONE pooled row.  Additive: gsw_version() stays 500.
 *
 * gsw_pool_rows, one launch per batch of sets:
 *   signs_dev   : uint8 [B, n_bits / 8], packed sign rows (gsw_sign_pack, gsw_quant_pack, gsw_level_pack[_l]); any alignment
 *   planes_dev  : uint8 [B, P, n_bits / 8], gsw_level_pack[_l]'s planes with P in 1 .. 4, or null with P = 0: every level is 1
 *   set_ptr_dev : int32 [G + 1], 4-byte aligned: set g is the images set_ptr[g] .. set_ptr[g + 1] - 1; set_ptr[0] = 0, strictly ascending,
 *                 set_ptr[G] = B (the caller gathers the images of a set into that order; indices outside [0, B] are clipped, not read)
 *   max_set     : the size of the largest set, stated by the caller (set_ptr lives on the device)
 *   Q           : planes of the pooled rows, 1 .. 10, at least the bit length of Lmax max_set with Lmax = 2^P - 1 (1 with P = 0)
 * With lev_bj = sum_k 2^k (bit j of plane k of image b) (1 with P = 0), h_bj bit j of the sign row and S_j = sum over the set of lev_bj (1 - 2 h_bj):
 *   out_signs_dev  : uint8 [G, n_bits / 8], bit j = (S_j < 0)
 *   out_planes_dev : uint8 [G, Q, n_bits / 8], plane k = bit k of |S_j|, packed as the rows (S_j = 0: sign 0, level 0)
 *   wsum_dev       : int32 [G], sum_j |S_j|            wsq_dev : int64 [G], 8-byte aligned, sum_j S_j^2
 * Every output byte is written, no atomics, no workspace, integer arithmetic only; a set larger than max_set loses the bits above plane Q - 1.
 * GSW_ERR_BAD_ARG: null pointer (planes_dev present exactly when P > 0), set_ptr_dev / wsum_dev / wsq_dev misaligned, P outside 0..4, B, G or
 * max_set < 1, G or max_set > B, n_bits < 8 or not a multiple of 8, Q < 1 or below the bit length above when that is at most 10.
 * GSW_ERR_UNSUPPORTED: Q or that bit length above 10 (more than 1023 images at unit levels, more than 68 at 15 levels), n_bits (1 + Q) >
 * 1 048 576 (the searches' domain), n_bits (2^Q - 1) >= 2^31.  In that order; every refusal happens before any launch.
 *
 * gsw_trace_keyed_pooled_topk: gsw_trace_keyed_soft_topk for rows of Q in 1 .. 10 planes, G sets in the place of its B images.
 * records_dev, record_stride, msg_bytes, n_records, k, idx_dev, score_dev and workspace_dev (gsw_trace_keyed_workspace_bytes(G, n_records,
 * k) bytes) as gsw_trace_keyed_topk; signs_dev, planes_dev, wsum_dev as gsw_pool_rows writes them.
 *   score[g, u] = wsum[g] - 2 sum_{k < Q} 2^k popcount(plane_k[g] & (signs[g] ^ codeword[u])), an exact int32: the sum over the set's images of
 *                 gsw_trace_keyed_topk's (P = 0) or gsw_trace_keyed_soft_topk's score of record u
 *   out         : the k best records per set by (score descending, index ascending), idx = -1 / score = INT32_MIN past the end
 * GSW_ERR_BAD_ARG: as gsw_trace_keyed_soft_topk, with Q < 1 in the place of its levels.  GSW_ERR_RAGGED: n_bits is not a multiple of
 * 8 msg_bytes.  GSW_ERR_UNSUPPORTED: Q > 10, n_bits (1 + Q) > 1 048 576, n_bits (2^Q - 1) >= 2^31, G > 65535, or the 1 + Q rows, each padded
 * to whole 64-byte blocks, beyond 128 KiB of LDS (a ragged row at the very end of the domain). */
int gsw_pool_rows(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int64_t n_bits, const int32_t* set_ptr_dev, int G, int max_set, int Q,
                  uint8_t* out_signs_dev, uint8_t* out_planes_dev, int32_t* wsum_dev, int64_t* wsq_dev, void* stream);
int gsw_trace_keyed_pooled_topk(const uint8_t* signs_dev, const uint8_t* planes_dev, const int32_t* wsum_dev, int Q, int G, int64_t n_bits,
                                const uint8_t* records_dev, int64_t record_stride, int msg_bytes, int64_t n_records, int k, int32_t* idx_dev,
                                int32_t* score_dev, void* workspace_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Error-corrected payloads: the message of message_bits = M bits is a codeword of the rate-1/2, constraint-length-7
 * convolutional code (generators 0o171, 0o133; state = the last 6 inputs, the newest at bit 5, starting at 0; 6 zero tail bits), so T = M / 2
 * trellis steps carry I = T - 6 info bits: payload (M / 16 - 3 bytes, bits MSB first), CRC-16/CCITT-FALSE of the payload (0x1021, init 0xFFFF,
 * no reflection, no final xor), 2 zero pad bits.  Code bit i sits at message position (i S) mod M, S the smallest odd integer >= (isqrt(M) | 1)
 * coprime to M.  Additive: gsw_version() stays 500.
 *
 * gsw_viterbi_decode, one launch per batch, one wavefront per image: the maximum-correlation path through the trellis for the votes
 *   score_dev   : int32 [B, score_stride] (4-byte aligned, score_stride >= M elements), positive = bit 1: gsw_extract_soft[_l]'s or
 *                 gsw_decode_robust's score, or 2 counts - copies; sum_t |score[b, t]| < 2^30 (every vote of this library stays below 15 x 2^20)
 * The branch from state 2 (s & 31) + d into state s (input s >> 5) adds (2 c0 - 1) x[2t] + (2 c1 - 1) x[2t + 1], x the de-interleaved row; only
 * state 0 is reachable before step 0, an unreachable predecessor never wins, the 6 tail steps have u = 0 branches only, on equal metrics the
 * predecessor with the lower index wins, the traceback starts from state 0.  Outputs, every element written for every image:
 *   info_dev    : uint8 [B, M / 16], the I info bits MSB first (the last byte: the 2 pad bits, then zeros)
 *   message_dev : uint8 [B, M / 8], the re-encoded, re-interleaved codeword: the corrected message
 *   metric_dev  : int32 [B], the winning path's correlation = sum_p (2 message_p - 1) score[p]
 *   flips_dev   : int32 [B], positions p with message_p != (score[p] > 0)
 *   ok_dev      : int32 [B], 1 when the CRC of the payload bytes matches and the last info byte is zero, else 0
 * Integer arithmetic only, no atomics, no workspace.
 * GSW_ERR_BAD_ARG: null or misaligned pointer, B < 1, M < 64 or not a multiple of 16, score_stride < M.  GSW_ERR_UNSUPPORTED: M > 8192.
 * In that order; every refusal happens before any launch. */
int gsw_viterbi_decode(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, uint8_t* info_dev, uint8_t* message_dev, int32_t* metric_dev,
                       int32_t* flips_dev, int32_t* ok_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * The list read of error-corrected payloads.  The code, the interleaver, the info word, the branch metrics, the tail and the
 * int32 bound are gsw_viterbi_decode's; the embed and the coded message do not change.  Additive: gsw_version() stays 500.
 *
 * gsw_viterbi_list_decode, one launch per batch, one wavefront per image: a parallel list Viterbi decode with list_size = L in {1, 2, 4, 8}.  Every
 * state s keeps at most L (metric, path) entries, best first.  Before step 0 state 0 holds one entry of metric 0 and nothing else holds any.  Step t
 * merges the lists of the predecessors 2 (s & 31) + d, d in {0, 1} (d = 0 entries + bm, d = 1 entries - bm) and keeps the first L: higher metric
 * first, on equal metrics a d = 0 entry before a d = 1 entry, entries of one predecessor in their rank order; an empty slot never precedes a filled
 * one and a state holds min(L, count0 + count1) entries; in the 6 tail steps only states with s >> 5 == 0 hold any.  After step T - 1 state 0 holds L
 * paths.  ok_r: the info word of rank r passes the CRC and its last byte is zero.  The selected rank is the lowest r with ok_r, rank 0 when there is none.
 * Outputs, every element written for every image; info, message, metric, flips and ok describe the SELECTED path exactly as gsw_viterbi_decode
 * describes its single path:
 *   rank_dev    : int32 [B], the selected rank
 *   n_ok_dev    : int32 [B], the number of ranks with ok_r (more than one: the CRC alone did not single the payload out)
 * At list_size 1 the first five outputs equal gsw_viterbi_decode's byte for byte, rank is 0 and n_ok equals ok.  A row that carries no payload gets
 * ok = 1 with probability at most L 2^-18 (16 CRC bits, 2 pad bits) instead of 2^-18.
 * Integer arithmetic only, no atomics, no workspace: the survivor records (L bits per state and step) live in LDS, one slice per wavefront of
 *   wave_lds(M, L) = M (5 + 1/16 + 9 L / 2) + 256 L bytes, rounded up to 16.
 * GSW_ERR_BAD_ARG: null or misaligned pointer (score, metric, flips, ok, rank, n_ok: 4 bytes), B < 1, M < 64 or not a multiple of 16,
 * score_stride < M, list_size not in {1, 2, 4, 8}.  GSW_ERR_UNSUPPORTED: wave_lds(M, L) > 163 840 (the LDS of a compute unit): M above 17 104,
 * 11 600, 7 056 and 3 936 at L = 1, 2, 4 and 8.  In that order; every refusal happens before any launch. */
int gsw_viterbi_list_decode(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, int list_size,
                            uint8_t* info_dev, uint8_t* message_dev, int32_t* metric_dev, int32_t* flips_dev,
                            int32_t* ok_dev, int32_t* rank_dev, int32_t* n_ok_dev, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------
 * Punctured payload codes: rates 2/3 and 3/4 of the same mother code, through both reads.  Additive: gsw_version() stays 500.
 *
 * rate in {0, 1, 2} = {1/2, 2/3, 3/4} ("conv", "conv23", "conv34").  The pattern has period P = rate + 1; step t keeps, in this order, c0 c1 in phase
 * t mod P = 0, c1 in phase 1 and c0 in phase 2 (c0: 0o171, c1: 0o133; the DVB / 802.11 patterns).  N(t) = (rate + 2) (t div P) + (0, 2, 3)[t mod P] is the
 * number of kept bits of the first t steps.  T is the largest multiple of 8 with N(T) <= M, I = T - 6, the info word has T / 8 bytes: payload
 * (T / 8 - 3 bytes), CRC-16, 2 pad bits, the tail.  Kept bit j < N = N(T) sits at message position (j S) mod M; the M - N spare positions carry 0 when
 * encoded and their votes are never read.  A punctured output adds nothing to a branch metric; everything else -- states, tie rule, list order,
 * traceback, the ok rule, the int32 bound -- is gsw_viterbi_decode's and gsw_viterbi_list_decode's.
 * Outputs as theirs, with info_dev uint8 [B, T / 8], message_dev carrying 0 at the spare positions and flips counted over the N code positions only.
 * At rate 0 every output equals the older entry point's byte for byte.
 * One wavefront's LDS slice, rounded up to 16 bytes: 4 M + 9 T + M + T / 8 (plain), 4 M + 256 L + 9 T L + M + T / 8 (list).
 * GSW_ERR_BAD_ARG: what the older entry point refuses with it, and a rate outside {0, 1, 2}.  GSW_ERR_UNSUPPORTED: M > 8192 (plain); a list slice above
 * 163 840 bytes: M above 17 104, 11 600, 7 056, 3 936 (rate 0), 14 752, 9 552, 5 600, 3 040 (rate 1) and 13 808, 8 784, 5 072, 2 736 (rate 2) at
 * L = 1, 2, 4, 8.  In that order; every refusal happens before any launch. */
int gsw_viterbi_decode_rate(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, int rate, uint8_t* info_dev, uint8_t* message_dev,
                            int32_t* metric_dev, int32_t* flips_dev, int32_t* ok_dev, void* stream);
int gsw_viterbi_list_decode_rate(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, int rate, int list_size,
                                 uint8_t* info_dev, uint8_t* message_dev, int32_t* metric_dev, int32_t* flips_dev,
                                 int32_t* ok_dev, int32_t* rank_dev, int32_t* n_ok_dev, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* GSWM_H */
