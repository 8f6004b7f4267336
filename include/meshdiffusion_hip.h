/*
 * meshdiffusion_hip.h -- C ABI of libmeshdiffusion_hip.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary underneath MeshDiffusion's Python score-model
 * API.  The reference has NO C/FFI boundary on this path: its
 * "kernels" are ATen calls made from Python modules.  Each entry point below
 * therefore cites the reference Python call site it replaces
 * (paths relative to the reference repo root).
 *
 * Conventions
 *   - plain pointers + sizes only; no torch types.  All pointers are DEVICE
 *     pointers owned by the caller (PyTorch allocator); the library never
 *     allocates, frees or retains device memory.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*),
 *     re-entrant and stateless.
 *   - return value: 0 = ok, negative = MD_ERR_*, positive = hipError_t.
 *
 * This file is also what the Python host reads its ctypes binding from (meshdiffusion_amd/_lib.py parse_header), so outside
 * comments and preprocessor lines it keeps to a subset of C, and anything else is an error at import:
 *   - `#define MD_X <integer expression>`: decimal literals, earlier MD_ names, + - * and parentheses, on one line;
 *   - `enum { MD_X = <integer expression>, ... };` (an enumerator without a value is the previous one plus 1);
 *   - `typedef struct Name { members } Name;`, a member being `[const] type[*] name[, name...];` (one name after a `*`);
 *   - prototypes `type md_<name> (parameters);`, a parameter being `[const] type[*] [name]`, `(void)` for none;
 *   - types: int, int32_t, int64_t, uint32_t, uint64_t, float, double by value (void as a return type); one level of pointer
 *     to those, to void, to int8_t / uint8_t or to a struct declared above.  No arrays, no function pointers.
 *   A pointer parameter is an address to ctypes (c_void_p), except a pointer to a struct, which is that struct in HOST memory
 *   (POINTER(struct)) unless the parameter's name ends in `_dev`: an array of the struct in device memory, an address again.
 *
 * Device tensor layouts (see DESIGN.md "Data layout in HBM")
 *   NCDHW : float32 [B][C][P]                      (the reference's layout, P = D*H*W)
 *   F32B  : float32 [B][C/8][P][8]                 (8-channel blocked fp32)
 *   S16B  : bf16    [B][C/8][2][P][8]              (8-channel blocked split-bf16:
 *                                                   plane 0 = hi = bf16(x),
 *                                                   plane 1 = lo = bf16(x - hi))
 *   WPK   : bf16    [rows/NT][K/KC][taps][KC/8][2][NT][8]  packed split-bf16
 *                                                   weight tiles (one tile = one LDS image)
 *   PB16  : bf16    [guard + Pp + guard][ceil(B/8)][2][C][8 samples]   position-major, sample-blocked
 *                                                   split-bf16 on the zero-padded grid (Pp positions)
 *                                                   with zeroed guard positions: operands of md_wgrad
 */
#ifndef MESHDIFFUSION_HIP_H
#define MESHDIFFUSION_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MD_OK 0
#define MD_ERR_BAD_ARG (-1)
#define MD_ERR_UNSUPPORTED (-2)
#define MD_ERR_NO_DEVICE (-3)

#define MD_ABI_VERSION 16

/* ---- tile configurations of md_gemm_conv (compile-time instantiations) ---- */
enum {
  MD_CFG_C3_128 = 0,     /* 3x3x3 s1, tile 4x8x8,  NT=128, KC=32  (main conv)        */
  MD_CFG_C3_128_K16 = 1, /* 3x3x3 s1, tile 4x8x8,  NT=128, KC=16  (stem, Cin<=16)    */
  MD_CFG_C3_32 = 2,      /* 3x3x3 s1, tile 4x8x8,  NT=32,  KC=32  (head, Cout<=32)   */
  MD_CFG_C3_LOW = 3,     /* 3x3x3 s1, tile 4x4x4,  NT=128, KC=32  (4^3 level)        */
  MD_CFG_C3_S2 = 4,      /* 3x3x3 s2 pad(0,1), tile 4x4x4, NT=128, KC=32 (Downsample)*/
  MD_CFG_G1_128 = 5,     /* 1x1x1 / GEMM, 256 cols, NT=128, KC=32                    */
  MD_CFG_G1_128_LOW = 6, /* 1x1x1 / GEMM, 64 cols,  NT=128, KC=32                    */
  MD_CFG_G1_64_LOW = 7,  /* 1x1x1 / GEMM, 64 cols,  NT=64,  KC=32                    */
  MD_CFG_C3_128_V2 = 8,  /* C3_128 + conflict-free halo layout + software-pipelined loads     */
  MD_CFG_C3_128_SW = 9,  /* (A/B) conflict-free halo layout only                              */
  MD_CFG_C3_128_PIPE = 10, /* (A/B) pipelined loads only                                       */
  /* 11..13: reserved (ids of retired experiments; md_gemm_conv answers MD_ERR_UNSUPPORTED)                  */
  MD_CFG_C3_128_FAST = 14, /* dedicated kernel for the hot conv: C3_128_V2 layout, taps unrolled, F32B out */
  MD_CFG_C5_128_K16 = 15, /* 5x5x5 s1 pad 2, tile 4x8x8, NT=128, KC=16 (ddpm_res128 stem / mask_layer)  */
  MD_CFG_C5_32_K16 = 16,  /* 5x5x5 s1 pad 2, tile 4x8x8, NT=32,  KC=16 (ddpm_res128 head)               */
  MD_CFG_C3_128_W4 = 17,  /* experiment: 3x3x3, tile 4x4x8, NT=128, 4 waves (2 workgroups/CU)          */
  MD_CFG_C3X_32 = 18,     /* 3x3x1 taps (one dx column of a 3x3x3 kernel), tile 4x8x8, NT=32, KC=32: dx-folded head */
  MD_CFG_C5X_32_K16 = 19, /* 5x5x1 taps, NT=32, KC=16: dx-folded 5x5x5 head of ddpm_res128                        */
  MD_CFG_C3X_128_K16 = 20, /* 3x3x1 taps, NT=128, KC=16: dx-folded 3x3x3 stem (K = 4 channels x 3 dx)                    */
  MD_CFG_C5X_128 = 21,     /* 5x5x1 taps, NT=128, KC=32: dx-folded 5x5x5 stem of ddpm_res128 (K = 4 channels x 5 dx)     */
  MD_CFG_G1_128_N128 = 22, /* 1x1x1 / GEMM, 128 cols, NT=128, KC=32: three workgroups per CU (HBM-bound shortcut NINs)         */
  MD_CFG_COUNT = 23
};

enum { MD_OUT_F32B = 0, MD_OUT_S16B = 1, MD_OUT_NCDHW = 2 };
enum { MD_A_PACKED = 0, MD_A_S16B = 1 };
enum { MD_B_S16B = 0, MD_B_F32B_GN = 1 };
/* MD_PREC_BF16X3: both operands split bf16 (hi, lo), 3 MFMAs per product (default, ~1e-5 per U-Net eval).
 * MD_PREC_FP16X2: weights split fp16 (hi, lo), activations ONE fp16 (plane 0 only), 2 MFMAs per product
 *                 (~1e-3 per eval, 7e-5 after 999 sampler steps; MD_CFG_C3_128_FAST only). */
enum { MD_PREC_BF16X3 = 0, MD_PREC_FP16X2 = 1 };

/*
 * md_gemm_conv: out[b][i][j] = alpha * sum_{tap,k} A[i][tap][k] * B[b][k][pos_j + tap]
 *                              + bias[b*bias_bstride + i] + residual[b][i][j]
 * computed on the matrix cores with a bf16x3 split (hi*hi + hi*lo + lo*hi,
 * fp32 accumulate).  i = output row (output channel), j = spatial position.
 * With ksplit > 1 (F32B output only) the K-chunk range is divided over grid.z workgroups that write
 * raw partial sums to `partial`; a second, deterministic kernel adds the slices in order and applies
 * alpha / bias / residual.  Used for the 4^3 and 8^3 levels where tiles alone cannot fill 256 CUs.
 *
 * Replaces: nn.Conv3d 3x3x3 (lib/diffusion/models/layers.py:118-124 used at
 * :654,:662, ddpm_res64.py:85-87,:121), Downsample pad+stride-2 conv
 * (layers.py:626-643), Upsample nearest x2 + conv (layers.py:611-623, `ups`=1
 * folds the interpolate into the halo load), NIN 1x1x1 (layers.py:573-582)
 * and the two attention einsums (layers.py:602,606; a_src = MD_A_S16B).
 */
typedef struct MdGemmConvArgs {
  const void* a;         /* WPK weights (a_src=0) or S16B tensor [B][K/8][2][a_rows][8] (a_src=1) */
  const void* b;         /* S16B activations [B][K/8][2][P_in][8]                               */
  void* out;             /* F32B / S16B [B][rows_alloc/8].. / NCDHW [B][rows][P]                */
  const float* bias;     /* may be NULL                                                        */
  const float* residual; /* F32B [.][rows_alloc/8][P][8], may be NULL                          */
  float alpha;
  int32_t cfg;           /* MD_CFG_*                                                           */
  int32_t batch;
  int32_t rows;          /* logical output rows (Cout); stores are guarded by it               */
  int32_t rows_alloc;    /* channel count of out/residual tensors (multiple of 8)              */
  int32_t kdim;          /* K per tap (Cin), multiple of the cfg's KC                          */
  int32_t D, H, W;       /* OUTPUT spatial dims; GEMM cfgs use D=H=1, W=P                      */
  int32_t ups;           /* 1: input is nearest-upsampled x2 on the fly                        */
  int32_t a_src;         /* MD_A_*                                                             */
  int32_t out_mode;      /* MD_OUT_*                                                           */
  int32_t a_rows;        /* a_src=1: rows (P) of the A tensor                                  */
  int64_t a_bstride;     /* a_src=1: elements (bf16) between batches of A; 0 = shared          */
  int64_t bias_bstride;  /* floats between batches of bias; 0 = shared                         */
  int64_t res_bstride;   /* floats between batches of residual; 0 = shared                     */
  int64_t b_bstride;     /* elements (bf16) between batches of B; 0 = shared                   */
  float* partial;        /* ksplit>1: fp32 workspace [ksplit][B][rows_alloc/8][P][8]            */
  int32_t ksplit;        /* split the K-chunk loop over this many workgroups (grid.z); 0/1 = off */
  int32_t prec;          /* MD_PREC_*: operand format of A (weights) and B (activations)        */
  double* stats;         /* optional [B][rows_alloc][2]: per-(sample, output channel) sum and sum of   */
                         /* squares of the values written to `out`, ADDED with fp64 atomics (caller    */
                         /* zeroes) -- the GroupNorm statistics of the consumer without another pass   */
                         /* over the tensor.  F32B output; written by MD_CFG_C3_128_FAST's epilogue or,  */
                         /* with ksplit > 1, by the split-K finish kernel of any configuration; else error */
  int32_t stagger;       /* MD_CFG_C3_128_FAST: shader cycles over which the start of the first workgroup */
                         /* of each CU is spread (0 = off); measured neutral on MI355X, kept as A/B switch */
  int32_t b_mode;        /* MD_B_S16B (0) or MD_B_F32B_GN (MD_PREC_BF16X3; MD_CFG_C3_128_FAST, MD_CFG_C3_LOW without  */
                         /* `ups`, and split-only -- b_ac NULL -- MD_CFG_G1_128 / MD_CFG_G1_128_N128): `b` (and  */
                         /* `b2`) are fp32 F32B tensors [B][C/8][P_in][8]; the kernel applies                 */
                         /* y = x*ac[c][0] + ac[c][1] (GroupNorm affine), SiLU (b_silu) and the bf16 hi/lo    */
                         /* split while it stages the halo tile in LDS -- nn.GroupNorm + nn.SiLU              */
                         /* (layers.py:676-681) without a pass of their own; positions outside the grid are   */
                         /* zero AFTER the transform (the conv pads the activated tensor)                     */
  const void* b2;        /* MD_B_F32B_GN: second part of a channel-concatenated input (torch.cat([h, skip], 1), */
                         /* ddpm_res64.py:174-176): K channels [b_split, kdim); NULL when b_split >= kdim    */
  const float* b_ac;     /* MD_B_F32B_GN: [B][kdim][2] = (rstd*gamma, beta - mean*rstd*gamma) from            */
                         /* md_gn_finalize, or NULL: no affine, no SiLU (plain split: Upsample's conv)        */
  int64_t b2_bstride;    /* floats between batches of b2 (b_bstride: floats between batches of b in this mode) */
  int32_t b_split;       /* channels taken from `b` (multiple of 8)                                           */
  int32_t b_silu;        /* apply SiLU after the affine                                                      */
} MdGemmConvArgs;

int md_abi_version(void);
/* number of visible HIP devices, or negative MD_ERR */
int md_device_count(void);

int md_gemm_conv(const MdGemmConvArgs* args, void* stream);
/* bytes of `partial` workspace md_gemm_conv needs for these args (0 when ksplit <= 1) */
int64_t md_gemm_conv_partial_bytes(const MdGemmConvArgs* args);
/* bytes of LDS and threads per workgroup of a cfg (for DESIGN/bench reporting) */
int md_gemm_conv_cfg_info(int32_t cfg, int32_t* nt, int32_t* kc, int32_t* cols,
                          int32_t* taps, int32_t* lds_bytes, int32_t* threads);

/*
 * md_pack_weights: fp32 weights -> WPK tiles (device side, run once per load).
 *   w      : float32, element (row i, k, tap) at  w[i*s_row + k*s_k + tap*s_tap]
 *            (Conv3d weight [Co][Ci][27]: s_row=Ci*27, s_k=27, s_tap=1;
 *             NIN W [Ci][Co] (layers.py:576): s_row=1, s_k=Co, s_tap=0)
 *   rows,kdim : logical sizes; tiles are zero-padded to NT / KC multiples.
 */
int md_pack_weights(const float* w, void* wpk, int32_t rows, int32_t kdim, int32_t taps,
                    int64_t s_row, int64_t s_k, int64_t s_tap, int32_t nt, int32_t kc,
                    int32_t prec, void* stream);
int64_t md_packed_weight_bytes(int32_t rows, int32_t kdim, int32_t taps, int32_t nt, int32_t kc);

/*
 * GroupNorm statistics + apply (+SiLU) + bf16 split.
 * Replaces nn.GroupNorm(32, C, eps=1e-6) + nn.SiLU (layers.py:652,660,676,681,
 * :589; ddpm_res64.py:120,186) and torch.cat([h, skip], 1) (ddpm_res64.py:174-176):
 * a concatenated input is expressed as two calls with channel offsets.
 *
 * md_gn_stats : accumulates per-(b, channel) sum / sum-of-squares (double) of an
 *               F32B tensor x[B][C/8][P][8] into sums[B][c_total][2] at channel
 *               offset c_off.  `sums` must be zeroed by the caller (md_zero).
 * md_gn_finalize: per-(b,c) params float4 = (mean(group), rstd(group)*gamma[c], beta[c], rstd(group))
 *               (biased variance, as torch's GroupNorm); optionally also the folded affine `ac`.
 * md_gn_apply : y = (x-mean)*rstd*gamma + beta (norm=1) ; y = silu(y) (silu=1); writes the
 *               split-bf16 S16B tensor out[B][c_total/8][2][P][8] at c_off.
 *               norm=0 copies/splits raw x (used for the NIN shortcut input).
 *               out_raw (may be NULL): second S16B tensor of the same shape receiving the bf16 split of
 *               the raw x from the same read (ResnetBlock: GN path and NIN shortcut share one pass).
 *               `silu` is a bit field: 1 = apply SiLU, 4 = MD_PREC_FP16X2 output (plane 0 = fp16(y),
 *               plane 1 not written), 2 = debug: round y to fp16 before the bf16 split.
 *               drop_p > 0 (training, nn.Dropout of ResnetBlockDDPM, layers.py:682): after SiLU, y is zeroed with
 *               probability drop_p and scaled by 1/(1-drop_p) otherwise.  The mask is a counter-based hash of
 *               (drop_seed, b, channel quad, position) -- md_gn_bwd_stats/apply regenerate it from the same
 *               (drop_p, drop_seed); md_dropout_scale writes it out as an F32B tensor of {0, 1/(1-p)} (tests).
 */
int md_gn_stats(const float* x, double* sums, int32_t batch, int32_t C, int64_t P,
                int32_t c_total, int32_t c_off, void* stream);
int md_gn_finalize(const double* sums, const float* gamma, const float* beta,
                   float* params, int32_t batch, int32_t c_total, int32_t groups,
                   int64_t P, float eps, float* ac, void* stream);
                   /* ac (may be NULL): float [B][c_total][2] = (rstd*gamma, beta - mean*rstd*gamma), the affine
                    * form consumed by md_gemm_conv's MD_B_F32B_GN operand mode */
int md_gn_apply(const float* x, const float* params, void* out, void* out_raw, int32_t batch,
                int32_t C, int64_t P, int32_t c_total, int32_t c_off, int32_t norm,
                int32_t silu, float drop_p, uint64_t drop_seed, void* stream);
int md_dropout_scale(float* out, int32_t batch, int32_t C, int64_t P, int32_t c_total, int32_t c_off,
                     float drop_p, uint64_t drop_seed, void* stream);
int md_zero(void* p, int64_t bytes, void* stream);

/*
 * Timestep embedding + dense layers (layers.py:542-556, ddpm_res64.py:132-136,
 * layers.py:679-680).
 * md_timestep_embedding: emb[b] = [sin(t_b*f_j) | cos(t_b*f_j)], f_j = exp(-ln(1e4)*j/(dim/2-1)).
 * md_linear: y[b][o] = sum_i act(x[b][i]) * w[o*in + i] + bias[o]  (act = SiLU if silu_in).
 */
int md_timestep_embedding(const float* t, float* emb, int32_t batch, int32_t dim, void* stream);
int md_linear(const float* x, const float* w, const float* bias, float* y, int32_t batch,
              int32_t in_dim, int32_t out_dim, int32_t silu_in, void* stream);

/*
 * md_fold_dx: second half of the dx-folded head convolution (ddpm_res64.py:121,189 / ddpm_res128.py:132,208).  The conv
 * runs with rows = (co, dx) and k x k x 1 taps (MD_CFG_C3X_32 / MD_CFG_C5X_32_K16: the 4 output channels would fill 4
 * of the 32 rows of an MFMA tile, the kx (co, dx) pairs fill 12 / 20), y: F32B [B][rows_alloc/8][P][8]; this kernel adds
 * the kx shifted columns: out[b][co][z][y][x] = bias[co] + sum_dx y[b][co*kx + dx][z][y][x + dx - kx/2] (x in range),
 * NCDHW fp32 [B][co][D*H*W].
 */
int md_fold_dx(const float* y, const float* bias, float* out, int32_t batch, int32_t co, int32_t kx, int32_t rows_alloc,
               int32_t D, int32_t H, int32_t W, void* stream);
/* NCDHW fp32 -> S16B with kx x-shifted copies per channel (channel ci*kx + dx = x[ci] shifted by dx - kx/2 along x, zero
 * outside): operand of the dx-folded stem conv (ddpm_res64.py:87,140 / ddpm_res128.py:90,150), MD_CFG_C3X_128_K16 / C5X_128. */
int md_ncdhw_to_s16b_xfold(const float* x, void* out, int32_t batch, int32_t C, int32_t kx, int32_t c_pad, int32_t D, int32_t H,
                           int32_t W, void* stream);
/* NCDHW fp32 [B][C][P] -> S16B [B][c_pad/8][2][P][8] (channels >= C zero filled). */
int md_ncdhw_to_s16b(const float* x, void* out, int32_t batch, int32_t C, int32_t c_pad,
                     int64_t P, void* stream);
/* F32B [B][C/8][P][8] <-> NCDHW [B][C][P] (tests / debugging / parity probes). */
int md_f32b_to_ncdhw(const float* x, float* out, int32_t batch, int32_t C, int64_t P, void* stream);
int md_ncdhw_to_f32b(const float* x, float* out, int32_t batch, int32_t C, int64_t P, void* stream);
int md_s16b_to_ncdhw(const void* x, float* out, int32_t batch, int32_t C, int64_t P, void* stream);

/*
 * Attention softmax over keys (layers.py:603-605).  s: F32B-like [B][N/8][N][8]
 * holding S^T (keys blocked by 8, queries as positions); p: S16B [B][N/8][2][N][8].
 */
int md_softmax_keys(const float* s, void* p, int32_t batch, int32_t n_keys, int32_t n_q,
                    void* stream);

/*
 * md_nin_f32: the ResnetBlock shortcut NIN_0 (1x1x1 channel mixing, layers.py:573-582 used at :667,:688) for the HBM-bound
 * shapes, as a persistent, barrier-free streaming kernel: the whole WPK weight matrix (MD_CFG_G1_128 tiles, K <= 256) is
 * resident in LDS, the fp32 input goes HBM -> registers -> bf16 split -> MFMA.
 *   x1, x2 : F32B [B][c1/8][P][8], [B][c2/8][P][8]: the channel parts of torch.cat([h, skip], 1) (x2 NULL when c2 = 0)
 *   wpk    : md_pack_weights(W, rows = cout, kdim = c1 + c2, taps = 1, nt = 128, kc = 32)
 *   out    : F32B [B][cout/8][P][8] = W^T x + bias
 * Supported: cout == 128, c1 + c2 in {128, 256}, c1 % 16 == c2 % 16 == 0, P % 256 == 0; otherwise MD_ERR_UNSUPPORTED
 * (md_gemm_conv handles every shape).  n_cu: workgroups to launch (0 = 256, one per CU).
 */
int md_nin_f32(const float* x1, const float* x2, int32_t c1, int32_t c2, const void* wpk, const float* bias,
               float* out, int32_t batch, int32_t cout, int64_t P, int32_t n_cu, void* stream);

/*
 * Winograd F(2,3)-along-w path of the 3x3x3 stride-1 convolution (inference): nn.GroupNorm + nn.SiLU + nn.Conv3d
 * (layers.py:676-681, :118-124), on torch.cat([h, skip], 1) (ddpm_res64.py:174-176) or on the nearest-x2 upsampled input
 * (layers.py:618-623).  2/3 of the matrix-core work of the direct form; bf16x3 products, fp32 accumulation.
 *
 * md_wino_prep: fp32 parts -> T[B][C/8][4][2][D][H][W/2][8 bf16]  (C = c1 + c2; 4 = transformed inputs d0-d2, d1+d2, d2-d1,
 *   d1-d3 of the output pair (2i, 2i+1), d_k = activated input at x = 2i-1+k, zero outside the grid; 2 = bf16 hi / lo plane)
 *   x1, x2 : F32B [B][c1/8][Pin][8], [B][c2/8][Pin][8] (x2 NULL when c2 = 0); Pin = D*H*W, or D*H*W/8 with ups = 1
 *   ac     : [B][C][2] folded GroupNorm affine of md_gn_finalize (y = x*ac[c][0] + ac[c][1]), or NULL: no affine, no SiLU
 *   D, H, W: OUTPUT grid of the convolution (W even); md_wino_operand_bytes gives the size of T
 *   drop_p > 0 (training): nn.Dropout after SiLU with the mask of md_gn_apply for the same (drop_p, drop_seed) -- the forward
 *            conv and the taped activation see the same zeros.  The mask belongs to the SOURCE tensor: C = c1 + c2 channels of
 *            Pin positions (two parts and ups = 1 included; the registered models use one part, no upsampling)
 * md_wino_pack_weights: Conv3d weight fp32 -> transformed, split tiles in fragment order; element (row, k, tap t27 = (kd*3+kh)*3+kw)
 *   is read at w[row*s_row + k*s_k + t27] ([Cout][Cin][3][3][3]: s_row = Cin*27, s_k = 27, flip = 0) or, with flip = 1, at
 *   w[row*s_row + k*s_k + 26 - t27] (the data-gradient conv of W[Co][Ci][27]: cout = Ci, cin = Co, s_row = 27, s_k = Ci*27)
 *   [Cout/128][Cin/16][kd*3+kh][4][row tile 4][plane 2][k-group 2][row 32][8 bf16]  (md_wino_weight_bytes)
 * md_conv3_wino: out F32B [B][cout/8][P][8] = conv(T, wpk) + bias[b*bias_bstride + co] + residual; stats as in MdGemmConvArgs
 *   Supported: cout % 128 == 0, cin % 32 == 0, D % 4 == 0, H % 8 == 0, W % 8 == 0, D*H*W < 2^28; else MD_ERR_UNSUPPORTED.
 *   variant: 0 (others are A/B schedules and timing-only ablations of tools/bench_wino.py).
 */
int64_t md_wino_operand_bytes(int32_t batch, int32_t cin, int32_t D, int32_t H, int32_t W);
int md_wino_prep(const float* x1, const float* x2, int32_t c1, int32_t c2, const float* ac, int32_t silu, int32_t ups,
                 void* t_out, int32_t batch, int32_t D, int32_t H, int32_t W, float drop_p, uint64_t drop_seed, void* stream);
int64_t md_wino_weight_bytes(int32_t cout, int32_t cin);
int md_wino_pack_weights(const float* w, void* wpk, int32_t cout, int32_t cin, int64_t s_row, int64_t s_k, int32_t flip,
                         void* stream);
int md_conv3_wino(const void* t_in, const void* wpk, float* out, const float* bias, int64_t bias_bstride,
                  const float* residual, int64_t res_bstride, double* stats, int32_t batch, int32_t cin, int32_t cout,
                  int32_t D, int32_t H, int32_t W, int32_t variant, void* stream);

/*
 * The same convolution (same reference lines, inference only) in the "f16f8" arithmetic: every product a*b of the Winograd-domain
 * contraction is  fp16(a) fp16(b)  +  [e4m3(a) e4m3(b_lo 2^11) + e4m3(a_lo 2^11) e4m3(b)] 2^-11,  a_lo = a - fp16(a): one
 * v_mfma_f32_32x32x16_f16 plus half a K-concatenated v_mfma_scale_f32_32x32x64_f8f6f4 (OCP e4m3, E8M0 scale) = two 32-cycle
 * matrix-core units per product where bf16x3 issues three; fp32 accumulation.  Error of one conv vs fp64 1.3e-5 (bf16x3 5.5e-6).
 * md_wino_prep_f8: as md_wino_prep (no dropout; W must divide 256), T of the same geometry with plane 0 = 8 fp16 and plane 1 =
 *   [e4m3(t) x 8 | e4m3((t - fp16(t)) 2^11) x 8]; size: md_wino_operand_bytes.
 * md_wino_pack_weights_f8 (two kernels: max |w| -> power-of-two pre-scale 2^sw kept on the device, then the fragments):
 *   [Cout/128][Cin*9/32 step pairs][4][row tile 4][piece 4][lane 64][16 B] + a 256-byte header {max |w|, sw, 2^-sw};
 *   size: md_wino_weight_bytes_f8.  Forward orientation only (s_row = Cin*27, s_k = 27 for [Cout][Cin][3][3][3]).
 * md_conv3_wino_f8: arguments, supported shapes and outputs as md_conv3_wino with T / wpk from the two calls above.
 * eq (md_wino_prep_f8 / _f6 and md_wino_pack_weights_f8 / _f6; may be NULL = none): float [Cin], the static per-input-channel
 *   power-of-two equaliser written by md_wino_equaliser.  The operand pass multiplies the activated value of channel c by eq[c], the
 *   weight fragments hold w[:, c] / eq[c] (both exact): the convolution is unchanged, but the channels of a K block reach the
 *   4-bit-significand cross-term images at comparable magnitudes whatever the GroupNorm affine in front of the conv is.  The SAME
 *   vector must be given to the operand pass and to the weight packing of a layer.
 * md_wino_equaliser (csrc/wino_eq.hip): eq[c] = 2^round(log2(g_c / a_c) / 2), clamped to 2^+-14, with a_c = rms of
 *   silu(gamma_c z + beta_c) over z ~ N(0, 1) (64-point midpoint rule on [-6, 6]) -- what nn.GroupNorm + nn.SiLU
 *   (layers.py:652,660,676-681) hand the conv, per channel -- and g_c = rms of w[:, c, :, :, :]; w element (co, ci, t27) at
 *   w[co * s_row + ci * s_k + t27].  gamma / beta: the GroupNorm affine over the (concatenated) Cin input channels.  The exponent is
 *   additionally bounded by the fp16 headroom of the operand: eq[c] (8 |gamma_c| + |beta_c|) 2 < 2^15.
 * md_wino_equaliser_measured (ABI 15): the same with a_c^2 = a2m[c], the MEASURED per-channel mean square of the operand (float [Cin]
 *   from md_wino_operand_ms over a calibration evaluation); gamma / beta may both be NULL (a conv on a tensor no GroupNorm precedes:
 *   Upsample, layers.py:611-623).  GroupNorm normalises groups of channels, so a channel's own scale inside its group -- which the
 *   static estimate cannot see -- is part of the measurement.  All exponents are then shifted by one common u so that
 *   max_c eq[c] sqrt(a2m[c]) = 2^0 (+-1/2): the operand's fp16 plane sits mid-range whatever the tensor's absolute magnitude.
 * md_wino_operand_ms (ABI 15): ms[c] += mean over samples and positions of act(x[c])^2 for up to two concatenated F32B parts, act =
 *   the conv's operand transform (x * ac[..][0] + ac[..][1], SiLU) or the identity (ac NULL); ms zeroed by the caller.
 */
int md_wino_equaliser(const float* gamma, const float* beta, const float* w, int32_t cout, int32_t cin, int64_t s_row, int64_t s_k,
                      float* eq, void* stream);
int md_wino_equaliser_measured(const float* gamma, const float* beta, const float* w, const float* a2m, int32_t cout, int32_t cin,
                               int64_t s_row, int64_t s_k, float* eq, void* stream);
int md_wino_operand_ms(const float* x1, const float* x2, int32_t c1, int32_t c2, const float* ac, int32_t silu, int32_t batch, int64_t P,
                       float* ms, void* stream);
int md_wino_prep_f8(const float* x1, const float* x2, int32_t c1, int32_t c2, const float* ac, int32_t silu, int32_t ups,
                    const float* eq, void* t_out, int32_t batch, int32_t D, int32_t H, int32_t W, void* stream);
int64_t md_wino_weight_bytes_f8(int32_t cout, int32_t cin);
int md_wino_pack_weights_f8(const float* w, const float* eq, void* wpk, int32_t cout, int32_t cin, int64_t s_row, int64_t s_k, void* stream);
int md_conv3_wino_f8(const void* t_in, const void* wpk, float* out, const float* bias, int64_t bias_bstride,
                     const float* residual, int64_t res_bstride, double* stats, int32_t batch, int32_t cin, int32_t cout,
                     int32_t D, int32_t H, int32_t W, void* stream);
/*
 * Training (ABI 15): the data-gradient convs of a step in the f16f6 arithmetic.
 * md_absmax: amax_bits[0] = max(amax_bits[0], max |x|) as the bit pattern of the float (the caller zeroes the word; x 16-byte aligned).
 * md_wino_prep_dual_f6: as md_wino_prep_dual for ONE raw fp32 part (an output gradient; c % 16 == 0, W | 256), except that T is the
 *   f16f6 operand of md_conv3_wino_f6 of 2^k x the tensor (gradient magnitudes lifted into the fp16 plane's normal range, saturated
 *   at its ends): amax_bits != NULL: k from the word md_absmax filled for this tensor (max |x| 2^k in [16, 32)); NULL: 2^k = tscale.
 *   U (md_wgrad_wino's operand) and sums are those of the unscaled tensor, bit-identical to md_wino_prep_dual's.
 * md_conv3_wino_f6_scaled: md_conv3_wino_f6 whose result is multiplied by out_scale (exact: a power of two) and, with amax_bits, by
 *   the inverse of the lift the operand pass derived from the same word.
 * The weights: an MD_PACK_WINO_F6 job of md_pack_batch (fixed pre-scale, `flip` for the data-gradient orientation).
 */
int md_absmax(const float* x, int64_t n, uint32_t* amax_bits, void* stream);
int md_wino_prep_dual_f6(const float* x, int32_t c, void* t_out, void* u_out, float* sums, float tscale, const uint32_t* amax_bits,
                         int32_t batch, int32_t D, int32_t H, int32_t W, void* stream);
int md_conv3_wino_f6_scaled(const void* t_in, const void* wpk, float* out, const float* bias, int64_t bias_bstride,
                            const float* residual, int64_t res_bstride, double* stats, int32_t batch, int32_t cin, int32_t cout,
                            int32_t D, int32_t H, int32_t W, float out_scale, const uint32_t* amax_bits, void* stream);

/*
 * The same convolution in the "f16f6" arithmetic: as f16f8, the two cross terms from MX block-scaled OCP e2m3 images (a K block = 16
 * channels x (value, (value - fp16(value)) 2^11) with one power-of-two scale), which the same K = 64 MFMA executes at twice its e4m3
 * rate (format code 2; measured 0.85 of the f16f8 pair-step in the fp16 mix, tools/probes/f6_probe.hip).  Error of one conv vs fp64
 * 1.7e-5 (tools/f16f8_numerics.py).  Buffers, sizes and arguments as the _f8 calls; plane 1 of T / pieces 2-3 of the weight
 * fragments hold the 32-byte record [6 dwords of codes | E8M0 byte | 0] of a block, split over its two 8-channel items.
 * md_wino_prep_f6 needs c1 and c2 to be multiples of 16 (whole K blocks per part).
 */
int md_wino_prep_f6(const float* x1, const float* x2, int32_t c1, int32_t c2, const float* ac, int32_t silu, int32_t ups,
                    const float* eq, void* t_out, int32_t batch, int32_t D, int32_t H, int32_t W, void* stream);
int md_wino_pack_weights_f6(const float* w, const float* eq, void* wpk, int32_t cout, int32_t cin, int64_t s_row, int64_t s_k, void* stream);
int md_conv3_wino_f6(const void* t_in, const void* wpk, float* out, const float* bias, int64_t bias_bstride,
                     const float* residual, int64_t res_bstride, double* stats, int32_t batch, int32_t cin, int32_t cout,
                     int32_t D, int32_t H, int32_t W, void* stream);

/*
 * md_wino_prep_f6_nin: one pass over the input of a ResnetBlock with a NIN shortcut (inference).  Purely additive: MD_ABI_VERSION stays
 * 16.  The block input cat(x1, x2) is read ONCE by a persistent workgroup of md_nin_f32's structure, which writes
 *   t_out : exactly the bytes md_wino_prep_f6(x1, x2, c1, c2, ac, silu, ups = 0, eq, ...) writes (Conv_0's f16f6 operand), and
 *   res   : exactly the bytes md_nin_f32(x1, x2, c1, c2, wpk, bias, ..., cout = 128) writes (the shortcut), F32B [B][16][P][8].
 * wpk == NULL: the operand only (bias and res are ignored) -- a persistent, prefetching form of md_wino_prep_f6.
 * Supported: what both take -- c1 + c2 in {128, 256}, c1 % 16 == c2 % 16 == 0, W even and a divisor of 256, D H W % 256 == 0 (and
 * D H W <= 2^25); the argument errors of md_wino_prep_f6 / md_nin_f32 are MD_ERR_BAD_ARG, other shapes MD_ERR_UNSUPPORTED.
 * n_cu: workgroups to launch (0 = 256, one per CU).
 */
int md_wino_prep_f6_nin(const float* x1, const float* x2, int32_t c1, int32_t c2, const float* ac, int32_t silu, const float* eq,
                        void* t_out, const void* wpk, const float* bias, float* res, int32_t batch, int32_t D, int32_t H, int32_t W,
                        int32_t n_cu, void* stream);

/*
 * The operand of an Upsample conv without its duplicates (inference).  Purely additive: MD_ABI_VERSION stays 16, every entry point
 * above keeps its signature, layout and bits.  fmt = MD_WINO_FMT_*: the arithmetic (md_wino_prep_v2 / _f8 / _f6 and md_conv3_wino /
 * _f8 / _f6 above).
 * md_wino_prep_upsdh: those passes with ups = 1 (no dropout), T in the COMPACT layout [B][C/8][4][2][D/2][H/2][W/2] items of 16 bytes:
 *   one row per source (z', y') instead of the four identical rows (2z' + i, 2y' + j) -- the transform runs along w only -- i.e.
 *   rows (2z', 2y') of the full operand, a quarter of md_wino_operand_bytes.  D, H, W: the OUTPUT grid, all even; W must divide 256
 *   and D*H*W/4 be a multiple of 256, else MD_ERR_UNSUPPORTED.
 * md_conv3_wino_upsdh: md_conv3_wino / _f8 / _f6 on the compact operand; arguments, supported shapes and results (bit for bit) as theirs.
 */
#define MD_WINO_FMT_BF16X3 0
#define MD_WINO_FMT_F16F8 1
#define MD_WINO_FMT_F16F6 2
int md_wino_prep_upsdh(int32_t fmt, const float* x1, const float* x2, int32_t c1, int32_t c2, const float* ac, int32_t silu,
                       const float* eq, void* t_out, int32_t batch, int32_t D, int32_t H, int32_t W, void* stream);
int md_conv3_wino_upsdh(int32_t fmt, const void* t_in, const void* wpk, float* out, const float* bias, int64_t bias_bstride,
                        const float* residual, int64_t res_bstride, double* stats, int32_t batch, int32_t cin, int32_t cout,
                        int32_t D, int32_t H, int32_t W, void* stream);

/*
 * md_conv3_wino_upsfold (csrc/conv3_wino_upsfold.hip; inference, purely additive): the Upsample conv with the nearest-x2 taps
 * folded into the weights.  Output (Z, Y) = (2z + a, 2y + b) is a 2 x 2 (d, h) x 3 (w) conv of the SOURCE rows for each phase
 * p = 2a + b: 4 (kd, kh) tap steps per 16-channel chunk instead of 9.
 *   fmt      : MD_WINO_FMT_F16F6 only; any other format, or a residual operand, is MD_ERR_UNSUPPORTED
 *   t_in     : the operand of md_wino_prep_upsdh (t_full = 0, compact layout) or of md_wino_prep_f6 with ups = 1 (t_full = 1): the
 *              kernel reads row (z', y') of the one, row (2z', 2y') of the other -- the same bits, the same result
 *   wpk      : md_wino_pack_weights_f6 with rows = 4 cout of the folded tensor [4 cout][cin][3][3][3]: row p * cout + co holds phase
 *              p of output channel co, taps pre-summed over the coinciding source rows (a = 0: (w0, w1 + w2, 0), a = 1: (0, w0 + w1, w2)
 *              along d; b likewise along h), the five dead (kd, kh) taps zero.  The image keeps its 9-tap layout; dead taps are not read.
 *   cout     : the conv's output channels (multiple of 128); cin a multiple of 32; D, H, W the OUTPUT grid: D / 2 a multiple of 4,
 *              H / 2 of 8, W of 8.  out, bias, stats as md_conv3_wino_f6.
 */
int md_conv3_wino_upsfold(int32_t fmt, const void* t_in, int32_t t_full, const void* wpk, float* out, const float* bias,
                          int64_t bias_bstride, const float* residual, int64_t res_bstride, double* stats, int32_t batch,
                          int32_t cin, int32_t cout, int32_t D, int32_t H, int32_t W, void* stream);

/*
 * md_conv3_wino_splitk (csrc/conv3_wino.hip; inference, purely additive: MD_ABI_VERSION stays 16): md_conv3_wino / _f8 / _f6 with the K
 * loop cut into `ksplit` slices of cin / ksplit channels, for launches whose (tiles x batch x cout / 128) workgroups leave most of the
 * chip idle (the 8^3 level).  A slice is a batch entry of the same operand: the conv kernel runs ksplit times the workgroups and writes
 * fp32 partial sums to `workspace` [ksplit][batch][cout/8][P][8]; the split-K finish kernel of md_gemm_conv then adds the slices in the
 * order 0 .. ksplit-1 and applies bias, residual and statistics.  Two runs give the same bits.
 *   fmt             : MD_WINO_FMT_*; t_in and wpk are the unsplit launch's operand and packed weights (md_wino_prep* / md_wino_pack_weights*)
 *   workspace       : at least md_conv3_wino_splitk_workspace_bytes(batch, cout, D, H, W, ksplit) = ksplit * batch * cout * P * 4 bytes
 *   bias, residual, stats, strides, batch, cin, cout, D, H, W : as md_conv3_wino
 * MD_ERR_BAD_ARG (nothing is launched): ksplit < 2, a null or misaligned pointer (16 bytes; bias 4, stats 8), a workspace that is too
 * small; MD_ERR_UNSUPPORTED (nothing is launched): cin not a multiple of 32 * ksplit (a slice is whole pair-steps), cout not a multiple
 * of 128, a grid md_conv3_wino does not take, more workgroups than a launch can have.
 */
int64_t md_conv3_wino_splitk_workspace_bytes(int32_t batch, int32_t cout, int32_t D, int32_t H, int32_t W, int32_t ksplit);
int md_conv3_wino_splitk(int32_t fmt, const void* t_in, const void* wpk, void* workspace, int64_t workspace_bytes, float* out,
                         const float* bias, int64_t bias_bstride, const float* residual, int64_t res_bstride, double* stats,
                         int32_t batch, int32_t cin, int32_t cout, int32_t D, int32_t H, int32_t W, int32_t ksplit, void* stream);

/*
 * md_conv3_stem: the dx-folded 3x3x3 input convolution from 4 channels (csrc/conv3_stem.hip; ddpm_res64.py:87-92 applied
 * :138-146: conv3x3(channels, nf)(x) + pos_layer(coords) + mask_layer(mask)) with the GroupNorm sums of its output: replaces
 * md_gemm_conv(MD_CFG_C3X_128_K16) + md_gn_stats.
 *   x16      : S16B [B][2][2][P][8]: the operand of md_ncdhw_to_s16b_xfold(kx = 3, c_pad = 16)
 *   wpk      : md_pack_weights(W2, rows = cout, kdim = 12 (padded to 16), taps = 9, nt = 128, kc = 16), W2[co][(ci, kx)][kd][kh]
 *   out      : F32B [B][cout/8][P][8] = conv + bias[co] + residual[co][p]
 *   residual : F32B [cout/8][P][8] shared by the batch (the input-independent terms), or NULL;  bias: [cout] or NULL
 *   stats    : optional zeroed double [B][cout][2] += per-(sample, channel) (sum, sum of squares) of out
 * Supported: cout % 8 == 0, D % 4 == 0, H % 8 == 0, W % 8 == 0; else MD_ERR_UNSUPPORTED.
 */
int md_conv3_stem(const void* x16, const void* wpk, float* out, const float* bias, const float* residual, double* stats,
                  int32_t batch, int32_t cout, int32_t D, int32_t H, int32_t W, void* stream);

/*
 * md_conv3_head: GroupNorm + SiLU + the dx-folded 3x3x3 output head in one kernel for inference (csrc/conv3_head.hip;
 * ddpm_res64.py:120-121 applied :186-189): replaces md_gn_apply + md_gemm_conv(MD_CFG_C3X_32); md_fold_dx finishes the conv.
 *   x   : F32B [B][cin/8][P][8] (the un-normalised tensor);  ac: [B][cin][2] folded GroupNorm affine of md_gn_finalize
 *   wpk : md_pack_weights(W2, rows = co * 3, kdim = cin, taps = 9, nt = 32, kc = 16), W2[(co, kw)][ci][kd][kh] (see md_fold_dx)
 *   y   : F32B [B][rows_alloc/8][P][8], rows (co, kw); no bias
 * Supported: cin % 32 == 0, rows_alloc in {8, 16, 24, 32}, D % 4 == 0, H % 8 == 0, W % 8 == 0, D*H*W < 2^30.
 */
int md_conv3_head(const float* x, const float* ac, const void* wpk, float* y, int32_t batch, int32_t cin, int32_t rows_alloc,
                  int32_t D, int32_t H, int32_t W, void* stream);

/*
 * md_conv3_stem_dgrad: data gradient of the 3x3x3 stem conv (csrc/conv3_head.hip, the head kernel's second instantiation;
 * ddpm_res64.py:72 applied :150), dx-folded like the head; md_fold_dx (kx = 3, bias NULL) finishes it:
 *   dx[b][ci][p] = sum_co sum_tap W[co][ci][tap] g0[b][co][p - (tap - 1)],  ci < 4 (rows (ci, kw): 12 of rows_alloc = 16)
 *   g0  : F32B [B][cout/8][P][8], the gradient of the stem's output, read as raw fp32 (no affine, no SiLU; bf16x3 split inside)
 *   wpk : md_pack_weights(W2, rows = ci * 3, kdim = cout, taps = 9, nt = 32, kc = 16),
 *         W2[(ci, kw)][co][kd][kh] = W[co][ci][2 - kd][2 - kh][2 - kw] (the flipped, transposed stem weight)
 *   y   : F32B [B][rows_alloc/8][P][8], rows (ci, kw)
 * Null or 16-byte-misaligned pointers, batch <= 0: MD_ERR_BAD_ARG.
 * Supported: cout % 32 == 0, rows_alloc in {8, 16, 24, 32}, D % 4 == 0, H % 8 == 0, W % 8 == 0, D*H*W < 2^30;
 * else MD_ERR_UNSUPPORTED.  Purely additive: MD_ABI_VERSION stays 16, no existing entry point changes.
 */
int md_conv3_stem_dgrad(const float* g0, const void* wpk, float* y, int32_t batch, int32_t cout, int32_t rows_alloc,
                        int32_t D, int32_t H, int32_t W, void* stream);

/*
 * md_pack_batch: several md_pack_weights / md_wino_pack_weights jobs in one launch (csrc/pack_batch.hip; a training step
 * re-packs every weight once: ~260 launches otherwise).  Bit-identical to the single-weight entry points.
 *   jobs_dev     : DEVICE array of n_jobs MdPackJob, sorted by block0; job j owns the blocks from block0 on
 *   total_blocks : sum over jobs of their block counts
 *   tiled = 0    : one 16-byte item per thread; a job has ceil(n_items / 256) blocks
 *     kind MD_PACK_WPK : fields as the arguments of md_pack_weights (n_items = md_packed_weight_bytes / 16)
 *     kind MD_PACK_WINO: rows = cout, kdim = cin, s_row, s_k, flip as md_wino_pack_weights (n_items = md_wino_weight_bytes / 16)
 *     kind MD_PACK_WINO_F6 (ABI 15): the f16f6 fragments of md_conv3_wino_f6 with a FIXED pre-scale 2^prec in place of the max |w|
 *                        pass of md_wino_pack_weights_f6 (no equaliser), `flip` as above; n_items = md_wino_weight_bytes_f8 / 16
 *                        (fragments + the 256-byte header, which the job writes)
 *   tiled = 1    : MD_PACK_WPK jobs only, taps > 1 with s_tap = +-1, 16 * kc * taps <= 13824 and nt % 16 == 0: a block stages 16
 *                  rows x one K chunk x all taps through LDS (contiguous reads, 256-byte write runs); a job has
 *                  ceil(rows / nt) * (nt / 16) * ceil(kdim / kc) blocks.  The form for the 3x3x3 weights, which hold most of the
 *                  parameters.  tiled = taps * 100 + kc (2732, 2716, 932, 916): the same with that geometry compiled in
 *                  (every job of the table must have it; float4 source reads).
 *   tiled = 3    : MD_PACK_WINO jobs, block-cooperative (a block = 32 rows x 16 channels x 27 taps); a job has
 *                  (cout / 32) * (cin / 16) blocks.
 */
enum { MD_PACK_WPK = 0, MD_PACK_WINO = 1, MD_PACK_WINO_F6 = 2 };
typedef struct MdPackJob {
  const float* w;
  void* out;
  int64_t s_row, s_k, s_tap, n_items, block0;
  int32_t rows, kdim, taps, nt, kc, prec, flip, kind;
} MdPackJob;
int md_pack_batch(const MdPackJob* jobs_dev, int32_t n_jobs, int64_t total_blocks, int32_t tiled, void* stream);

/*
 * md_conv3_s2: the stride-2 3x3x3 convolution of Downsample (layers.py:626-643: F.pad(x, (0, 1, 0, 1, 0, 1)) +
 * nn.Conv3d(C, C, 3, stride=2, padding=0)) for inference, reading the raw fp32 tensor (csrc/conv3_s2.hip): replaces the
 * split pass md_gn_apply(norm = 0) + md_gemm_conv(MD_CFG_C3_S2).  bf16x3 products, fp32 accumulation.
 *   x      : F32B [B][cin/8][(2D)(2H)(2W)][8]
 *   wpk    : md_pack_weights(W, rows = cout, kdim = cin, taps = 27, nt = 128, kc = 16)
 *   out    : F32B [B][rows_alloc/8][D*H*W][8] = conv + bias[b*bias_bstride + co]   (D, H, W: OUTPUT grid)
 *   stats  : optional zeroed double [B][rows_alloc][2] += per-(sample, channel) (sum, sum of squares) of out
 * Supported: cin % 32 == 0, D % 4 == 0, H % 8 == 0, W % 8 == 0, D*H*W < 2^27; else MD_ERR_UNSUPPORTED (md_gemm_conv
 * with MD_CFG_C3_S2 handles every shape).
 */
int md_conv3_s2(const float* x, const void* wpk, float* out, const float* bias, int64_t bias_bstride, double* stats,
                int32_t batch, int32_t cin, int32_t rows, int32_t rows_alloc, int32_t D, int32_t H, int32_t W, void* stream);

/* md_wino_prep in two phases through LDS (csrc/wino_prep2.hip), bit-identical output, 13 % faster (the host package's default);
 * additionally needs W | 256 and D*H*W % 256 == 0 (whole rows per workgroup), else MD_ERR_UNSUPPORTED. */
int md_wino_prep_v2(const float* x1, const float* x2, int32_t c1, int32_t c2, const float* ac, int32_t silu, int32_t ups,
                    void* t_out, int32_t batch, int32_t D, int32_t H, int32_t W, float drop_p, uint64_t drop_seed, void* stream);

/* md_wino_prep_v2 with a second output u_out in the layout of T: per output pair (x = 2i, 2i+1) of the (activated) tensor
 * v the four values (v[2i], v[2i] + v[2i+1], v[2i] - v[2i+1], v[2i+1]), hi / lo bf16 planes -- the dY operand of
 * md_wgrad_wino when the tensor is an output gradient (training backward: one pass over dY feeds both the Winograd data
 * gradient conv, T, and the Winograd weight gradient, U).  sums (optional, float [B][c1 + c2], accumulated with atomics, not
 * with ups): += per-(sample, channel) sums of the activated tensor over the grid -- the bias gradient of the same pass.
 * Same shape restrictions as md_wino_prep_v2. */
int md_wino_prep_dual(const float* x1, const float* x2, int32_t c1, int32_t c2, const float* ac, int32_t silu, int32_t ups,
                      void* t_out, void* u_out, float* sums, int32_t batch, int32_t D, int32_t H, int32_t W, float drop_p,
                      uint64_t drop_seed, void* stream);

/*
 * md_attn_fwd: fused single-head self-attention (AttnBlock.forward, layers.py:595-608: the two einsums :602,:606 and the
 * softmax :604) -- QK^T, online softmax over the keys and PV in one kernel, bf16x3 MFMA for both contractions; the
 * [B][N][N] score matrix is never materialised.
 *   qk  : S16B [B][2C/8][2][N][8]  q = channels 0..C-1, k = channels C..2C-1 (NIN_0 | NIN_1 outputs, one GEMM)
 *   vT  : S16B over tokens [B][N/8][2][C][8]  (NIN_2 output WITHOUT its bias, token-major)
 *   out : S16B [B][C/8][2][N][8]   o[c][q] = sum_key v[c][key] softmax_key(scale * k[:,key].q[:,q]) + bias_v[c]
 * Supported: C == 256, N % 128 == 0 (the 16^3 attention levels of ddpm_res64); other shapes return MD_ERR_UNSUPPORTED
 * and take the GEMM + md_softmax_keys path.
 */
int md_attn_fwd(const void* qk, const void* vT, void* out, const float* bias_v, int32_t batch, int32_t C,
                int32_t N, float scale, void* stream);

/*
 * One DDPM ancestral-sampling update (models/utils.py:191-198 score scaling,
 * sampling.py:222-230 predictor, sampling.py:476-478 mask), all NCDHW fp32:
 *   x_mean = (x - beta/sigma * eps) / sqrt(1-beta);  x = x_mean + sqrt(beta)*z
 *   x, x_mean *= mask[P]   (mask may be NULL)
 * beta/sigma/… are passed per batch element (coef[b][4] = beta, sigma, sqrt(1-beta), sqrt(beta)).
 * P % 4 == 0; x, eps, z, mask and the outputs 16-byte aligned (coef: 4), else MD_ERR_BAD_ARG.
 */
int md_ancestral_step(const float* x, const float* eps, const float* z, const float* mask,
                      const float* coef, float* x_out, float* x_mean_out, int32_t batch,
                      int32_t C, int64_t P, void* stream);
/*
 * One deterministic DDIM update (sde_lib.py:113-140 `discretize_ddim` + the mask / inpainting lines of
 * `ddim_sampler`, sampling.py:556-565).  State in float64 like the reference:
 *   x0s = x - a2*eps ; x0_pred = x0s/a1 ; x_new = r1*x + (r2-r1)*(x - x0s) ; both *= mask[P] (mask may be NULL);
 *   channel `ch`: v = v*(1-pmask) + partial*pmask when partial/pmask ([P] each) are given.
 * coef[b][4] = {a1 = sqrt(abar_t), a2 = sqrt(1-abar_t), r1 = a1_prev/a1, r2 = a2_prev/a2} as doubles;
 * x_f32 receives float(x_new): the next U-Net input.
 */
int md_ddim_step(const double* x, const float* eps, const float* mask, const double* coef, const float* partial,
                 const float* pmask, int32_t ch, double* x_out, double* x0_out, float* x_f32, int32_t batch,
                 int32_t C, int64_t P, void* stream);
/*
 * Predictor-corrector sampling (ABI 16; sampling.py:185-210 predictors, :259-321 correctors), all NCDHW fp32 [B][C][P],
 * mask [P] binary or NULL, per-sample coefficient rows built by the host with the reference's float32 expressions.
 * Bit-identical to the reference's elementwise torch chains for the same eps / z / coefficient rows.
 *
 * Langevin / ALD corrector step, two launches on one stream, deterministic (no atomics):
 *   md_langevin_norms: slabs[b][s] = {sum eps^2, sum z^2} (fp64) over workgroup s's share of sample b;
 *                      slabs is double[batch][MD_LANGEVIN_SLABS][2]
 *   md_langevin_step : step_b = (snr * mean_b' sqrt(sum z^2) / mean_b' (sqrt(sum eps^2)/sigma_b'))^2 * 2 * alpha_b
 *                      (mode MD_CORRECTOR_LANGEVIN, reduces the slabs of the whole batch in its prologue) or
 *                      step_b = coef[b][2] (mode MD_CORRECTOR_ALD, slabs may be NULL); then with score = -eps/sigma_b
 *                      x_mean = x + step_b*score ; x = x_mean + sqrt(step_b*2)*z ; both *= mask ; step_out[b] = step_b
 *   coef[b][3] = {sigma = sqrt(1-abar_t), alpha = 1-beta_t, (snr*std(t))^2*2*alpha}
 *
 * SDE predictor step, one launch; coef[b][5] = {sigma, c1, c2, c3, c4}, score = -eps/sigma:
 *   MD_SDE_REVERSE_DIFFUSION: x_mean = x - ((c1*x - x) - (c2*score)*c3) ; x = x_mean + c4*z
 *                             c1 = sqrt(alpha), c2 = sqrt(beta)^2, c3 = 1 (0.5 probability flow), c4 = sqrt(beta) (0 p.f.)
 *   MD_SDE_EULER_MARUYAMA   : x_mean = x + (c1*x - c2*score)*c3 ; x = x_mean + c4*z
 *                             c1 = -0.5*beta(t), c2 = sqrt(beta(t))^2, c3 = -1/N, c4 = sqrt(beta(t))*sqrt(1/N)
 *   x, x_mean *= mask
 * P % 4 == 0 for all three; every state-sized tensor, the mask and the slabs 16-byte aligned (coef, step_out: 4), else
 * MD_ERR_BAD_ARG.
 */
#define MD_LANGEVIN_SLABS 64
#define MD_CORRECTOR_LANGEVIN 0
#define MD_CORRECTOR_ALD 1
#define MD_SDE_REVERSE_DIFFUSION 0
#define MD_SDE_EULER_MARUYAMA 1
int md_langevin_norms(const float* eps, const float* z, int32_t batch, int32_t C, int64_t P, double* slabs, void* stream);
int md_langevin_step(const float* x, const float* eps, const float* z, const float* mask, const float* coef,
                     const double* slabs, float snr, int32_t mode, float* x_out, float* x_mean_out, float* step_out,
                     int32_t batch, int32_t C, int64_t P, void* stream);
int md_sde_step(const float* x, const float* eps, const float* z, const float* mask, const float* coef, int32_t kind,
                float* x_out, float* x_mean_out, int32_t batch, int32_t C, int64_t P, void* stream);
/*
 * Right-hand side of the probability-flow ODE of the VP SDE (likelihood.py:63-78 drift_fn / div_fn; one launch):
 *   drift = (c_x*x + c_e*eps_hat) * mask              formed in double, rounded to float once
 *   coef[b][2] = {c_x = -0.5*beta(t), c_e = 0.5*beta(t)/sigma(t)} as doubles (score = -eps_hat/sigma, built by the host)
 * With g (the vector-Jacobian product J^T probe of eps_hat) and probe, both [B][C][P]:
 *   slabs[b][s] = sum over workgroup s's share of sample b of probe*(c_x*probe + c_e*g)*mask    (written, not added to)
 * slabs is double[batch][MD_LANGEVIN_SLABS]; the sum of a sample's slabs is the Hutchinson estimate of the drift's
 * divergence.  Deterministic: fixed grid, fixed order, fp64 partial sums, no atomics.  g and probe are both NULL (drift
 * only: the ODE sampler) or both given, then with slabs; mask [P] binary or NULL.  P % 4 == 0; pointers 16-byte aligned (coef,
 * slabs: 8); anything else MD_ERR_BAD_ARG.  Purely additive: MD_ABI_VERSION stays 16.
 */
int md_pf_ode_rhs(const float* x, const float* eps_hat, const float* g, const float* probe, const float* mask,
                  const double* coef, float* drift, double* slabs, int32_t batch, int32_t C, int64_t P, void* stream);
/*
 * Reconstruction guidance of the conditional samplers (diffusion posterior sampling, Chung et al. 2023): each step also descends
 * the gradient of the measurement error ||r|| of the predicted clean grid on the visible voxels of channel `ch`.  With
 * alpha = sqrt(abar_t), sigma = sqrt(1-abar_t) of the level the step starts from, y the partial grid (src, batch stride
 * src_bstride = 0 or P), pm its visibility mask [P], gm the grid mask [P] or NULL, all NCDHW [B][C][P]:
 *   md_guide_residual : coef[b][2] = {alpha, sigma} as doubles.  x0_hat = (x - sigma*eps_hat)/alpha ;
 *                       cot[ch] = r = (pm*gm)*(x0_hat[ch] - y), formed in double and rounded to float once; every other channel
 *                       of cot is written as +0 (x and eps_hat are read in channel ch only).  slabs[b][s] = sum over workgroup
 *                       s's share of sample b of the squares of the ROUNDED r (written, not added to): the norm belongs to the
 *                       cotangent that the U-Net's backward sees.  slabs is double[batch][MD_LANGEVIN_SLABS].
 *   the caller then forms g = J^T cot, the vector-Jacobian product of eps_hat with respect to x.
 *   md_guide_apply_f32: in place.  coef[b][3] = {alpha, sigma, zeta} as doubles.  n_b = sqrt(slabs[b][0] + slabs[b][1] + ...),
 *                       added in ascending order in double ; k_b = zeta/(alpha*n_b), exactly 0 when n_b == 0 (nothing visible),
 *                       NaN when n_b is NaN.  d = (k_b*(cot - sigma*g))*gm = zeta * d||r||/dx, formed in double and rounded to
 *                       float once ; x = fl(x - d) ; x_mean (may be NULL) likewise from the same d.
 *   md_guide_apply_f64: the same update of the DDIM sampler's float64 state with d kept in double: x64 -= d ;
 *                       x_f32 = float(x64), the next U-Net input.
 * Deterministic: fixed grid, fixed order, fp64 partial sums, no atomics.  P % 4 == 0; pointers 16-byte aligned (coef, slabs: 8);
 * 0 <= ch < C; no output may share memory with an input or with the other output; anything else MD_ERR_BAD_ARG, before any
 * launch.  Purely additive: MD_ABI_VERSION stays 16.
 */
int md_guide_residual(const float* x, const float* eps_hat, const float* src, int64_t src_bstride, const float* pmask,
                      const float* gmask, const double* coef, int32_t ch, float* cot, double* slabs, int32_t batch, int32_t C,
                      int64_t P, void* stream);
int md_guide_apply_f32(float* x, float* x_mean, const float* cot, const float* g, const float* gmask, const double* coef,
                       const double* slabs, int32_t batch, int32_t C, int64_t P, void* stream);
int md_guide_apply_f64(double* x64, float* x_f32, const float* cot, const float* g, const float* gmask, const double* coef,
                       const double* slabs, int32_t batch, int32_t C, int64_t P, void* stream);
/*
 * One update of the multistep exponential integrator in the data prediction (DPM-Solver++, Lu et al. 2022; orders 1-3, the ODE
 * and the SDE variant), one launch.  All tensors NCDHW [B][C][P]; state and history in float64 like md_ddim_step's state.  With
 * coef[b][8] = {alpha_s, sigma_s, c_x, c_0, c_1, c_2, c_z, unused} as doubles (alpha_s, sigma_s: the level the step starts from;
 * the c's formed by the host from the half-log-SNR of the two levels), everything evaluated in double:
 *   x0    = (x - sigma_s*eps)/alpha_s                           the clean-grid prediction of this step
 *   x_new = c_x*x + c_0*x0 + c_1*h1 + c_2*h2 + c_z*z            added left to right; a term whose pointer is NULL is skipped
 *   x_new, x0 *= mask[P]   (mask may be NULL)
 *   channel `ch`: v = v*(1-pmask) + partial*pmask on both when partial/pmask ([P] each) are given: the order of md_ddim_step
 * h1, h2: the x0_out of the previous step and of the one before it (the caller keeps them); z: float32 noise (SDE variant).
 * x_out = x_new ; x0_out = x0 ; x_f32 = (float)x_new, the next U-Net input.  Deterministic: no atomics, no LDS.
 * P % 4 == 0; pointers 16-byte aligned (coef: 8); 0 <= ch < C; partial and pmask both given or both NULL; h2 only with h1; no
 * output may share memory with an input or with another output; anything else MD_ERR_BAD_ARG, before any launch.  Purely
 * additive: MD_ABI_VERSION stays 16.
 */
int md_multistep_step(const double* x, const float* eps, const double* h1, const double* h2, const float* z,
                      const float* mask, const double* coef, const float* partial, const float* pmask, int32_t ch,
                      double* x_out, double* x0_out, float* x_f32, int32_t batch, int32_t C, int64_t P, void* stream);
/*
 * Spherical interpolation between pairs of latents (evaler.py:63-71 `slerp`, the reference's formula evaluated in double; the
 * reference itself runs it in the tensors' float32).  Two launches on one stream, deterministic (no atomics):
 *   a, b : fp32 [pairs][C][P], the two endpoints of each pair;  mask: fp32 [P] binary, shared by pairs and channels, or NULL
 *   md_slerp_dots: slabs[p][s][0..3] = {sum a*b, sum a*a, sum b*b, 0} (fp64 products and sums of the masked values) over
 *                  workgroup s's share of pair p (written, not added to); slabs is double[pairs][MD_LANGEVIN_SLABS][4]
 *   md_slerp_mix : adds pair p's slabs in ascending order in double ; c = sum ab / (sqrt(sum aa)*sqrt(sum bb)) clamped to [-1, 1] ;
 *                  theta = acos(c) ; with alpha double[K] on the device, for every k < K
 *                    w1_k = sin((1-alpha_k) theta)/sin(theta) ; w2_k = sin(alpha_k theta)/sin(theta)
 *                    out[p][k] = float((w1_k*a + w2_k*b)*mask), formed in double and rounded once ; out is fp32 [pairs][K][C][P]
 *                  theta_out (double[pairs], may be NULL) receives theta.  a and b are read once for all K.
 * Endpoints: alpha = 0 gives a*mask and alpha = 1 gives b*mask bit for bit (sin(theta)/sin(theta) is exactly 1, sin(0) exactly 0;
 * no special case).  Degenerate pairs, the one deviation from the reference, which returns NaN there: where
 * (1-c)(1+c) < 2^-40 the endpoints are parallel or antiparallel and the weights are (1-alpha_k, alpha_k), linear interpolation;
 * theta is still reported.  A zero endpoint (sum aa or sum bb = 0) makes the pair NaN, as in the reference.  A non-finite value
 * anywhere in an endpoint makes theta and every output of that pair NaN; other pairs of the launch are not touched by it.
 * The mask multiplies the result, as in md_ddim_step: outside it a finite pair gives (signed) zero, a NaN pair NaN.
 * MD_ERR_BAD_ARG, before any launch: K < 1 or K > MD_SLERP_MAX_K; P % 4 != 0; pairs < 1 or C < 1; a, b or out null or not
 * 16-byte aligned (mask: 16 when given); slabs or alpha null or not 8-byte aligned (theta_out: 8 when given); an output
 * sharing memory with an input or with the other output.  Two runs give the same bits.  Purely additive: MD_ABI_VERSION stays 16.
 */
#define MD_SLERP_MAX_K 256
int md_slerp_dots(const float* a, const float* b, const float* mask, int32_t pairs, int32_t C, int64_t P,
                  double* slabs, void* stream);
int md_slerp_mix(const float* a, const float* b, const float* mask, const double* slabs, const double* alpha, int32_t K,
                 float* out, double* theta_out, int32_t pairs, int32_t C, int64_t P, void* stream);
/*
 * Classifier-free guidance on the output of one doubled U-Net evaluation (the reference has no counterpart; Ho & Salimans 2022,
 * rescale: Lin et al. 2023, section 3.4).  Every sampler consumes the combined eps_hat as it consumes the U-Net's.
 *   eps2: fp32 [2*batch][n]: rows 0..batch-1 the conditional evaluation ec, rows batch..2*batch-1 the null-class evaluation eu
 *   w   : fp32 [batch], the guidance scale of every sample
 *   md_cfg_combine: out[b][i] = fmaf(w[b], ec - eu, eu): one float32 subtraction and one fused multiply-add, round to nearest.
 *                   w = 0 gives eu bit for bit wherever ec - eu is finite; NaN and inf propagate.  One pass over eps2.  With
 *                   slabs given (double[batch][MD_LANGEVIN_SLABS][4]) workgroup s of sample b also writes (not adds)
 *                   slabs[b][s] = {sum ec, sum ec^2, sum out, sum out^2} over its strided share, every term and sum in double
 *                   (the square of a float is exact there), in a fixed order: no atomics, the same bits every run.
 *   md_cfg_rescale: per sample, adds the slabs in ascending order in double; mean = sum/n, var = sum2/n - mean^2 (population,
 *                   over all n values), f = phi*sqrt(var_ec/var_out) + (1 - phi) finished in double; out[b][i] *= (float)f, one
 *                   float32 product.  Where var_out is not > 0 or f is not finite (a constant sample, a non-finite value in either
 *                   tensor) the sample is left as it is and f reads 1.  factor_out (double[batch], may be NULL) receives f.
 * n is any positive count: four values per thread where n % 4 == 0, one value at a time otherwise, the sums in the same order.
 * MD_ERR_BAD_ARG, before any launch: eps2, out null or not 16-byte aligned where n % 4 == 0 (4-byte otherwise); w null or not
 * 4-byte aligned; slabs not 8-byte aligned (md_cfg_rescale: or null), factor_out not 8-byte aligned; batch < 1, n < 1; phi outside
 * [0, 1] or NaN; an output sharing memory with an input or with another output (out may alias neither half of eps2).
 * Purely additive: MD_ABI_VERSION stays 16.
 */
int md_cfg_combine(const float* eps2, const float* w, int32_t batch, int64_t n, float* out, double* slabs, void* stream);
int md_cfg_rescale(float* out, const double* slabs, double phi, double* factor_out, int32_t batch, int64_t n, void* stream);
/*
 * Inpainting blend of one channel (sampling.py:443-467):
 *   v = (x*(1-m) + src*m) * gm     applied in place to channel `ch` of x [B][C][P];
 *   src has batch stride src_bstride (0 = shared partial grid).
 */
int md_inpaint_blend(float* x, const float* src, const float* pmask, const float* gmask,
                     int32_t batch, int32_t C, int32_t ch, int64_t P, int64_t src_bstride,
                     void* stream);

/*
 * Re-noise the conditioned channel to the current level (sampling.py:460-466), in place:
 *   upd = coef[b][0]*x + coef[b][1]*z[b] ; x[ch] = (x[ch]*(1-m) + upd*m)*gm ; x_mean[ch] = x[ch]
 * coef[b] = (exp(log_mean_coeff(t)), std(t)) of VPSDE.marginal_prob (sde_lib.py:210-214);
 * z is [B][P]; x_mean may be NULL.
 */
int md_inpaint_renoise(float* x, float* x_mean, const float* z, const float* pmask,
                       const float* gmask, const float* coef, int32_t batch, int32_t C,
                       int32_t ch, int64_t P, void* stream);

/*
 * Training-step pieces that do not need the U-Net backward (lib/diffusion/losses.py:38-78, models/ema.py:32-51).
 *   md_ddpm_perturb : out = (coef[b][0]*x0 + coef[b][1]*noise) * mask            (losses.py:63-65)
 *   md_masked_sq_err: sums[b] += sum_i (eps_hat-noise)^2 * mask (fp64; zero `sums` first);
 *                     grad (may be NULL) = gscale * 2 (eps_hat-noise) * mask = dLoss/d eps_hat   (losses.py:68-78)
 *   md_grad_sqnorm  : *out += sum g^2 (fp64; zero first)          (clip_grad_norm_, losses.py:48)
 *   md_adam_ema_step: clip by min(1, max_norm/(sqrt(*grad_sqnorm)+1e-6)) (skipped when grad_sqnorm NULL or
 *                     max_norm < 0), torch.optim.Adam update with bias correction for `step` (1-based),
 *                     then ema -= (1-ema_decay)*(ema - p) (ema may be NULL).  One pass over 5 flat arrays.
 *   md_adam_ema_step_d: the same with every hyper-parameter as a double, so that the fp32 scalars are formed as the reference
 *                     forms them: fl(1.0 - beta1), fl(1.0 - beta2), bias corrections from the double betas, EMA rate
 *                     fl(1.0 - ema_decay) (torch.optim.Adam; models/ema.py `update`).  A value that went through a float first
 *                     gives 1 - x up to 2^-24/(1-x) relative off (1.3e-5 for beta2 = 0.999, 1.66e-4 for a decay of 0.9999);
 *                     md_adam_ema_step widens its floats and is exact only for hyper-parameters that are floats.
 *                     Purely additive: MD_ABI_VERSION stays 16, no existing entry point changes.
 */
int md_ddpm_perturb(const float* x0, const float* noise, const float* mask, const float* coef, float* out,
                    int32_t batch, int32_t C, int64_t P, void* stream);
int md_masked_sq_err(const float* eps_hat, const float* noise, const float* mask, double* sums, float* grad,
                     float gscale, int32_t batch, int32_t C, int64_t P, void* stream);
int md_grad_sqnorm(const float* g, int64_t n, double* out, void* stream);
int md_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int32_t step, float ema_decay,
                     const double* grad_sqnorm, float max_norm, void* stream);
int md_adam_ema_step_d(float* p, const float* g, float* m, float* v, float* ema, int64_t n, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int32_t step, double ema_decay,
                       const double* grad_sqnorm, float max_norm, void* stream);

/*
 * Backward-pass support (csrc/backward.hip).  Contractions of the backward re-use md_gemm_conv:
 *   dgrad  = the forward conv kernels on WPK tiles packed from the flipped/transposed weight
 *   wgrad  = split-K GEMM over (position, sample) on PB16 operands, one B-pointer offset per tap
 * PB16: bf16 [guard + (D+2)(H+2)(W+2) + guard][B/8][2][C][8 samples], zero padded.
 *   md_to_pb16      : F32B (mode 0) / S16B (mode 1) -> PB16; up=1 nearest-upsamples a (D/2)^3 source, stuff=1
 *                     places it at odd fine positions (stride-2 conv backward).  Zero-fills `out` first.
 *   md_wgrad_finish : GEMM result [ntap][rows/8][cols_alloc][8] -> dw[row*s_row + col*s_k + (tap0+t)*s_tap] += .
 *   md_gn_bwd_*     : GroupNorm(+SiLU)(+dropout) backward in three streaming passes (see backward.hip); `sums`
 *                     zeroed by the caller; dgamma/dbeta accumulate; (drop_p, drop_seed) as given to md_gn_apply.
 *   md_channel_sums : out[b][c] += sum_p x (bias / FiLM gradients); md_grad_resample: Upsample backward
 *                     (mode 0: sum of the 8 children) and zero-stuffing (mode 1).
 */
int64_t md_pb16_bytes(int32_t batch, int32_t C, int32_t D, int32_t H, int32_t W, int32_t guard, int32_t pad);
int md_to_pb16(const void* src, void* out, int32_t batch, int32_t C, int32_t c_src, int32_t D, int32_t H, int32_t W,
               int32_t guard, int32_t pad, int32_t mode, int32_t up, int32_t stuff, int32_t zsplit, int32_t zhalo,
               void* stream);
               /* channels >= c_src are zero; pad = halo of the grid: 1 (3x3x3, 1x1x1 consumers) or 2 (5x5x5).
                * zsplit in {1,2,4,8}: each sample is cut into zsplit z-slabs of D planes (whole depth D*zsplit) and the
                * slabs become the "samples" of the sample blocks (batch*zsplit virtual samples), so that batches below 8
                * still fill the 8-sample k-groups of md_wgrad; zhalo = 1 (activation operand): z-halo planes hold the
                * neighbouring slab's data, zhalo = 0 (dY operand): they are zero.  md_pb16_bytes / md_wgrad then take
                * batch*zsplit and the slab dims (D, H, W). */
int md_wgrad_finish(const float* g, float* dw, int32_t rows, int32_t cols, int32_t cols_alloc, int32_t ntap,
                    int32_t tap0, int64_t s_row, int64_t s_k, int64_t s_tap, void* stream);
/*
 * md_wgrad: dw[row*s_row + col*s_k + tap*s_tap] += sum_{position, sample} dY[row][pos] * A[col][pos + off(tap)]
 * for the taps of a k^3 convolution, taps = k^3 in {27, 125} (tap = (dz*k+dy)*k+dx, positions on the grid padded by
 * p = k/2), or the single tap of a 1x1x1 layer (taps = 1, p = 1) -- autograd of nn.Conv3d (layers.py:118-124,
 * ddpm_res128.py:90-92,132) / NIN (layers.py:573-582).
 * dy_pb / act_pb: PB16 tensors from md_to_pb16 (pad = p) with a_ch / b_ch channels (multiples of 8) on the same cubic
 * grid (H = W; D may be a z-slab depth, see md_to_pb16) and `guard` >= p((H+2p)^2 + (H+2p) + 1) + 10; rows <= a_ch,
 * cols <= b_ch are the valid co / ci.  bf16x3 MFMA, fp32
 * accumulate; the contraction is split into `ksplit` position ranges whose partial sums live in `workspace`
 * (md_wgrad_workspace_bytes) and are reduced in a fixed order, so results are run-to-run identical.
 */
int64_t md_wgrad_workspace_bytes(int32_t rows, int32_t cols, int32_t taps, int32_t ksplit);
int md_wgrad(const void* dy_pb, const void* act_pb, float* dw, void* workspace, int64_t workspace_bytes, int32_t batch,
             int32_t a_ch, int32_t b_ch, int32_t rows, int32_t cols, int32_t D, int32_t H, int32_t W, int32_t guard,
             int32_t taps, int32_t ksplit, int64_t s_row, int64_t s_k, int64_t s_tap, void* stream);

/*
 * md_wgrad_wino: weight gradient of a 3x3x3 stride-1 convolution in the Winograd F(2,3)-along-w domain (csrc/wgrad_wino.hip;
 * autograd of nn.Conv3d, layers.py:118-124, for the layers whose forward runs through md_conv3_wino):
 *   dw[co*s_row + ci*s_k + ((kd*3+kh)*3+kw)*s_tap] += sum_{sample, position} dY[co][pos] * A[ci][pos + (kd-1, kh-1, kw-1)]
 * from  u_dy  = md_wino_prep_dual's second output for dY            [B][co/8][4][2][D][H][W/2][8 bf16]
 *       t_act = the operand T of the forward convolution (md_wino_prep / _v2 of the activated input, kept from the forward)
 * 4 products per output pair and (kd, kh) instead of 6 (2/3 of md_wgrad's matrix-core work), no PB16 re-layout; bf16x3 MFMA,
 * fp32 accumulate.  co, ci multiples of 128; W in {32, 64} (rows of 16 / 32 pairs), D, H >= 2.  The contraction is split
 * into `ksplit` ranges of (sample, z) planes (1 <= ksplit <= batch * (D - 1)); partial sums live in `workspace`
 * (md_wgrad_wino_workspace_bytes) and are reduced in a fixed order: results are run-to-run identical.
 */
int64_t md_wgrad_wino_workspace_bytes(int32_t co, int32_t ci, int32_t ksplit);
int md_wgrad_wino(const void* u_dy, const void* t_act, float* dw, void* workspace, int64_t workspace_bytes, int32_t batch,
                  int32_t co, int32_t ci, int32_t D, int32_t H, int32_t W, int32_t ksplit, int64_t s_row, int64_t s_k,
                  int64_t s_tap, void* stream);

/*
 * md_wgrad_nin: weight gradient of a 1x1x1 NIN layer (autograd of layers.py:573-582) straight from S16B tensors:
 *   dw[co*s_row + ci*s_k] += sum_{sample, position} dY[co][pos] * x[ci][pos]
 * dy_s16 / x_s16: S16B [B][C/8][2][P][8] (md_gn_apply with norm = 0 of dY / of the layer's input) -- no PB16 re-layout
 * (md_to_pb16 + md_wgrad with taps = 1 remain for the other shapes).  co, ci multiples of 128, P a multiple of 16; the
 * contraction is split into `ksplit` ranges of 16-position elements (1 <= ksplit <= batch * P / 16), reduced in a fixed order.
 */
int64_t md_wgrad_nin_workspace_bytes(int32_t co, int32_t ci, int32_t ksplit);
int md_wgrad_nin(const void* dy_s16, const void* x_s16, float* dw, void* workspace, int64_t workspace_bytes, int32_t batch,
                 int32_t co, int32_t ci, int64_t P, int32_t ksplit, int64_t s_row, int64_t s_k, void* stream);
int md_gn_bwd_stats(const float* x, const float* dy, const float* params, double* sums, int32_t batch, int32_t C,
                    int64_t P, int32_t c_total, int32_t c_off, int32_t dy_ctotal, int32_t silu, float drop_p,
                    uint64_t drop_seed, void* stream);
int md_gn_bwd_finalize(const double* sums, const float* params, const float* gamma, float* coef, float* dgamma,
                       float* dbeta, int32_t batch, int32_t c_total, int32_t groups, int64_t P, void* stream);
int md_gn_bwd_apply(const float* x, const float* dy, const float* params, const float* coef, float* dx, int32_t batch,
                    int32_t C, int64_t P, int32_t c_total, int32_t c_off, int32_t dy_ctotal, int32_t silu,
                    int32_t accumulate, float drop_p, uint64_t drop_seed, const float* residual, float* ch_sums,
                    uint32_t* amax_bits, void* stream);
                    /* amax_bits (ABI 15, may be NULL): zeroed word receiving max |dx| of this call as md_absmax would (the lift of the
                     * f16f6 data-gradient conv that consumes dx: saves that conv's separate md_absmax pass) */
                    /* residual (may be NULL, ignored when accumulate): F32B like dx, dx = residual + gradient (the identity
                     * shortcut of a ResnetBlock without a separate copy); ch_sums (may be NULL): float [B][c_total],
                     * += per-(sample, channel) sum of the gradient written for this part (bias / FiLM gradients). */
int md_channel_sums(const float* x, float* out, int32_t batch, int32_t C, int64_t P, void* stream);
/* S16B blocked transpose: in [B][R/8][2][Cn][8] -> out [B][Cn/8][2][R][8] (attention backward operands). */
int md_s16b_transpose(const void* in, void* out, int32_t batch, int32_t R, int32_t Cn, void* stream);
/* softmax-over-keys backward: ds = split(alpha * P * (dP - sum_keys P*dP)); layouts as md_softmax_keys. */
int md_softmax_keys_bwd(const void* p, const float* dp, void* ds, int32_t batch, int32_t n_keys, int32_t n_q,
                        float alpha, void* stream);
int md_grad_resample(const float* in, float* out, int32_t batch, int32_t C, int32_t Dc, int32_t Hc, int32_t Wc,
                     int32_t mode, int32_t accumulate, void* stream);

/*
 * Marching tetrahedra on a STATIC tet grid (nvdiffrec/lib/geometry/dmtet.py:105-163), n_meshes meshes per call:
 * chunks of 1024 edges / tets per workgroup, four launches on `stream` (chunk totals, per-mesh scan, vertices, faces).
 * Static tables (built once on the host from the tet file, see meshdiffusion_amd/dmtet.py):
 *   tets       int32 [T][4]
 *   edges      int32 [E][2]   lexicographically sorted unique (min,max) vertex pairs of all tets
 *   tet_edges  int32 [T][6]   edge id of each tet's 6 edges in base_tet_edges order (dmtet.py:54)
 * Per mesh:   pos float32 [M][N][3], sdf float32 [M][N]
 * Outputs:    verts float32 [M][E][3] (first counts[m][0] rows valid),
 *             faces int64 [M][2T][3]  (first counts[m][1] rows valid),
 *             face_tet int64 [M][2T]  (tet id of each face = face_to_valid_tet; may be NULL),
 *             counts int32 [M][4] = {n_verts, n_faces, n_tets_1tri, n_tets_2tri}
 * Face order == reference: all 1-triangle tets (tet order), then 2-triangle tets.
 * Workspace:  md_marching_tets_workspace_bytes(M, E, T) bytes (edge -> vertex id table + per-chunk counters).
 * tets must be 16-byte and edges 8-byte aligned (rows are read whole).  n_meshes <= 65535.
 */
int64_t md_marching_tets_workspace_bytes(int32_t n_meshes, int32_t n_edges, int32_t n_tets);
int md_marching_tets(const float* pos, const float* sdf, const int32_t* tets,
                     const int32_t* edges, const int32_t* tet_edges, int32_t n_meshes,
                     int32_t n_verts, int32_t n_edges, int32_t n_tets, float* verts,
                     int64_t* faces, int64_t* face_tet, int32_t* counts, void* workspace,
                     int64_t workspace_bytes, void* stream);
/*
 * Backward of the vertex interpolation of md_marching_tets, and the SDF sign regulariser of dmtet.py:169-175 with its
 * backward.  Purely additive: MD_ABI_VERSION stays 16, no existing entry point changes.
 * Static incidence list of the edge table (CSR over grid vertices, see TetTables.incidence in meshdiffusion_amd/dmtet.py):
 *   inc_ptr int32 [N+1], inc int32 [2E] = 2 * edge id + (0: the vertex is edges[e][0], 1: it is edges[e][1]),
 *   ascending edge id inside a vertex.
 * md_marching_tets_bwd: one launch for all meshes, one thread per (mesh, grid vertex), no atomics (bit-reproducible).
 *   pos, sdf, edges as in md_marching_tets; vid int32 [M][E] = the first M*E words of that call's workspace (edge ->
 *   vertex id or -1); counts int32 [M][4] of that call; grad_verts float32 [M][E][3] (rows >= counts[m][0] are never
 *   read); dpos float32 [M][N][3], dsdf float32 [M][N]: every element is written (zero where no edge crosses).
 * md_sdf_reg_loss: loss = mean bce_with_logits(s0, [s1 > 0]) + mean bce_with_logits(s1, [s0 > 0]) over the edges with
 *   torch.sign(s0) != torch.sign(s1); sdf float32 [N], edges int32 [E][2] (8-byte aligned).  Two launches: fp64 partial
 *   sums and integer counts of MD_SDF_REG_SLABS workgroups at fixed positions of `workspace`
 *   (MD_SDF_REG_WORKSPACE_BYTES, 8-byte aligned), then a fixed-order reduction; loss float32 [1], count int32 [1] stay on
 *   the device.  An empty mask gives loss = nan (the mean of an empty tensor), as the reference does.
 * md_sdf_reg_loss_bwd: dsdf float32 [N] = grad_out[0] / count[0] * d(sum)/dsdf, every element written; exactly 0 at
 *   vertices without a masked edge.  count and grad_out are device pointers.
 */
#define MD_SDF_REG_SLABS 64
#define MD_SDF_REG_WORKSPACE_BYTES (MD_SDF_REG_SLABS * 24)
int md_marching_tets_bwd(const float* pos, const float* sdf, const int32_t* edges, const int32_t* vid,
                         const int32_t* counts, const float* grad_verts, const int32_t* inc_ptr, const int32_t* inc,
                         int32_t n_meshes, int32_t n_verts, int32_t n_edges, float* dpos, float* dsdf, void* stream);
int md_sdf_reg_loss(const float* sdf, const int32_t* edges, int32_t n_verts, int32_t n_edges, void* workspace,
                    float* loss, int32_t* count, void* stream);
int md_sdf_reg_loss_bwd(const float* sdf, const int32_t* edges, const int32_t* inc_ptr, const int32_t* inc,
                        const int32_t* count, const float* grad_out, int32_t n_verts, int32_t n_edges, float* dsdf,
                        void* stream);

/*
 * Smooth vertex normals of an extracted mesh (nvdiffrec/lib/render/mesh.py:200-229 `auto_normals`, called from
 * nvdiffrec/eval.py:422 on the marching-tets output): face normals cross(v1-v0, v2-v0) accumulated on their three
 * vertices, degenerate sums replaced by (0,0,1), normalised.  verts float32 [V][3], faces int64 [F][3] (as returned by
 * md_marching_tets); v_nrm float32 [V][3] (zeroed by the call), f_nrm float32 [F][3] or NULL (unnormalised face normals).
 */
int md_vertex_normals(const float* verts, const int64_t* faces, int64_t n_verts, int64_t n_faces, float* v_nrm,
                      float* f_nrm, void* stream);

/*
 * Point-cloud supervision of the fitting loop (nvdiffrec/lib/geometry/dmtet.py:454-459: sample_points + chamfer_distance;
 * dmtet.py:249-251: nearest other vertex).  Purely additive: MD_ABI_VERSION stays 16.  Batched: `batch` clouds / meshes per
 * call, batch <= 65535 (else MD_ERR_UNSUPPORTED).  The kernels index with the given tables unchecked: the host checks the
 * ranges of faces / neighbour indices once (meshdiffusion_amd/pointcloud.py).
 *
 * md_nn_sided: for every point of p float32 [B][N][3] the squared distance to, and the index of, its nearest point of
 *   q float32 [B][M][3]: dist float32 [B][N], idx int64 [B][N].  Distances in the direct form (px-qx)^2 + (py-qy)^2 +
 *   (pz-qz)^2 in fp32 (multiply-adds may be fused), never the expanded |p|^2 + |q|^2 - 2 p.q.  Ties go to the lowest index.
 *   skip_same_index != 0 excludes q[i] for query i (p == q: the nearest OTHER point).  A NaN distance wins, as in torch.min:
 *   a query with a NaN coordinate gets NaN.  No candidate at all (M == 1 with skip_same_index): dist = +inf, idx = -1.
 *   Two launches (partial minima per chunk of q, then the minimum over chunks of 64-bit (distance, index) keys); no atomics,
 *   bit-identical from run to run.  workspace: md_nn_sided_workspace_bytes(B, N, M) bytes, 8-byte aligned.
 * md_chamfer_bwd: gradient of  L[b] = w1 * mean_i dist(p_i, q_idx_pq(i)) + w2 * mean_j dist(q_j, p_idx_qp(j))  (squared
 *   distances, neighbours held fixed) times grad_out float32 [B] (device): dp float32 [B][N][3], and dq float32 [B][M][3]
 *   unless dq is NULL.  Gathers, no float atomics: (ptr_p int32 [B][N+1], order_p int32 [B][M]) is the CSR of idx_qp -- the
 *   j sorted stably by idx_qp[b][j], ptr_p[b][i] = first position of target i -- and (ptr_q [B][M+1], order_q [B][N]) that of
 *   idx_pq (needed when dq is given).  A negative neighbour index contributes nothing.
 * md_face_areas: areas float32 [B][F] = 0.5 |(v1 - v0) x (v2 - v0)| of verts float32 [B][V][3], faces int64 [F][3] (shared).
 * md_sample_points: S samples per mesh.  Face of sample s: face_choices_in int64 [B][S] if given, else the first f with
 *   cdf[b][f] > r_face[b][s] * cdf[b][F-1], cdf float32 [B][F] = inclusive prefix sum of the areas, which must be
 *   non-decreasing (the host accumulates it with torch.cumsum in float64 and rounds to float32; zero-area faces are never
 *   chosen).  Point: u = sqrt(r_u), w0 = 1 - u, w1 = u (1 - r_v), w2 = u r_v, (w0 v0 + w1 v1) + w2 v2 unfused
 *   (geometry/utils.py:34-45).  r_face, r_u, r_v float32 [B][S] in [0, 1).  Outputs: points float32 [B][S][3], face_choices
 *   int64 [B][S], weights float32 [B][S][3] or NULL.
 * md_sample_points_bwd: dverts float32 [B][V][3] (every element written) = sum over the (sample, corner) pairs naming the
 *   vertex of weights * grad_points; (ptr int32 [B][V+1], order int32 [B][3S]) is the CSR of the codes 3 * sample + corner
 *   sorted stably by faces[face_choices[sample]][corner].  A gather, no atomics.  The face choice is not differentiated.
 */
int64_t md_nn_sided_workspace_bytes(int32_t batch, int32_t n, int32_t m);
int md_nn_sided(const float* p, const float* q, int32_t batch, int32_t n, int32_t m, int32_t skip_same_index,
                float* dist, int64_t* idx, void* workspace, int64_t workspace_bytes, void* stream);
int md_chamfer_bwd(const float* p, const float* q, const int64_t* idx_pq, const int64_t* idx_qp,
                   const int32_t* ptr_p, const int32_t* order_p, const int32_t* ptr_q, const int32_t* order_q,
                   int32_t batch, int32_t n, int32_t m, float w1, float w2, const float* grad_out, float* dp,
                   float* dq, void* stream);
int md_face_areas(const float* verts, const int64_t* faces, int32_t batch, int32_t n_verts, int32_t n_faces,
                  float* areas, void* stream);
int md_sample_points(const float* verts, const int64_t* faces, const float* cdf, const float* r_face,
                     const float* r_u, const float* r_v, const int64_t* face_choices_in, int32_t batch,
                     int32_t n_verts, int32_t n_faces, int32_t n_samples, float* points, int64_t* face_choices,
                     float* weights, void* stream);
int md_sample_points_bwd(const float* grad_points, const float* weights, const int32_t* ptr, const int32_t* order,
                         int32_t batch, int32_t n_verts, int32_t n_samples, float* dverts, void* stream);

/*
 * Depth and silhouette rasteriser of the fitting loop (nvdiffrec/lib/render/render.py:287-329: dr.DepthPeeler, two layers, +
 * dr.interpolate(v_pos) + the distance to the camera), csrc/raster.hip.  Purely additive: MD_ABI_VERSION stays 16.
 *
 * The rasterisation contract
 *   pos_clip float32 [B][V][4] = (x, y, z, w) (16-byte aligned), faces int64 [F][3] shared by the views, resolution (H, W) with
 *   H, W <= 2048, F < 2^24, B <= 64: anything else MD_ERR_UNSUPPORTED.  The kernels index with `faces` unchecked: the host checks
 *   the range once (meshdiffusion_amd/render.py).
 *   Snap: X = rint(((x / w) * 0.5 + 0.5) * (256 W)), Y likewise with H, zw = z / w; every fp32 operation rounded on its own
 *   (correctly rounded divide, no contraction); X, Y clamped to +-2^22.
 *   Skipped: a triangle with a vertex of w <= 0 or a non-finite coordinate (no clipping), or with integer doubled area
 *   A2 = (X1-X0)(Y2-Y0) - (X2-X0)(Y1-Y0) == 0.  No back-face culling.
 *   Coverage (exact integers): pixel (row i, column j) has the centre Q = (256 j + 128, 256 i + 128), row 0 is y = -1.  With the
 *   triangle oriented so that A2 > 0, edge a -> b (d = b - a) has e = d.x (Q.y - a.y) - d.y (Q.x - a.x); covered iff all three
 *   e >= 0, where e == 0 counts only if d.y < 0 or (d.y == 0 and d.x > 0).
 *   Fragment depth: zf = sum_k (e_k / A2) zw_k in fp32 (e_k opposite vertex k); fragments with zf outside [-1, 1] are dropped.
 *   Layers: by the key (zf, face index); layer 1 the smallest, layer 2 the second smallest; independent of the visiting order.
 *   rast float32 [B][H][W][4] per layer: (u, v, zf, face index + 1), zeros where uncovered.  u, v: perspective-correct from the
 *   unsnapped clip floats -- fx = (2j+1)/W - 1, fy = (2i+1)/H - 1, p_k = (x_k - fx w_k, y_k - fy w_k), a0 = p1 x p2, a1 = p2 x p0,
 *   a2 = p0 x p1, u = a0 / (a0+a1+a2), v = a1 / (a0+a1+a2), not clamped; an attribute is u A0 + v A1 + (1-u-v) A2.
 *   Depth buffers: gb_pos = that interpolation of the world vertices, depth = |gb_pos - campos|; uncovered: 20.0 (layer 1),
 *   -1.0 (layer 2); mask = 1.0 where covered.
 *   Gradient of both depth layers w.r.t. verts, ids fixed, through the attribute path AND the barycentric path (u, v <- pos_clip
 *   <- verts through mvp); none for mvp / campos.
 *
 * md_raster_bin_count: counts int32 [B][F] = the 16x16-pixel tiles the bounding box of face f touches in view b (0: skipped or
 *   off screen).
 * md_raster_bin_emit: offsets int64 [B][F] = the exclusive prefix sum of counts, total = their sum (> 2^31 - 1:
 *   MD_ERR_UNSUPPORTED); writes pair_tile int32 [total] = (b * tiles_y + ty) * tiles_x + tx and pair_face int32 [total].
 * md_raster_tiles: tile_ptr int32 [B * tiles_y * tiles_x + 1], tile_faces int32 [total]: the pairs sorted by tile (CSR); writes
 *   every element of rast1, rast2.
 * md_raster_depth: verts float32 [V][3] (world space, shared by the views), campos float32 [B][3]; depth1/2, mask1/2 float32
 *   [B][H][W].
 * md_raster_depth_bwd: cov int32 [n_cov] = (b * 2 + layer) * H W + pixel of the covered entries (3 n_cov < 2^31), gd1 / gd2
 *   float32 [B][H][W] = d L / d depth, mvp float32 [B][4][4] row-major (pos_clip = mvp (P, 1)); corner_grad float32 [n_cov][3][3]
 *   workspace; (ptr int32 [V+1], order int32 [3 n_cov]) the CSR of the codes 3 * entry + corner sorted stably by
 *   faces[id][corner]; dverts float32 [V][3], every element written.  A gather: no float atomics, bit-reproducible.
 */
int md_raster_bin_count(const float* pos_clip, const int64_t* faces, int32_t batch, int32_t n_verts, int32_t n_faces,
                        int32_t H, int32_t W, int32_t* counts, void* stream);
int md_raster_bin_emit(const float* pos_clip, const int64_t* faces, const int64_t* offsets, int32_t batch, int32_t n_verts,
                       int32_t n_faces, int32_t H, int32_t W, int64_t total, int32_t* pair_tile, int32_t* pair_face,
                       void* stream);
int md_raster_tiles(const float* pos_clip, const int64_t* faces, const int32_t* tile_ptr, const int32_t* tile_faces,
                    int32_t batch, int32_t n_verts, int32_t n_faces, int32_t H, int32_t W, float* rast1, float* rast2,
                    void* stream);
int md_raster_depth(const float* rast1, const float* rast2, const float* verts, const int64_t* faces, const float* campos,
                    int32_t batch, int32_t n_verts, int32_t n_faces, int32_t H, int32_t W, float* depth1, float* depth2,
                    float* mask1, float* mask2, void* stream);
int md_raster_depth_bwd(const int32_t* cov, int32_t n_cov, const float* rast1, const float* rast2, const float* gd1,
                        const float* gd2, const float* pos_clip, const float* verts, const int64_t* faces, const float* mvp,
                        const float* campos, const int32_t* ptr, const int32_t* order, int32_t batch, int32_t n_verts,
                        int32_t n_faces, int32_t H, int32_t W, float* corner_grad, float* dverts, void* stream);

/*
 * Silhouette antialiasing of the fitting loop, in the manner of nvdiffrast's dr.antialias (nvdiffrec/lib/render/render.py:256-276),
 * not equal to it; csrc/antialias.hip.  Purely additive: MD_ABI_VERSION stays 16.
 *
 * The antialiasing contract
 *   color float32 [B][H][W][C], 1 <= C <= 8; rast float32 [B][H][W][4], one layer of the rasterisation contract: (u, v, zf,
 *   face + 1), zeros where uncovered; pos_clip float32 [B][V][4]; faces int64 [F][3]; nbr int32 [F][3].  The limits on B, H, W, F
 *   are those of the rasterisation contract, anything else MD_ERR_UNSUPPORTED; null or misaligned pointers and non-positive
 *   sizes MD_ERR_BAD_ARG.  A rast id outside [0, F] makes every pair it takes part in inactive; it is never an index.
 *   Neighbours: nbr[f][k] belongs to the edge opposite corner k of face f (vertices faces[f][(k+1)%3], faces[f][(k+2)%3], as an
 *   unordered pair): the other face's opposite vertex if exactly two face corners of the mesh own that pair, else -1.
 *   Pairs: every pixel with its right neighbour and with the pixel below it, inside the image.  Ids t0, t1, depths z0, z1 of the
 *   first / second pixel: a candidate iff t0 != t1; the owning pixel P is the second if t0 == 0, the first if t1 == 0, otherwise
 *   the first iff z0 < z1 (fp32 compare of the stored values); Q the other, T = P's triangle, s = +1 if Q follows P, else -1.
 *   A triangle T with a vertex of w <= 0 or a non-finite coordinate has no edge.
 *   Decisions (exact integers; snapped X, Y of the rasterisation contract, P's centre (Px, Py) = (256 j + 128, 256 i + 128)):
 *   the edges of T in the order k = 0, 1, 2 (a = faces[T][(k+1)%3] -> b = faces[T][(k+2)%3], opposite corner o); the first that
 *   passes all of the following is the pair's edge, without one the pair is inactive.
 *     Silhouette: nbr < 0, or the neighbour vertex o' has w <= 0 or a non-finite coordinate, or
 *       sign(cross(b-a, o-a)) sign(cross(b-a, o'-a)) >= 0 (int64).
 *     Orientation: |Yb-Ya| >= |Xb-Xa| for a horizontal pair, |Xb-Xa| >= |Yb-Ya| for a vertical one.
 *     Crossing: u = s (X - Px), v = Y - Py (X, Y swapped for a vertical pair): (va > 0) != (vb > 0), and with den = vb - va,
 *       n = ua den - va (ub - ua): 0 <= n sign(den) <= 256 |den|.
 *   Value (fp32, every operation rounded on its own, correctly rounded divide, no contraction; unsnapped floats, pixels relative
 *   to P's centre): fu = s ((x / w - fx_P) W/2), fv = (y / w - fy_P) H/2 (roles swapped for a vertical pair);
 *   t = clamp(fu_a - fv_a (fu_b - fu_a) / (fv_b - fv_a), 0, 1), a zero denominator makes the pair inactive; w = t - 0.5;
 *   w >= 0: out[Q] += w (color[P] - color[Q]), else out[P] += (-w) (color[Q] - color[P]).  A pixel's result is
 *   color + right pair + pair below + left pair + pair above, summed in that order.
 *   Gradient: color (the operator is linear in it) and pos_clip (through t: x, y, w of the edge's two vertices, no z; zero where
 *   the clamp is active).  No floating-point atomics: bit-reproducible.
 *
 * md_mesh_edge_neighbours: sorted_keys int64 [3 F] = the keys min(a, b) * V + max(a, b) of the corners f * 3 + k sorted stably,
 *   order int64 [3 F] = the corner of each sorted entry; writes every element of nbr.
 * md_antialias_pairs: writes pairs int32 [B][H][W][2][4] (16-byte aligned): per pixel the record of its right pair and of the
 *   pair below, (va, vb, the bits of the float w, P is the first pixel); va = vb = -1 where inactive or outside the image.
 * md_antialias_blend: out float32 [B][H][W][C], every element written.
 * md_antialias_bwd_color: grad_out float32 [B][H][W][C] -> dcolor, every element written.
 * md_antialias_bwd_pos: active int64 [n_active] = the flat indices ((b H + i) W + j) * 2 + direction of the active pairs
 *   (2 n_active < 2^31, B V < 2^31 - 1); vert_grad float32 [n_active][2][3] workspace; (ptr int32 [B V + 1], order int32
 *   [2 n_active]) the CSR of the codes 2 * entry + end sorted stably by b V + vertex; dpos_clip float32 [B][V][4] (16-byte
 *   aligned), every element written, z component 0.
 */
int md_mesh_edge_neighbours(const int64_t* sorted_keys, const int64_t* order, const int64_t* faces, int32_t n_faces, int32_t* nbr,
                            void* stream);
int md_antialias_pairs(const float* rast, const float* pos_clip, const int64_t* faces, const int32_t* nbr, int32_t batch,
                       int32_t n_verts, int32_t n_faces, int32_t H, int32_t W, int32_t* pairs, void* stream);
int md_antialias_blend(const float* color, const int32_t* pairs, int32_t batch, int32_t H, int32_t W, int32_t C, float* out,
                       void* stream);
int md_antialias_bwd_color(const float* grad_out, const int32_t* pairs, int32_t batch, int32_t H, int32_t W, int32_t C,
                           float* dcolor, void* stream);
int md_antialias_bwd_pos(const int64_t* active, int32_t n_active, const float* color, const float* grad_out, const int32_t* pairs,
                         const float* pos_clip, const int32_t* ptr, const int32_t* order, int32_t batch, int32_t n_verts, int32_t H,
                         int32_t W, int32_t C, float* vert_grad, float* dpos_clip, void* stream);

/* ---- attribute interpolation, barycentric gradients, differentiable vertex normals (csrc/interp.hip) ----
 * THE INTERPOLATION CONTRACT (the header comment of csrc/interp.hip has it in full; tests/interp_cases.py restates it)
 *   rast float32 [B][H][W][4] one layer of the rasteriser (16-byte aligned); attr float32 [Ba][N][C], Ba = 1 or B, 1 <= C <= 8;
 *   tri int64 [F][3] with indices into N (8-byte aligned; tri[f] = (f, f, f), N = F for face-constant attributes).  The limits on
 *   B, H, W, F are those of the rasterisation contract, anything else is MD_ERR_UNSUPPORTED.
 *   Value: a pixel with 1 <= id = rast.w <= F gets out[c] = (u A0[c] + v A1[c]) + t A2[c], t = (1 - u) - v, A_k =
 *   attr[tri[id-1][k]]; every other pixel gets zeros; an id above F is never an index.
 *   d attr: w_k g of corner k of every covered pixel, summed per destination row in ascending order of the code 3 * entry +
 *   corner (entry: the rank of the pixel among the covered pixels in flat (b, i, j) order; Ba == 1 sums over the views).
 *   d rast: du = sum_c g[c] (A0[c] - A2[c]), dv = sum_c g[c] (A1[c] - A2[c]) in channels 0, 1; everything else zero.
 *   Barycentric backward: (du, dv) -> d pos_clip by the formulas of md_raster_depth_bwd, gathered per (view, vertex) in
 *   ascending code order; z gets none.  No floating-point atomics anywhere: bit-reproducible.
 *   Sums: every sum over codes of this contract (d attr, d pos_clip, the vertex normals' s_v, d verts) is a compensated (Kahan)
 *   fp32 sum in ascending code order, every operation rounded on its own and none contracted: sum = 0, lost = 0; per term x:
 *   y = x - lost, t = sum + y, lost = (t - sum) - y, sum = t.  The result is `sum`.
 *
 * md_interpolate: out float32 [B][H][W][C], every element written.
 * md_interpolate_bwd: cov int32 [n_cov] = the flat pixel indices (b H + i) W + j of the covered pixels, ascending (3 n_cov <
 *   2^31, Ba N < 2^31 - 1); corner_grad float32 [n_cov][3][C] workspace; (ptr int32 [Ba N + 1], order int32 [3 n_cov]) the CSR of
 *   the codes sorted stably by (Ba == 1 ? 0 : b) N + tri[id-1][corner]; dattr float32 [Ba][N][C] and drast float32 [B][H][W][4]
 *   (16-byte aligned) are each written in full when not null; one of them may be null, and its launch or store is skipped.
 * md_raster_bary_bwd: drast float32 [B][H][W][4] holding (du, dv) in channels 0, 1; corner_grad float32 [n_cov][3][3]
 *   workspace receiving (d x, d y, d w); (ptr int32 [B V + 1], order int32 [3 n_cov]) the CSR of the codes sorted stably by
 *   b V + faces[id-1][corner]; dpos_clip float32 [B][V][4] (16-byte aligned), every element written, z component 0.
 * md_vertex_normals_det: fn_f = cross(v1 - v0, v2 - v0) -> f_nrm float32 [F][3]; s_v = the sum of fn_f over the corners that name
 *   v in ascending order of the code 3 f + k, over (ptr int32 [V + 1], order int32 [3 F]), the CSR of the codes sorted stably by
 *   vertex; s_v . s_v <= 1e-20 replaces s_v by (0, 0, 1); v_nrm = s_v / sqrt(max(s_v . s_v, 1e-20)); v_len float32 [V] =
 *   that square root, 0 for a replaced vertex.
 * md_vertex_normals_bwd: d s_v = (g - n (n . g)) / |s_v| (zero for a replaced vertex), d fn_f = its sum over the face's corners,
 *   d a = b x d fn, d b = d fn x a for a = v1 - v0, b = v2 - v0; face_grad float32 [F][3][3] workspace; dverts float32 [V][3],
 *   every element written, gathered over the same CSR.
 */
int md_interpolate(const float* rast, const float* attr, const int64_t* tri, int32_t batch, int32_t attr_batch, int32_t n_rows,
                   int32_t C, int32_t n_faces, int32_t H, int32_t W, float* out, void* stream);
int md_interpolate_bwd(const int32_t* cov, int32_t n_cov, const float* rast, const float* grad_out, const float* attr,
                       const int64_t* tri, const int32_t* ptr, const int32_t* order, int32_t batch, int32_t attr_batch,
                       int32_t n_rows, int32_t C, int32_t n_faces, int32_t H, int32_t W, float* corner_grad, float* dattr,
                       float* drast, void* stream);
int md_raster_bary_bwd(const int32_t* cov, int32_t n_cov, const float* rast, const float* drast, const float* pos_clip,
                       const int64_t* faces, const int32_t* ptr, const int32_t* order, int32_t batch, int32_t n_verts,
                       int32_t n_faces, int32_t H, int32_t W, float* corner_grad, float* dpos_clip, void* stream);
int md_vertex_normals_det(const float* verts, const int64_t* faces, const int32_t* ptr, const int32_t* order, int32_t n_verts,
                          int32_t n_faces, float* v_nrm, float* f_nrm, float* v_len, void* stream);
int md_vertex_normals_bwd(const float* verts, const int64_t* faces, const int32_t* ptr, const int32_t* order, const float* v_nrm,
                          const float* v_len, const float* grad_v_nrm, int32_t n_verts, int32_t n_faces, float* face_grad,
                          float* dverts, void* stream);

/*
 * The fixed-topology second pass of the DMTet fit (nvdiffrec/fit_dmtets.py:758-793, dmtet_fixedtopo.py:176-288, regularizer.py:
 * 41-60), csrc/fixedtopo.hip.  Purely additive: MD_ABI_VERSION stays 16, no existing entry point changes.
 *
 * THE FIXED-TOPOLOGY CONTRACT (the header comment of csrc/fixedtopo.hip has it in full; tests/fixedtopo_cases.py restates it)
 *   Plan: edge int32 [Vm][2] (8-byte aligned) = the grid endpoints (a, b) of mesh vertex i, the crossing edges of the sorted edge
 *   table in ascending edge id (md_marching_tets's numbering); grid-vertex CSR ptr int32 [N+1], inc int32 [2 Vm] of the codes
 *   2 * mesh vertex + endpoint, ascending inside a grid vertex; face-corner CSR ptr int32 [V+1], order int32 [3 F] of the codes
 *   3 f + k sorted stably by vertex (that of md_vertex_normals_det).  An index outside its table is skipped, never read.
 *   Sizes are int64: non-positive MD_ERR_BAD_ARG; N, V, 2 Vm beyond int32 or F >= 2^24 MD_ERR_UNSUPPORTED; null or misaligned
 *   pointers MD_ERR_BAD_ARG.  fp32, no contraction, no floating-point atomics: two runs agree bit for bit.
 * md_fixedtopo_verts: verts float32 [Vm][3] = pos[a] * (-sb / den) + pos[b] * (sa / den), den = sa - sb, the expressions of
 *   md_marching_tets in its order: bit-equal to it on the same pos float32 [N][3], sdf float32 [N].
 * md_fixedtopo_verts_bwd: dpos float32 [N][3] = per grid vertex the plain fp32 sum, in ascending code order, of grad_verts[i] * the
 *   forward's weight: bit-equal to the dpos of md_marching_tets_bwd; zeros where a vertex has no codes.  No gradient for sdf.
 * md_laplace_umbrella: y = x - base (base may be NULL); term float32 [V][3] = the compensated sum over the corners (f, k) of v, in
 *   ascending code order, of (y[f[(k+1)%3]] - y_v) + (y[f[(k+2)%3]] - y_v), divided by max(2 corners, 1); loss float32 [1] =
 *   mean(term^2) over 3 V from fp64 partial sums at MD_LAPLACE_SLABS fixed slabs of `workspace` (MD_LAPLACE_WORKSPACE_BYTES,
 *   8-byte aligned) added by one wave in a fixed order; it stays on the device.
 * md_laplace_umbrella_bwd: q float32 [V][3] workspace = ((2 / (3 V)) grad_out[0]) * term / max(2 corners, 1); dx float32 [V][3] =
 *   the compensated sum over the corners of v of (q[f[(k+1)%3]] + q[f[(k+2)%3]]) - 2 q_v, every element written, exactly 0 for a
 *   vertex no face names.  grad_out is a device pointer.
 */
#define MD_LAPLACE_SLABS 64
#define MD_LAPLACE_WORKSPACE_BYTES (MD_LAPLACE_SLABS * 8)
int md_fixedtopo_verts(const float* pos, const float* sdf, const int32_t* edge, int64_t n_verts, int64_t n_mesh_verts, float* verts,
                       void* stream);
int md_fixedtopo_verts_bwd(const float* grad_verts, const float* sdf, const int32_t* edge, const int32_t* ptr, const int32_t* inc,
                           int64_t n_verts, int64_t n_mesh_verts, float* dpos, void* stream);
int md_laplace_umbrella(const float* x, const float* base, const int64_t* faces, const int32_t* ptr, const int32_t* order,
                        int64_t n_verts, int64_t n_faces, float* term, void* workspace, float* loss, void* stream);
int md_laplace_umbrella_bwd(const float* term, const int64_t* faces, const int32_t* ptr, const int32_t* order, const float* grad_out,
                            int64_t n_verts, int64_t n_faces, float* q, float* dx, void* stream);

/*
 * Visible-tet labelling of the single-view fit (nvdiffrec/lib/render/render.py:346-407 with get_visible_tets, fit_singleview.py:
 * 795-820), csrc/visibility.hip.  Purely additive: MD_ABI_VERSION stays 16, no existing entry point changes.
 *
 * THE VISIBILITY CONTRACT (the header comment of csrc/visibility.hip has it in full; tests/visibility_cases.py restates it)
 *   rast float32 [B][H][W][4] (16-byte aligned) is layer 1 of the rasterisation contract.  D = zf where the id is not 0, else 100.
 *   Dmin = the minimum of D over the (2 r + 1)^2 window clipped to the image, 0 <= r <= 15.  A tet centre p is projected as
 *   c = mvp (p, 1) (products summed left to right), n = c.xyz / c.w, q_k = rint((n_k / 2 + 0.5) * S_k), S = (W-1, H-1, H-1), each
 *   fp32 operation rounded on its own; it is valid iff every q_k lies in [0, S_k] (compared in float), c is finite and c.w > 0, and
 *   visible iff valid and (Dmin[q_y][q_x] >= n.z or Dmin[q_y][q_x] == 100).  1 <= B <= 64, 1 <= H, W <= 2048, r > 15:
 *   MD_ERR_UNSUPPORTED beyond; counts are int64, non-positive MD_ERR_BAD_ARG, beyond int32 (faces: 2^24) MD_ERR_UNSUPPORTED; null or
 *   misaligned pointers MD_ERR_BAD_ARG.  No atomics: every label store writes the same value, two runs agree bit for bit.
 * md_window_min: dmin float32 [B][H][W].
 * md_tet_visibility: visible uint8 [B][T] (0 / 1) from dmin, centres float32 [T][3], mvp float32 [B][4][4]; every element written.
 * md_rast_mark_tets: rast_tet uint8 [T], zeroed by the caller: 1 where a pixel has 1 <= id <= F and face_tet[id - 1] (int64 [F]) is
 *   this tet; ids above F and tets outside [0, T) are skipped.
 * md_tets_mark_verts: vis float32 [N] and vis_rast uint8 [N], zeroed by the caller: vis[v] = 1.0 where a tet visible in any of the
 *   `batch` views names v (indices int64 [T][4]), vis_rast[v] = 1 where such a tet or one with rast_tet[t] != 0 does (rast_tet may be
 *   NULL: none); vertices outside [0, N) are skipped.
 */
int md_window_min(const float* rast, int32_t batch, int32_t H, int32_t W, int32_t radius, float* dmin, void* stream);
int md_tet_visibility(const float* dmin, const float* centres, const float* mvp, int32_t batch, int64_t n_tets, int32_t H, int32_t W,
                      uint8_t* visible, void* stream);
int md_rast_mark_tets(const float* rast, const int64_t* face_tet, int32_t batch, int32_t H, int32_t W, int64_t n_faces,
                      int64_t n_tets, uint8_t* rast_tet, void* stream);
int md_tets_mark_verts(const uint8_t* visible, const uint8_t* rast_tet, const int64_t* indices, int32_t batch, int64_t n_tets,
                       int64_t n_verts, float* vis, uint8_t* vis_rast, void* stream);

/*
 * Generation metrics (MMD / COV / 1-NNA under the chamfer distance), csrc/shape_metrics.hip: the all-pairs matrix of sided mean
 * squared distances between two sets of point clouds.  The reference has no counterpart.  Purely additive: MD_ABI_VERSION stays
 * 16, no existing entry point changes.
 *
 * md_sided_mean_matrix: x float32 [nx][p][3], y float32 [ny][q][3] -> out float32 [nx][ny] (every element written),
 *     out[i][j] = (1/p) * sum_a min_b |x[i][a] - y[j][b]|^2.
 *   The chamfer distance of a pair is out_xy[i][j] + out_yx[j][i]; x == y is allowed (the union matrix of one set is S + S^T).
 *   Arithmetic as md_nn_sided: distances in the direct form dz*dz + (dy*dy + dx*dx) in fp32 (never the expanded form, no
 *   matrix-core instruction); the per-point minima are summed in float64 in a fixed order (lane, wave, workgroup), divided by p
 *   and rounded once to fp32.  No atomics, no workspace, one launch; the result does not depend on how the launch is cut up and
 *   two runs agree bit for bit.  Non-finite coordinates: out[i][j] is torch's d2.min(dim=1).values.mean() on the direct-form fp32
 *   distances (a NaN distance, inf - inf included, wins its row's minimum and makes the mean NaN).
 *   Null pointers or sizes < 1: MD_ERR_BAD_ARG.  nx is the x dimension of a grid of 256-lane workgroups, whose threads along x must
 *   stay below 2^32: nx >= 2^24 is MD_ERR_UNSUPPORTED.  The runs of y clouds per x cloud (at most 2048) are its y dimension.
 */
int md_sided_mean_matrix(const float* x, const float* y, int32_t nx, int32_t ny, int32_t p, int32_t q, float* out, void* stream);

/*
 * Generation metrics under the earth mover's distance, csrc/emd.hip: the all-pairs matrix
 *     out[i][j] = (1/p) * min over permutations pi of sum_k |x[i][k] - y[j][pi(k)]|        (Euclidean distance, not its square)
 * of two sets of clouds of the same size p.  The reference has no counterpart.  Purely additive: MD_ABI_VERSION stays 16.
 *
 * THE EMD CONTRACT (the header comment of csrc/emd.hip has it in full; tests/emd_cases.py restates it and derives the bars)
 *   Distance: fp32, direct form sqrtf(dz*dz + (dy*dy + dx*dx)), no contraction, correctly rounded square root.
 *   Integer:  q = rint(d / quantum); quantum is a positive power of two, one per call, so the entries of a matrix are comparable.
 *   Solver:   the integer assignment problem on q is solved exactly, by a forward Jacobi auction with eps-scaling on the costs
 *             q (p + 1) whose last phase runs at eps = 1; prices and bids are 64-bit integers.  Ties for a bidder's best object go to
 *             the lowest index, an object takes its highest bid, ties to the lowest bidder.
 *   Output:   out = (float)((double)total * quantum / p), total the optimal integer cost -- unique where the assignment is not, so
 *             out depends neither on the bidding order nor on the launch, two runs agree bit for bit, and
 *             md_emd_matrix(x, y)[i][j] == md_emd_matrix(y, x)[j][i] bit for bit.
 *   status[i][j]: 0 solved; 1 the pair reached max_rounds bidding rounds (out NaN, total -1, perm -1; the other pairs of the launch
 *             are unaffected); 2 some d / quantum >= 2^21: the quantum is too small for the data (NaN likewise); 3 a NaN or infinite
 *             coordinate in either cloud (NaN, no bidding).
 *   triangular != 0 (needs x == y and nx == ny): only the pairs i < j are solved and written to [i][j] and [j][i] (perm[j][i] is the
 *             inverse permutation); the diagonal is exactly 0 with status 0 and the identity (a non-finite cloud: status 3 there too).
 *   total, rounds (bidding rounds run) and perm (perm[i][j][k] = the point of y[j] matched to point k of x[i]) may be null.
 *   One workgroup per pair, both clouds in LDS: p <= 2048, nx * ny < 2^31 and 2^-126 <= quantum <= 2^126, else MD_ERR_UNSUPPORTED.
 *   Null x, y, out or status, sizes < 1, max_rounds < 1, a quantum that is not a positive finite power of two, triangular with
 *   x != y or nx != ny: MD_ERR_BAD_ARG.
 */
int md_emd_matrix(const float* x, const float* y, int32_t nx, int32_t ny, int32_t p, float quantum, int32_t max_rounds,
                  int32_t triangular, float* out, int32_t* status, int64_t* total, int32_t* rounds, int32_t* perm, void* stream);

/*
 * Post-processing of generated meshes (the tail of nvdiffrec/eval.py:421-456: a diffuse quick-look image and a clean-up), csrc/
 * meshpost.hip.  In the manner of that tail, not bit-equal to MeshLab or nvdiffrast.  Purely additive: MD_ABI_VERSION stays 16, no
 * existing entry point changes.
 *
 * THE MESH POST-PROCESSING CONTRACT (the header comment of csrc/meshpost.hip has it in full; tests/meshpost_cases.py restates it)
 *   A mesh batch is concatenated: verts float32 [V][3], faces int64 [F][3] (8-byte aligned) of global vertex ids; meshes laid end to
 *   end share no edge, so no entry point needs their number.  fp32, no contraction, no floating-point atomics (integer atomicMin /
 *   atomicAdd only): two runs agree bit for bit.  Null or misaligned pointers and non-positive sizes MD_ERR_BAD_ARG; V, 2 V (smoothing:
 *   the codes), n_codes or 3 F beyond int32 MD_ERR_UNSUPPORTED.  An index outside its table is absent, never read.  Nothing is
 *   allocated: the caller passes the scratch.
 * md_mesh_smooth: ptr int32 [V+1], adj int32 [n_codes = 2 E] is the neighbour CSR of the undirected edge table, codes
 *   2 * neighbour + (1 if the edge belongs to exactly one face), ascending inside a row.  `steps` >= 0 umbrella steps, step i with
 *   w = lam (i even, or mu NaN = unset) or mu (Taubin): a vertex whose row holds a boundary code keeps only the boundary codes; n
 *   codes left: n == 0 keeps the vertex's bits, else x' = x + w (s / (float)n - x), s the compensated sum of the neighbours in row
 *   order.  One launch per step, all issued by this call; `verts` is never written and may alias neither `out` nor `scratch`
 *   (float32 [V][3], needed for steps >= 2); the result is in `out`; steps == 0 copies.  lam not finite, mu neither finite nor NaN:
 *   MD_ERR_BAD_ARG.
 * md_mesh_components: label int32 [V] = the smallest vertex index connected to v through faces (a degenerate face connects too, a
 *   vertex no face names is its own component), by hook-and-compress rounds (one thread per face atomicMin's the smallest of its
 *   three roots into the other two, one thread per vertex compresses) until a round lowers no label; `workspace`
 *   (MD_MESH_COMPONENTS_WORKSPACE_BYTES, 4-byte aligned) holds the device flag, read with one 4-byte copy per round, so the call
 *   synchronises the stream.  More than MD_MESHPOST_MAX_ROUNDS rounds: MD_ERR_UNSUPPORTED, never an unbounded loop.  comp_faces int32
 *   [V]: at index label the number of faces whose first vertex carries it, 0 elsewhere.  *rounds (host, may be NULL) = the rounds run.
 * md_shade_diffuse: rast float32 [B][H][W][4] (16-byte aligned) one layer of the rasterisation contract, campos float32 [B][3], sh
 *   float32 [9][3] radiance coefficients in the real spherical harmonics of bands 0-2, kd float32 [3] -> out float32 [B][H][W][4]
 *   (16-byte aligned): where 1 <= id <= F, rgb = kd * max(e, 0) and alpha 1, e the irradiance over pi at the geometric normal of
 *   face id - 1 turned towards campos (a uniform environment of radiance 1 gives kd); four zeros elsewhere.  B <= 64, H, W <= 2048,
 *   F < 2^24, else MD_ERR_UNSUPPORTED.  Forward only.
 */
#define MD_MESHPOST_MAX_ROUNDS 64
#define MD_MESH_COMPONENTS_WORKSPACE_BYTES 16
int md_mesh_smooth(const float* verts, const int32_t* ptr, const int32_t* adj, int64_t n_verts, int64_t n_codes, int32_t steps,
                   float lam, float mu, float* out, float* scratch, void* stream);
int md_mesh_components(const int64_t* faces, int64_t n_verts, int64_t n_faces, int32_t* label, int32_t* comp_faces, void* workspace,
                       int32_t* rounds, void* stream);
int md_shade_diffuse(const float* rast, const float* verts, const int64_t* faces, const float* campos, const float* sh,
                     const float* kd, int32_t batch, int64_t n_verts, int64_t n_faces, int32_t H, int32_t W, float* out, void* stream);

/*
 * Isotropic remeshing of generated meshes (the meshing_isotropic_explicit_remeshing of nvdiffrec/eval.py:449-456), csrc/remesh.hip.
 * In the manner of MeshLab's filter, not bit-equal to it.  Purely additive: MD_ABI_VERSION stays 16.
 *
 * THE REMESHING CONTRACT (the header comment of csrc/remesh.hip has it in full; tests/remesh_cases.py restates it in float32 numpy)
 *   One iteration = split, collapse rounds, flip rounds, relax, driven by meshdiffusion_amd/postprocess.py remesh, which rebuilds
 *   the tables between launch groups: the edge table lo, hi, mult int64 [E] sorted by (lo, hi); the neighbour CSR ptr int32 [V+1],
 *   adj int32 [2 E] (neighbour = code >> 1, ascending); the corner CSR cptr int32 [V+1], corner int32 [3 F] (codes 3 f + k,
 *   ascending); vflag int32 [V] (bit 0: on an edge of one face; bit 1: on an edge of three or more faces or named by a face that
 *   names a vertex twice; non-zero = fixed); vert_mesh int32 [V] and lo2 / hi2 float32 [M], the squares of 4/5 and 4/3 of the
 *   target length of each mesh.  Every decision is a function of the state before the launch: two runs agree bit for bit.  fp32,
 *   no contraction, predicates without sqrt or division, integer atomicMin / atomicAdd only.  Null or misaligned pointers (int64
 *   and the 64-bit priority words: 8 bytes) and non-positive sizes MD_ERR_BAD_ARG; V, 2 E or 3 F beyond int32 MD_ERR_UNSUPPORTED.
 *   An index outside its table is absent, never read.  Nothing is allocated and no entry point synchronises.
 * md_remesh_split_mark: mark int32 [E] = len2 > hi2[mesh of lo], mid float32 [E][3] = the midpoint of every edge.
 * md_remesh_split_count: count int32 [F] = 1 + the marked edges of a face (1 for a face that names a vertex twice).
 * md_remesh_split_emit: rank int32 [E] = the exclusive cumsum of mark (marked edge e becomes vertex V + rank[e]), offset int32 [F] =
 *   the exclusive cumsum of count -> out_faces int64 [F_out][3], the children of face f at offset[f], by the fixed patterns.
 * md_remesh_collapse_candidates: cand int32 [E], prio uint64 [E] = (float bits of len2) << 32 | e (all ones: no candidate).
 * md_remesh_collapse_claim: atomicMin of prio into word uint64 [V] (set to all ones by the caller) over N(a) u N(b).
 * md_remesh_collapse_apply: a candidate all of whose words hold its prio writes verts[a] = midpoint, remap[b] = a (remap int32 [V],
 *   set to the identity by the caller) and adds one to *counter (device int32, zeroed by the caller).
 * md_remesh_flip_candidates: cos2 = cos^2 of the flip angle in [0, 1]; info int32 [E][4] = (face (a,b,c), face (b,a,d), c, d) or -1;
 *   a flip that would lower the smallest of the six angles of its two faces is no candidate; prio = (16 - gain) << 32 | e.  md_remesh_flip_claim: atomicMin over a, b, c, d.  md_remesh_flip_apply: a winner rewrites its two
 *   face slots with (a,d,c) and (d,b,c) in place and adds one to *counter.
 * md_remesh_relax: out float32 [V][3] (not verts) = x + lam (d - n (n . d)), d the umbrella mean minus x, n the normalised sum of
 *   the incident face normals; a fixed vertex or one without neighbours keeps its bits.  lam must be finite.
 */
#define MD_REMESH_COLLAPSE_ROUNDS 8
#define MD_REMESH_FLIP_ROUNDS 4
#define MD_REMESH_MAX_ITERS 32
int md_remesh_split_mark(const float* verts, const int64_t* lo, const int64_t* hi, const int32_t* vert_mesh, const float* hi2,
                         int64_t n_verts, int64_t n_edges, int64_t n_meshes, int32_t* mark, float* mid, void* stream);
int md_remesh_split_count(const int64_t* faces, const int64_t* lo, const int64_t* hi, const int32_t* mark, int64_t n_verts,
                          int64_t n_edges, int64_t n_faces, int32_t* count, void* stream);
int md_remesh_split_emit(const float* verts, const int64_t* faces, const int64_t* lo, const int64_t* hi, const int32_t* mark,
                         const int32_t* rank, const int32_t* offset, int64_t n_verts, int64_t n_edges, int64_t n_faces,
                         int64_t n_faces_out, int64_t* out_faces, void* stream);
int md_remesh_collapse_candidates(const float* verts, const int64_t* faces, const int64_t* lo, const int64_t* hi, const int64_t* mult,
                                  const int32_t* ptr, const int32_t* adj, const int32_t* cptr, const int32_t* corner,
                                  const int32_t* vflag, const int32_t* vert_mesh, const float* lo2, const float* hi2, int64_t n_verts,
                                  int64_t n_edges, int64_t n_faces, int64_t n_meshes, int32_t* cand, uint64_t* prio, void* stream);
int md_remesh_collapse_claim(const int64_t* lo, const int64_t* hi, const int32_t* ptr, const int32_t* adj, const int32_t* cand,
                             const uint64_t* prio, int64_t n_verts, int64_t n_edges, uint64_t* word, void* stream);
int md_remesh_collapse_apply(const int64_t* lo, const int64_t* hi, const int32_t* ptr, const int32_t* adj, const int32_t* cand,
                             const uint64_t* prio, uint64_t* word, int64_t n_verts, int64_t n_edges, float* verts, int32_t* remap,
                             int32_t* counter, void* stream);
int md_remesh_flip_candidates(const float* verts, const int64_t* faces, const int64_t* lo, const int64_t* hi, const int64_t* mult,
                              const int32_t* ptr, const int32_t* cptr, const int32_t* corner, const int32_t* vflag, float cos2,
                              int64_t n_verts, int64_t n_edges, int64_t n_faces, int32_t* cand, uint64_t* prio, int32_t* info,
                              void* stream);
int md_remesh_flip_claim(const int64_t* lo, const int64_t* hi, const int32_t* cand, const uint64_t* prio, const int32_t* info,
                         int64_t n_verts, int64_t n_edges, uint64_t* word, void* stream);
int md_remesh_flip_apply(const int64_t* lo, const int64_t* hi, const int32_t* cand, const uint64_t* prio, const int32_t* info,
                         const uint64_t* word, int64_t n_verts, int64_t n_edges, int64_t n_faces, int64_t* faces, int32_t* counter,
                         void* stream);
int md_remesh_relax(const float* verts, const int64_t* faces, const int32_t* ptr, const int32_t* adj, const int32_t* cptr,
                    const int32_t* corner, const int32_t* vflag, int64_t n_verts, int64_t n_edges, int64_t n_faces, float lam,
                    float* out, void* stream);

/*
 * Distance from points to triangle meshes (csrc/meshdist.hip): closest point and generalised winding number by brute force, for the
 * warm start of the DMTet fit (meshdiffusion_amd/meshdist.py) and the re-projection of the remesher.  Purely additive:
 * MD_ABI_VERSION stays 16.
 *
 * THE MESH DISTANCE CONTRACT (the header comment of csrc/meshdist.hip has it in full; tests/meshdist_cases.py restates it)
 * md_mesh_query: tri float32 [T][3][3] gathered corners grouped by mesh, tri_ptr int32 [M+1] and query_ptr int32 [M+1] ascending
 *   CSRs on the device (clamped by the kernel, not read by the export), query float32 [Q][3] grouped by mesh.  Outputs, each may be
 *   NULL, one at least is not: dist2 float32 [Q], face int32 [Q] (index into tri, -1 when no triangle was taken), closest float32
 *   [Q][3], winding float32 [Q].  Closest point: Ericson's region classification in fp32 without contraction on (a, b - a, c - a),
 *   tests in the order A, B, C, AB, AC, BC, interior; triangles in ascending order, a candidate replaces the best only when d2 <
 *   best (ties keep the lowest index, NaN is never taken); no triangle taken: +inf, -1, the query.  Winding: the sum over the mesh's
 *   triangles of 2 atan2f(det, den) in float64 in ascending order, over 4 pi, rounded once; NaN in gives NaN.  No atomics: two
 *   runs agree bit for bit, however the launch is cut up.  In this order: null or misaligned tri_ptr / query / query_ptr,
 *   misaligned tri or output, no output: MD_ERR_BAD_ARG; a negative count, NULL tri with T > 0: MD_ERR_BAD_ARG; T or Q beyond
 *   int32, M > MD_MESHDIST_MAX_MESHES: MD_ERR_UNSUPPORTED; an output that is an input: MD_ERR_BAD_ARG.  Q == 0 or M == 0: MD_OK,
 *   nothing launched.  One mesh's triangles are not split over workgroups.  Nothing is allocated, nothing synchronises.
 */
#define MD_MESHDIST_MAX_MESHES 65535
int md_mesh_query(const float* tri, const int32_t* tri_ptr, const float* query, const int32_t* query_ptr, int64_t n_tris,
                  int64_t n_queries, int64_t n_meshes, float* dist2, int32_t* face, float* closest, float* winding, void* stream);

/*
 * Generation metrics under a light-field distance in the manner of Chen et al. 2003 (csrc/lfd.hip): a 48-byte descriptor per
 * silhouette and the all-pairs matrix of models, each L light fields of 10 silhouettes.  The original executable traces contours
 * and scales differently: values are NOT comparable with its numbers.  The reference has no counterpart.  Purely additive:
 * MD_ABI_VERSION stays 16.
 *
 * THE LFD CONTRACT (the header comment of csrc/lfd.hip has it in full; tests/lfd_cases.py restates it and derives the bars)
 * md_lfd_describe: mask uint8 [n][R][R] -> desc uint8 [n][48], coef float32 [n][45] (may be NULL), status int32 [n].
 *   A pixel is set where its byte is non-zero; pixel (row y, column x) sits at (x, y).  With `count` set pixels the centroid is
 *   c = (sum x / count, sum y / count) (integer sums, exact), rmax = max(0.5, max_p |p - c|), and per set pixel rho = |p - c| / rmax,
 *   theta = atan2(dy, dx).
 *   Zernike: for n = 1..10, m = n mod 2, ..., n in steps of 2 (35 values, in that order)
 *       z_nm = |sum_p R_nm(rho) e^{-i m theta}| / count,   R_nm(rho) = sum_s (-1)^s (n-s)! / (s! ((n+m)/2-s)! ((n-m)/2-s)!) rho^(n-2s).
 *   Signature: 64 angular bins, b = floor(64 theta / 2 pi + 0.5) mod 64; sig[b] = the largest rho of the bin's pixels, 0 when empty.
 *   Fourier: f_k = |sum_b sig[b] e^{-2 pi i k b / 64}| / sum_b sig[b] for k = 1..10; 0 when sum_b sig[b] = 0 (one pixel).
 *   coef = the 45 values 512 z, 512 f rounded to fp32; desc = min(255, rint(coef)) as bytes, then three zero bytes.
 *   An empty mask: desc and coef 0, status 1; otherwise status 0.
 *   Evaluation scheme: the integers Nx = x count - sum x, Ny = y count - sum y, q = Nx^2 + Ny^2 and Q = max q are exact; Qe =
 *   max(Q, count^2 / 4), inv = fp32(1 / sqrt(Qe)), inv2 = fp32(1 / Qe), both formed in float64 once per mask.  Per pixel, in fp32
 *   without contraction: w = (fp32(Nx) inv, -(fp32(Ny) inv)) = rho e^{-i theta}, t = fp32(q) inv2 = rho^2; W_0 = 1, W_m = W_{m-1} w
 *   (complex product, four multiplies, an add and a subtract); R_nm(rho) e^{-i m theta} = P_nm(t) W_m with P_nm the polynomial of
 *   degree (n-m)/2 in t with the integer coefficients above, by Horner's rule from the highest power (a multiply and an add per
 *   step); both components of P W_m are multiplied by 2^32, rounded to integers and summed as 64-bit integers, so the sums are
 *   exact in any order.  |sum| / count, the signature (sig[b] = sqrt(max q of the bin / Qe), the maximum an exact integer), the
 *   64-point transform and the normalisation are float64, rounded once to fp32.  The bin of a pixel is computed in fp32:
 *   floorf(atan2f(fp32(Ny), fp32(Nx)) * fp32(64 / 2 pi) + 0.5f) mod 64.  Two runs agree bit for bit, however the launch is cut up.
 *   Null mask, desc or status, coef not 4-byte aligned, n < 1 or R < 1: MD_ERR_BAD_ARG; R > MD_LFD_MAX_RES or n >= 2^31 / 256:
 *   MD_ERR_UNSUPPORTED.  One workgroup per mask.
 * md_lfd_matrix: x uint8 [nx][L][10][48], y uint8 [ny][L][10][48] on the device (4-byte aligned), perm uint8 [G][10] ON THE HOST
 *   (read by the export before it returns) -> out int32 [nx][ny],
 *       out[i][j] = min over la, lb < L and g < G of sum_{v<10} SAD48(x[i][la][v], y[j][lb][perm[g][v]]),
 *   SAD48 the sum of absolute differences over all 48 bytes.  Integers throughout: exact, independent of the launch.
 *   triangular != 0 (needs x == y and nx == ny): only the pairs i < j are computed and written to [i][j] and [j][i]; the diagonal
 *   is 0.  In this order: null or misaligned pointers, sizes < 1: MD_ERR_BAD_ARG; L > MD_LFD_MAX_FIELDS or G >
 *   MD_LFD_MAX_ROTATIONS: MD_ERR_UNSUPPORTED; a perm entry >= 10, triangular with x != y or nx != ny: MD_ERR_BAD_ARG; nx >= 2^24 or
 *   ny > 65535 MD_LFD_RUN: MD_ERR_UNSUPPORTED.  A workgroup owns one x model and
 *   MD_LFD_RUN consecutive y models.  Nothing is allocated, nothing synchronises.
 */
#define MD_LFD_MAX_RES 512
#define MD_LFD_DESC_BYTES 48
#define MD_LFD_COEFS 45
#define MD_LFD_VIEWS 10
#define MD_LFD_MAX_FIELDS 16
#define MD_LFD_MAX_ROTATIONS 64
#define MD_LFD_RUN 8
int md_lfd_describe(const uint8_t* mask, int32_t n, int32_t R, uint8_t* desc, float* coef, int32_t* status, void* stream);
int md_lfd_matrix(const uint8_t* x, const uint8_t* y, const uint8_t* perm, int32_t nx, int32_t ny, int32_t L, int32_t G,
                  int32_t triangular, int32_t* out, void* stream);

/*
 * Textures for meshes (csrc/texture.hip): the bilinear fetch of dr.texture (filter_mode = 'linear', no mip levels) with gradients
 * for the texture and the uv, one dilation step of a baked atlas, and the multi-view projection bake
 * (meshdiffusion_amd/texture.py, render.render_textured, fit.fit_texture).  Purely additive: MD_ABI_VERSION stays 16.
 *
 * THE TEXTURE CONTRACT (the header comment of csrc/texture.hip has it in full; tests/texture_cases.py restates it in numpy)
 * tex float32 [T][Ht][Wt][C], T = 1 or B, 1 <= C <= 8, Ht, Wt <= MD_TEXTURE_MAX_RES; uv float32 [B][H][W][2]; rast float32
 *   [B][H][W][4] or NULL.  A pixel with rast id 0, or whose x = u Wt - 0.5 or y = v Ht - 0.5 is not finite, is skipped: zeros out,
 *   nothing to any gradient.  Texel (row i, column j) has its centre at ((j + 0.5) / Wt, (i + 0.5) / Ht); row 0 is v = 0.
 *   fp32 without contraction: x0 = floor(x), fx = x - x0 (y likewise), out = (t00 (1 - fx) + t10 fx) (1 - fy) + (t01 (1 - fx) + t11
 *   fx) fy; boundary MD_TEXTURE_CLAMP clamps the four indices, MD_TEXTURE_WRAP takes them modulo the size.
 * md_texture_sample: the fetch.  tex and out 16-byte aligned, uv 8, rast 16.
 * md_texture_codes: dest int32 [B H W][4] (16-byte aligned), the texel row (t Ht + iy) Wt + ix of the code 4 pixel + corner, corners
 *   (t00, t10, t01, t11), and T Ht Wt for the codes of a skipped pixel: the host sorts the codes stably by row into (ptr int32
 *   [T Ht Wt + 2], order int32 [4 B H W]).
 * md_texture_sample_bwd: dtex (may be NULL; needs ptr and order) = per texel the Kahan sum of w_k grad_out[pixel] in the order of
 *   the CSR, every element written; duv (may be NULL) = (Wt sum_c g ((t10 - t00)(1 - fy) + (t11 - t01) fy), Ht sum_c g ((t01 - t00)
 *   (1 - fx) + (t11 - t10) fx)), zeros where skipped.  One of the two at least.  No atomics: two runs agree bit for bit.
 * md_texture_dilate: one step.  A texel with mask <= 0.5 and a covered 8-neighbour becomes the mean of those neighbours (summed in
 *   row-major order) and gets mask 1; the rest is copied.  tex float32 [Ht][Wt][C], mask float32 [Ht][Wt]; no output may overlap
 *   an input or the other output (MD_ERR_BAD_ARG).
 * md_texture_project: per texel with texmask > 0.5 the cos^power-weighted mean over the views (ascending, V <=
 *   MD_TEXTURE_MAX_VIEWS) of the bilinear fetch of image [V][H][W][3] at the texel's projection, a view counting only if w > 0,
 *   ndc in [-1, 1]^2, the four footprint pixels inside the image with viewmask > 0.5, |p - campos| - depth[nearest pixel] <=
 *   depth_bias and cos > cos_min.  color float32 [Ht][Wt][3] (zeros where the weights sum to 0), weight float32 [Ht][Wt].
 * Every export, in this order: null or misaligned pointers: MD_ERR_BAD_ARG; a size < 1, T not 1 or B, an unknown boundary, a NaN
 *   scalar: MD_ERR_BAD_ARG; C outside 1..8, Ht or Wt > MD_TEXTURE_MAX_RES, B or H or W beyond the rasteriser's limits, V >
 *   MD_TEXTURE_MAX_VIEWS: MD_ERR_UNSUPPORTED; aliasing: MD_ERR_BAD_ARG.  Nothing is allocated, nothing synchronises.
 */
#define MD_TEXTURE_CLAMP 0
#define MD_TEXTURE_WRAP 1
#define MD_TEXTURE_MAX_RES 2048
#define MD_TEXTURE_MAX_VIEWS 64
int md_texture_sample(const float* tex, const float* uv, const float* rast, int32_t T, int32_t Ht, int32_t Wt, int32_t C, int32_t B,
                      int32_t H, int32_t W, int32_t boundary, float* out, void* stream);
int md_texture_codes(const float* uv, const float* rast, int32_t T, int32_t Ht, int32_t Wt, int32_t B, int32_t H, int32_t W,
                     int32_t boundary, int32_t* dest, void* stream);
int md_texture_sample_bwd(const float* tex, const float* uv, const float* rast, const float* grad_out, const int32_t* ptr,
                          const int32_t* order, int32_t T, int32_t Ht, int32_t Wt, int32_t C, int32_t B, int32_t H, int32_t W,
                          int32_t boundary, float* dtex, float* duv, void* stream);
int md_texture_dilate(const float* tex, const float* mask, int32_t Ht, int32_t Wt, int32_t C, float* out_tex, float* out_mask,
                      void* stream);
int md_texture_project(const float* pos, const float* nrm, const float* texmask, const float* image, const float* depth,
                       const float* viewmask, const float* mvp, const float* campos, int32_t Ht, int32_t Wt, int32_t V, int32_t H,
                       int32_t W, float depth_bias, float cos_min, float power, float* color, float* weight, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MESHDIFFUSION_HIP_H */
