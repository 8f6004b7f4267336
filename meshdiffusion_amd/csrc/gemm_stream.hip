// md_gemm_stream: the 1x1x1 convolutions / GEMMs of MD_CFG_G1_128 with F32B output (attention projections, small-grid NINs and
// shortcuts) in the form of md_nin_f32_kernel: positions stream HBM -> registers -> MFMA, only the weights pass through LDS.
//
// Replaces (reference, Python/ATen): NIN 1x1x1, lib/diffusion/models/layers.py:573-582 (used at :598-608 and :667,:688).
// md_gemm_conv (gemm_conv.hip) routes to this kernel; it has no export.
//
// The generic tile stages BOTH operands of every 32-channel chunk in LDS behind a barrier.  Here a workgroup owns the generic tile's
// 128 rows x 256 positions (same grid, same XCD-aware order) with one wave per 32 positions and four 32x32 accumulators per wave:
//   * B operand: the lane's 8 channels of its position go straight from global memory into registers -- 16-byte hi and lo items of
//     the S16B tensor, or 32 bytes of the fp32 parts split by md_split2 (split-only loader) -- in two register sets of four
//     16-channel steps, each refilled with the set two ahead as soon as it is consumed.
//   * A operand: the WPK tiles of the workgroup's row block in stages of 128 channels (4 tiles = 64 KB, a linear copy), double-
//     buffered in LDS: the next stage is requested at the start of a stage and stored at its end, one barrier per 96 MFMAs of a wave.
// Per output element the MFMA chain is the generic kernel's (chunks ascending, the two 16-channel k-steps, alo*bhi, ahi*blo, ahi*bhi)
// and the epilogue is its F32B branch expression for expression: bit-identical words (tests/test_gpu_small_level_bits.py).
// Takes K = multiples of 128; other K, other output modes, an S16B A operand and split-K stay with the generic tile.
#include "md_common.h"

namespace {
constexpr int GS_ROWS = 128, GS_WAVES = 8, GS_THREADS = GS_WAVES * 64, GS_COLS = GS_WAVES * 32;
constexpr int GS_STAGE_CH = 128;                              // channels per weight stage
constexpr int GS_STAGE_ITEMS = (GS_STAGE_CH / 32) * 1024;     // 16-byte items per stage: four WPK tiles
constexpr int GS_W_PER_THREAD = GS_STAGE_ITEMS / GS_THREADS;  // 8
typedef uint32_t gs_u32x4 __attribute__((ext_vector_type(4)));   // a first-class 16-byte value: a uint4 copy global -> private -> LDS
                                                                // stays a pair of memcpys through a stack slot
constexpr int GS_SET = 4;                                     // 16-channel steps per B register set; a stage = two sets
}  // namespace

template <bool F32>
__global__ __launch_bounds__(GS_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void md_gemm_stream_kernel(const MdGemmConvArgs A) {
  __shared__ __attribute__((aligned(16))) gs_u32x4 wl[2 * GS_STAGE_ITEMS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int64_t P = A.W;
  const int tiles = A.W / GS_COLS;
  int bid = blockIdx.x;
  if ((gridDim.x & 7) == 0) bid = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const int b = bid / tiles, t = bid % tiles;
  const int rt = blockIdx.y;
  const int nst = A.kdim / GS_STAGE_CH;
  const int64_t pos = (int64_t)t * GS_COLS + wid * 32 + j;

  // ---- weights: stage s of row tile rt = WPK tiles (rt, 4 s .. 4 s + 3), contiguous ----
  const gs_u32x4* wsrc = (const gs_u32x4*)A.a + (int64_t)rt * nst * GS_STAGE_ITEMS + tid;
  gs_u32x4 wreg[GS_W_PER_THREAD];
  auto w_issue = [&](gs_u32x4 (&r)[GS_W_PER_THREAD], int s) {
#pragma unroll
    for (int i = 0; i < GS_W_PER_THREAD; ++i) r[i] = wsrc[(int64_t)s * GS_STAGE_ITEMS + i * GS_THREADS];
  };
  auto w_commit = [&](const gs_u32x4 (&r)[GS_W_PER_THREAD], int buf) {
#pragma unroll
    for (int i = 0; i < GS_W_PER_THREAD; ++i) wl[buf * GS_STAGE_ITEMS + tid + i * GS_THREADS] = r[i];
  };

  // ---- B operand: 16-channel step k16 -> channel group g8 = 2 k16 + h of the lane's position ----
  const uint4* bs16 = (const uint4*)A.b + (int64_t)b * (A.b_bstride / 8) + pos;
  const uint4* bp1 = (const uint4*)A.b + (int64_t)b * (A.b_bstride / 4) + pos * 2;
  const uint4* bp2 = (const uint4*)A.b2 + (int64_t)b * (A.b2_bstride / 4) + pos * 2;
  const int split8 = A.b_split >> 3;
  uint4 s0[2 * GS_SET], s1[2 * GS_SET];
  auto b_issue = [&](uint4 (&st)[2 * GS_SET], int k16_0) {
#pragma unroll
    for (int k = 0; k < GS_SET; ++k) {
      const int g8 = 2 * (k16_0 + k) + h;
      if constexpr (F32) {
        const uint4* cb = (g8 < split8) ? bp1 + (int64_t)g8 * P * 2 : bp2 + (int64_t)(g8 - split8) * P * 2;
        st[2 * k] = cb[0];
        st[2 * k + 1] = cb[1];
      } else {
        st[2 * k] = bs16[(int64_t)(g8 * 2) * P];
        st[2 * k + 1] = bs16[(int64_t)(g8 * 2 + 1) * P];
      }
    }
  };

  f32x16 acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[r][e] = 0.f;
  const bf16x8* wf = (const bf16x8*)wl;
  // k-step kl (0..7) of the stage in buffer `buf`: tile kl / 2, group 2 (kl & 1) + h, item ((group * 2 + plane) * 128 + row)
  auto step = [&](int buf, int kl, const uint4& r0, const uint4& r1) {
    bf16x8 bhi, blo;
    if constexpr (F32) {
      uint32_t hw[4], lw[4];
      md_split2(__uint_as_float(r0.x), __uint_as_float(r0.y), hw[0], lw[0]);
      md_split2(__uint_as_float(r0.z), __uint_as_float(r0.w), hw[1], lw[1]);
      md_split2(__uint_as_float(r1.x), __uint_as_float(r1.y), hw[2], lw[2]);
      md_split2(__uint_as_float(r1.z), __uint_as_float(r1.w), hw[3], lw[3]);
      bhi = __builtin_bit_cast(bf16x8, make_uint4(hw[0], hw[1], hw[2], hw[3]));
      blo = __builtin_bit_cast(bf16x8, make_uint4(lw[0], lw[1], lw[2], lw[3]));
    } else {
      bhi = __builtin_bit_cast(bf16x8, r0);
      blo = __builtin_bit_cast(bf16x8, r1);
    }
    const bf16x8* wt = wf + buf * GS_STAGE_ITEMS + (kl >> 1) * 1024 + ((2 * (kl & 1) + h) * 2) * GS_ROWS + j;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bf16x8 ahi = wt[r * 32];
      const bf16x8 alo = wt[GS_ROWS + r * 32];
      acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, bhi, acc[r], 0, 0, 0);
      acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, blo, acc[r], 0, 0, 0);
      acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, bhi, acc[r], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);   // one scheduling region per step: the scheduler would hoist the LDS reads of all steps
  };

  w_issue(wreg, 0);
  b_issue(s0, 0);
  b_issue(s1, GS_SET);
  w_commit(wreg, 0);
  __syncthreads();
  const int last16 = (nst - 1) * 2 * GS_SET;       // first step of the last stage: refills past the end repeat it, never used
  for (int s = 0; s < nst; ++s) {
    const int buf = s & 1;
    w_issue(wreg, s + 1 < nst ? s + 1 : s);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < GS_SET; ++k) step(buf, k, s0[2 * k], s0[2 * k + 1]);
    b_issue(s0, s + 1 < nst ? (s + 1) * 2 * GS_SET : last16);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < GS_SET; ++k) step(buf, GS_SET + k, s1[2 * k], s1[2 * k + 1]);
    b_issue(s1, s + 1 < nst ? (s + 1) * 2 * GS_SET + GS_SET : last16 + GS_SET);
    __builtin_amdgcn_sched_barrier(0);
    w_commit(wreg, buf ^ 1);                   // read last in stage s - 1: every wave has passed that stage's barrier
    __syncthreads();
  }

  // ---- epilogue: the generic kernel's F32B branch ----
  const float alpha = A.alpha;
  const int rows = A.rows, rows_alloc = A.rows_alloc;
  const int rg_alloc = rows_alloc / 8;
  const int64_t gp = pos;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rowbase = rt * GS_ROWS + r * 32;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = rowbase + 8 * q + 4 * h;
      if (row >= rows_alloc) continue;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x = alpha * acc[r][q * 4 + e];
        if (A.bias != nullptr && row + e < rows) x += A.bias[(int64_t)b * A.bias_bstride + row + e];
        v[e] = x;
      }
      const int64_t o = (((int64_t)b * rg_alloc + (row >> 3)) * P + gp) * 8 + (row & 7);
      if (A.residual != nullptr) {
        const int64_t ro = (int64_t)b * A.res_bstride + (((int64_t)(row >> 3)) * P + gp) * 8 + (row & 7);
        const f32x4 r4 = *(const f32x4*)(A.residual + ro);
        v[0] += r4[0]; v[1] += r4[1]; v[2] += r4[2]; v[3] += r4[3];
      }
      f32x4 o4 = {v[0], v[1], v[2], v[3]};
      *(f32x4*)((float*)A.out + o) = o4;
    }
  }
}

// The launches this kernel takes: a subset of what launch_cfg<Cfg_G1_128> accepts; everything else, and every launch it would
// refuse, stays with the generic kernel and its own argument checks.
bool md_gemm_stream_takes(const MdGemmConvArgs& a) {
  if (a.cfg != MD_CFG_G1_128 || a.a_src != MD_A_PACKED || a.out_mode != MD_OUT_F32B || a.ksplit > 1 || a.ups) return false;
  if (a.D != 1 || a.H != 1 || a.W <= 0 || a.W % GS_COLS != 0 || a.prec != MD_PREC_BF16X3) return false;
  if (a.kdim <= 0 || a.kdim % GS_STAGE_CH != 0 || a.rows <= 0 || a.rows_alloc % 8 != 0 || a.batch <= 0) return false;
  if (a.b_mode == MD_B_S16B) return true;
  if (a.b_mode != MD_B_F32B_GN || a.b_ac != nullptr) return false;
  if ((a.b_split & 7) || a.b_split <= 0 || (a.b_split < a.kdim && a.b2 == nullptr)) return false;
  return true;
}

int md_launch_gemm_stream(const MdGemmConvArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W / GS_COLS) * a.batch), (unsigned)((a.rows + GS_ROWS - 1) / GS_ROWS));
  MD_HIP_CLEAR_ERROR();
  if (a.b_mode == MD_B_F32B_GN) hipLaunchKernelGGL((md_gemm_stream_kernel<true>), grid, dim3(GS_THREADS), 0, stream, a);
  else hipLaunchKernelGGL((md_gemm_stream_kernel<false>), grid, dim3(GS_THREADS), 0, stream, a);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
