// md_conv3_low: the 3x3x3 convolutions of the 4^3 level (MD_CFG_C3_LOW launches of md_gemm_conv with the fp32-parts loader and
// split-K) with the batch folded into the MFMA columns.
//
// Replaces (reference, Python/ATen): nn.GroupNorm + nn.SiLU + nn.Conv3d 3x3x3 of the ResnetBlocks at the lowest resolution,
// lib/diffusion/models/layers.py:676-681 and :118-124.  md_gemm_conv (gemm_conv.hip) routes to this kernel; it has no export.
//
// Why a file of its own.  On a 4^3 grid the generic tile is one workgroup per (sample, 128 rows, K slice): 6 MFMAs per wave between
// two barriers, and every sample's workgroup fetches the same weight tiles again (8 x at B = 8).  Here a workgroup owns
// 32 output rows x the 64 positions of CL_SB = 4 samples x one K slice:
//   * one wave per sample: 32 rows x 64 columns = two 32x32 accumulators.  The A fragments (weights) of a (chunk, tap) step are the
//     same for the four waves; every wave loads them straight from the WPK tiles into registers (the three repeats hit the L1),
//     so a weight tile leaves the L2 once per four samples.
//   * the wave's operand is its sample's zero-padded 6^3 halo of the slice's current 32-channel chunk in LDS, [4 groups][hi|lo][306
//     slots] 16-byte items (38 KB per sample), staged once per chunk by the wave itself: 64 lanes = 64 positions, the same
//     GroupNorm affine + SiLU + md_split2 arithmetic as the generic kernel's BF loader.  The rim is zeroed once and never written.
//   * the 27 taps are straight-line code: a tap is a constant slot offset, so the LDS addresses are one VGPR per lane + immediates.
//     Weight fragments travel through a ring of CL_RING = 9 taps of registers (27 = 3 x 9: static ring slots across chunks), each
//     slot refilled with the tap nine ahead as soon as it is consumed; the next chunk's 8 fp32 values per lane and channel group
//     are requested at tap 18.  A wave reads only what it wrote itself: the two barriers per chunk order its own LDS traffic.
// Per output element the MFMA chain is the generic kernel's: chunks ascending inside the slice, taps 0..26, the two 16-channel
// k-steps, alo*bhi, ahi*blo, ahi*bhi with the same channels in the same k positions -- the words written to `partial` are
// bit-identical (tests/test_gpu_small_level_bits.py), and md_splitk_reduce(_stats) finishes the job as before.
#include "md_common.h"

namespace {
constexpr int CL_SB = 4;                            // samples per workgroup = waves
constexpr int CL_THREADS = CL_SB * 64;
constexpr int CL_ROWS = 32;                         // output rows per workgroup: a quarter of a WPK tile (NT = 128)
constexpr int CL_KC = 32, CL_KG = CL_KC / 8;        // K chunk of the WPK tiles, its 8-channel groups
constexpr int CL_NT = 128;
constexpr int CL_TAPS = 27;
// halo slot of (hz, hy, hx) in 0..5: hz * 52 + hy * 8 + hx.  With these strides the 16 lanes of every ds_read_b128 group (4 x of
// rows y 0 and 3 of one z, rows y 1 and 2 of the next) fall on 16 different 16-byte bank groups for every tap; the dense 36 / 6
// strides are 3-way conflicted (tests/test_cpu_small_level_layout.py).  306 slots instead of 216: 153 KB of LDS for four samples.
constexpr int CL_SZ = 52, CL_SY = 8;
constexpr int CL_HS = 5 * CL_SZ + 5 * CL_SY + 6;    // halo slots of one (group, plane)
constexpr int CL_SAMPLE_ITEMS = CL_KG * 2 * CL_HS;  // 16-byte items of one sample's halo image
constexpr int CL_W_ITEMS = CL_KG * 2 * CL_NT;       // 16-byte items of one WPK tile
constexpr int CL_RING = 9;                          // taps of weight fragments in flight per wave
static_assert(CL_TAPS % CL_RING == 0, "ring slots must be static across chunks");
static_assert(CL_SB * CL_SAMPLE_ITEMS * 16 <= 160 * 1024, "LDS budget");
}  // namespace

// AC: the GroupNorm affine is given (b_ac); SILU: SiLU after it.  Template flags, and loads whose index is clamped instead of
// skipped, keep the chunk body free of branches: the compiler's vmcnt bookkeeping stays exact only in straight-line code, and one
// conservative s_waitcnt vmcnt(0) per ring cycle would drain the nine taps in flight.
template <bool AC, bool SILU>
__global__ __launch_bounds__(CL_THREADS) void md_conv3_low_kernel(const MdGemmConvArgs A, int nrb, int nsb) {
  __shared__ __attribute__((aligned(16))) uint4 smem[CL_SB * CL_SAMPLE_ITEMS];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 31, h = lane >> 5;

  // XCD-aware block order (workgroup i runs on XCD i % 8): the sample blocks that share a weight slice are neighbours on one XCD
  int bid = blockIdx.x;
  if ((gridDim.x & 7) == 0) bid = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const int sb = bid % nsb, rb = (bid / nsb) % nrb, kz = bid / (nsb * nrb);
  const int b = sb * CL_SB + wid;
  const bool valid = b < A.batch;

  const int ncc_total = A.kdim / CL_KC;
  const int cc_lo = (int)(((int64_t)kz * ncc_total) / A.ksplit);
  const int ncc = (int)(((int64_t)(kz + 1) * ncc_total) / A.ksplit) - cc_lo;
  const int nsteps = ncc * CL_TAPS;

  uint4* own = smem + wid * CL_SAMPLE_ITEMS;
  for (int i = lane; i < CL_SAMPLE_ITEMS; i += 64) own[i] = make_uint4(0, 0, 0, 0);

  // ---- weight fragments: WPK tile (rb / 4, chunk, tap), rows (rb % 4) * 32 + j, item ((ks * 2 + h) * 2 + plane) * 128 + row ----
  const uint4* wp = (const uint4*)A.a + ((int64_t)(rb >> 2) * ncc_total + cc_lo) * CL_TAPS * CL_W_ITEMS + h * 2 * CL_NT + (rb & 3) * CL_ROWS + j;
  uint4 wr[CL_RING][4];
  auto w_issue = [&](uint4 (&r)[4], int s) {
    const uint4* p = wp + (int64_t)s * CL_W_ITEMS;
    r[0] = p[0];                         // k-step 0: hi, lo
    r[1] = p[CL_NT];
    r[2] = p[4 * CL_NT];                 // k-step 1: hi, lo
    r[3] = p[5 * CL_NT];
  };

  // ---- operand: 8 fp32 channels of the lane's position per channel group, and the group's folded affine ----
  const uint4* p1 = (const uint4*)A.b + (int64_t)b * (A.b_bstride / 4);
  const uint4* p2 = (const uint4*)A.b2 + (int64_t)b * (A.b2_bstride / 4);
  uint4 hx[2 * CL_KG];
  f32x4 hac[CL_KG][4];
  auto h_issue = [&](int cc) {
#pragma unroll
    for (int kg = 0; kg < CL_KG; ++kg) {
      const int g8 = (cc_lo + cc) * CL_KG + kg;
      const uint4* cb = (g8 < (A.b_split >> 3)) ? p1 + (int64_t)g8 * 64 * 2 : p2 + (int64_t)(g8 - (A.b_split >> 3)) * 64 * 2;
      hx[2 * kg] = cb[lane * 2];
      hx[2 * kg + 1] = cb[lane * 2 + 1];
      if constexpr (AC) {
        const f32x4* ap = (const f32x4*)(A.b_ac + ((int64_t)b * A.kdim + (int64_t)g8 * 8) * 2);
#pragma unroll
        for (int q = 0; q < 4; ++q) hac[kg][q] = ap[q];
      }
    }
  };
  const int islot = ((lane >> 4) + 1) * CL_SZ + (((lane >> 2) & 3) + 1) * CL_SY + (lane & 3) + 1;   // position `lane` inside the 6^3 halo
  auto h_commit = [&]() {
#pragma unroll
    for (int kg = 0; kg < CL_KG; ++kg) {
      const uint4 r0 = hx[2 * kg], r1 = hx[2 * kg + 1];
      const float v[8] = {__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), __uint_as_float(r0.w),
                          __uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z), __uint_as_float(r1.w)};
      float yv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {          // the generic BF loader's arithmetic, expression for expression
        float y = v[e];
        if constexpr (AC) {
          y = y * hac[kg][e >> 1][(e & 1) * 2] + hac[kg][e >> 1][(e & 1) * 2 + 1];
          if constexpr (SILU) y = y * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(y * -1.4426950408889634f));
        }
        // opaque per value: from the pair build of md_split2 upwards the vectoriser would otherwise pack two values' chains into
        // v_pk_fma_f32 / v_pk_mul_f32, and the words then differ from the generic loader's scalar v_fma_f32 ... v_mul_f32
        asm volatile("" : "+v"(y));
        yv[e] = y;
      }
      uint32_t hi[4], lo[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) md_split2(yv[2 * e], yv[2 * e + 1], hi[e], lo[e]);
      own[(kg * 2) * CL_HS + islot] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
      own[(kg * 2 + 1) * CL_HS + islot] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    }
  };

  // ---- B fragments: column j of tile cm is position cm * 32 + j; group ks * 2 + h; tap (dz, dy, dx) adds a constant slot offset ----
  const bf16x8* bl = (const bf16x8*)own + h * 2 * CL_HS + (j >> 4) * CL_SZ + ((j >> 2) & 3) * CL_SY + (j & 3);
  f32x16 acc[2];
#pragma unroll
  for (int cm = 0; cm < 2; ++cm)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[cm][r] = 0.f;

  if (valid) {
    h_issue(0);
#pragma unroll
    for (int s = 0; s < CL_RING; ++s) w_issue(wr[s], s);          // nsteps >= 27
  }
  for (int cc = 0; cc < ncc; ++cc) {
    __syncthreads();                      // the previous chunk's fragment reads are done
    if (valid) h_commit();
    __syncthreads();
    if (valid) {
#pragma unroll
      for (int t = 0; t < CL_TAPS; ++t) {
        const int toff = (t / 9) * CL_SZ + ((t / 3) % 3) * CL_SY + t % 3;
        uint4 (&w)[4] = wr[t % CL_RING];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const bf16x8 ahi = __builtin_bit_cast(bf16x8, w[2 * ks]), alo = __builtin_bit_cast(bf16x8, w[2 * ks + 1]);
          bf16x8 bhi[2], blo[2];
#pragma unroll
          for (int cm = 0; cm < 2; ++cm) {
            bhi[cm] = bl[(ks * 4) * CL_HS + cm * 2 * CL_SZ + toff];
            blo[cm] = bl[(ks * 4 + 1) * CL_HS + cm * 2 * CL_SZ + toff];
          }
          // the two accumulators' chains interleaved; each chain in the generic kernel's order
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, bhi[0], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, bhi[1], acc[1], 0, 0, 0);
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, blo[0], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, blo[1], acc[1], 0, 0, 0);
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, bhi[0], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, bhi[1], acc[1], 0, 0, 0);
        }
        // scheduling fences: without them the scheduler sinks every refill down to its use nine taps later (one tap in flight)
        __builtin_amdgcn_sched_barrier(0);
        const int sn = cc * CL_TAPS + t + CL_RING;
        w_issue(w, sn < nsteps ? sn : nsteps - 1);                  // past the end: the last step once more, never used
        if (t == 18) h_issue(cc + 1 < ncc ? cc + 1 : cc);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // ---- raw partial sums -> workspace slice [ksplit][B][rows_alloc / 8][64][8], as the generic kernel writes them ----
  if (!valid) return;
  const int rga = A.rows_alloc / 8;
  float* part = A.partial + ((int64_t)kz * A.batch + b) * rga * 64 * 8;
#pragma unroll
  for (int cm = 0; cm < 2; ++cm) {
    const int gp = cm * 32 + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = rb * CL_ROWS + 8 * q + 4 * h;
      if (row >= A.rows_alloc) continue;
      const f32x4 o4 = {acc[cm][q * 4 + 0], acc[cm][q * 4 + 1], acc[cm][q * 4 + 2], acc[cm][q * 4 + 3]};
      *(f32x4*)(part + ((int64_t)(row >> 3) * 64 + gp) * 8 + (row & 7)) = o4;
    }
  }
}

// The launches this kernel takes: exactly the ones launch_cfg<Cfg_C3_LOW> would accept with the fp32-parts loader, split-K and a
// 4^3 grid.  Everything else (and every launch it would refuse) stays with the generic kernel and its own argument checks.
bool md_conv3_low_takes(const MdGemmConvArgs& a) {
  if (a.cfg != MD_CFG_C3_LOW || a.b_mode != MD_B_F32B_GN || a.ups || a.ksplit <= 1) return false;
  if (a.D != 4 || a.H != 4 || a.W != 4) return false;
  if (a.a_src != MD_A_PACKED || a.out_mode != MD_OUT_F32B || a.prec != MD_PREC_BF16X3) return false;
  if (a.kdim <= 0 || a.kdim % CL_KC != 0 || a.rows <= 0 || a.rows_alloc % 8 != 0 || a.batch <= 0) return false;
  if ((a.b_split & 7) || a.b_split <= 0 || (a.b_split < a.kdim && a.b2 == nullptr)) return false;
  if (a.b_silu && a.b_ac == nullptr) return false;
  if (a.partial == nullptr || a.ksplit > a.kdim / CL_KC) return false;
  return true;
}

int md_launch_conv3_low(const MdGemmConvArgs& a, hipStream_t stream) {
  // the rows the generic grid covers: whole WPK tiles, cut at rows_alloc
  int rows_cover = ((a.rows + CL_NT - 1) / CL_NT) * CL_NT;
  if (rows_cover > a.rows_alloc) rows_cover = a.rows_alloc;
  const int nrb = (rows_cover + CL_ROWS - 1) / CL_ROWS;
  const int nsb = (a.batch + CL_SB - 1) / CL_SB;
  MD_HIP_CLEAR_ERROR();
  const dim3 grid((unsigned)(nrb * nsb * a.ksplit)), block(CL_THREADS);
  if (a.b_ac == nullptr) hipLaunchKernelGGL((md_conv3_low_kernel<false, false>), grid, block, 0, stream, a, nrb, nsb);
  else if (a.b_silu) hipLaunchKernelGGL((md_conv3_low_kernel<true, true>), grid, block, 0, stream, a, nrb, nsb);
  else hipLaunchKernelGGL((md_conv3_low_kernel<true, false>), grid, block, 0, stream, a, nrb, nsb);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
