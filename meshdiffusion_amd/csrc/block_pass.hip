// md_wino_prep_f6_nin: ONE pass over the input of a ResnetBlock with a NIN shortcut.  The block input cat(h, skip) feeds two
// HBM-bound kernels, md_wino_prep_f6 (Conv_0's f16f6 operand T) and md_nin_f32 (the shortcut `res`); here a workgroup of
// md_nin_f32_kernel's structure (nin_stream.hip: persistent, the packed NIN weights resident in LDS, the full K of a
// 256-position tile streamed HBM -> registers through two register sets refilled two groups ahead) writes both from the
// one copy of the input it holds.  Same bits as the two kernels: the MFMA sequence and the `res` epilogue are md_nin_f32's,
// the operand arithmetic is compiled from md_prep_f6.h / md_split_f16f6 like md_wino_prep2_f6_kernel's.
//
// Per 16-channel step a lane (j = position of the wave's 32-position segment, h = channel group of the K block) holds 8 raw
// fp32 values.  After the MFMAs it
//   activates them (a x + c, SiLU, equaliser; a / c / eq come from LDS tables: the sample's a / c in a wave-private copy,
//   because the waves of a workgroup never synchronise and may stand in different samples),
//   takes the activated values of positions j - 1 and j + 1 from the neighbouring lanes (DPP wave shifts); lanes j = 0 / 31 take
//   them from the HALO: per group of 4 steps, lane L < 32 loads 16 bytes of the position in front of / behind the segment
//   (L = step, channel group, end, half) and activates them once (pulled with ds_bpermute) -- zero where that position lies outside the row,
//   forms the two frequencies of its position's parity on its own 8 channels (even position of a pair: f0, f1; odd: f2, f3),
//   swaps one of them with the lane holding the other channel group of the same position (v_permlane32_swap): every lane now
//   has ONE frequency f = 2 (j & 1) + h of pair j >> 1 with all 16 channels of the K block,
//   md_split_f16f6, and the four 16-byte stores of the two-phase pass: a wave's store covers 4 runs (one per frequency) of 256 B.
// wpk == NULL: no weights, no MFMAs, no `res` -- a persistent, prefetching form of the plain operand pass.
#include "md_common.h"
#include "md_prep_f6.h"

namespace {
constexpr int BP_ROWS = 128, BP_WAVES = 8, BP_THREADS = BP_WAVES * 64, BP_TILE = BP_WAVES * 32;   // 256 positions per tile

// wave-uniform 64-bit base in SGPRs + one 32-bit byte offset per lane (see nin_stream.hip)
__device__ __forceinline__ uint64_t bp_uniform(const void* p) {
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
typedef uint32_t bp_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const bp_u32x4* bp_gload_t;
typedef __attribute__((address_space(1))) bp_u32x4* bp_gstore_u_t;
typedef __attribute__((address_space(1))) f32x4* bp_gstore_t;
__device__ __forceinline__ uint4 bp_load(uint64_t base, uint32_t off) { return __builtin_bit_cast(uint4, *(bp_gload_t)(base + off)); }
__device__ __forceinline__ void bp_store(uint64_t base, uint32_t off, f32x4 v) { *(bp_gstore_t)(base + off) = v; }
__device__ __forceinline__ void bp_store(uint64_t base, uint32_t off, uint4 v) {
  *(bp_gstore_u_t)(base + off) = __builtin_bit_cast(bp_u32x4, v);
}
__device__ __forceinline__ float bp_pull(int addr, float v) {      // v of lane addr / 4
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, v)));
}
// v of lane - 1 / lane + 1 by a DPP wave shift (wave_shr:1 / wave_shl:1: over all 64 lanes; lane 0 / lane 63 get zero): one
// v_mov_b32_dpp, no LDS-pipe round trip and no lgkmcnt wait.  (The consumer is a select, which the compiler does not give a DPP source.)
__device__ __forceinline__ float bp_from_prev(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float bp_from_next(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, true));
}
}  // namespace

template <int KSTEPS, bool NIN>   // K / 16: 8 (K = 128) or 16 (K = 256)
__global__ __launch_bounds__(BP_THREADS) void md_block_pass_kernel(const uint4* __restrict__ x1, const uint4* __restrict__ x2, int split8,
                                                                   int c1, int c2, const float* __restrict__ ac, int silu,
                                                                   const float* __restrict__ eq, uint4* __restrict__ T,
                                                                   const uint4* __restrict__ wpk, const float* __restrict__ bias,
                                                                   float* __restrict__ res, int64_t P, int W, int n_tiles,
                                                                   int tiles_per_sample) {
  constexpr int GS = 4;                  // 16-channel steps per register set
  constexpr int NG = KSTEPS / GS;        // groups per tile (2 or 4): group g of a tile travels through set g & 1
  constexpr int K = KSTEPS * 16;
  __shared__ __attribute__((aligned(16))) uint4 wl[NIN ? (KSTEPS / 2) * 4 * 2 * BP_ROWS : 1];    // KSTEPS/2 tiles of 16 KB
  __shared__ __attribute__((aligned(16))) float acl[BP_WAVES][2 * K];      // [wave][channel](a, c) of the sample the wave stands in
  __shared__ __attribute__((aligned(16))) float eql[K];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  if constexpr (NIN) {
    for (int i = tid; i < (KSTEPS / 2) * 1024; i += BP_THREADS) wl[i] = wpk[i];
  }
  if (eq != nullptr && tid < K) eql[tid] = eq[tid];
  __syncthreads();
  const unsigned char* wb = (const unsigned char*)wl;
  const int64_t Ph = P >> 1;

  // ---- loop-invariant lane geometry ----
  const int xr = (wid * 32 + j) & (W - 1);                       // x of the lane's position (W is a power of two, rows are whole)
  const bool has_l = xr > 0, has_r = xr < W - 1;                  // the neighbour lies inside the row
  const bool first = j == 0, last = j == 31;                      // ... and outside the wave's segment: the halo
  const bool take_l = has_l && !first, take_r = has_r && !last, use_h = (first && has_l) || (last && has_r);
  const bool no_l = !take_l, no_r = !take_r;
  const bool odd = j & 1;
  // halo holder L = lane & 31 (lanes < 32 load): step hk of the group, channel group hh of its K block, end hend, 16-byte half hq
  const int hk = (lane >> 3) & 3, hh = (lane >> 2) & 1, hend = (lane >> 1) & 1, hq = lane & 1;
  const bool seg_l = ((wid * 32) & (W - 1)) != 0, seg_r = ((wid * 32 + 32) & (W - 1)) != 0;      // wave-uniform: that end has a halo
  const bool hload = lane < 32 && (hend ? seg_r : seg_l);
  const int a_h = (4 * h + 2 * (last ? 1 : 0)) * 4;              // + (8 k + half) * 4: the holder of the lane's halo at step k

  uint4 s0[2 * GS], s1[2 * GS], g0 = make_uint4(0, 0, 0, 0), g1 = g0;
  const uint32_t loff = (uint32_t)(((int64_t)h * P + wid * 32 + j) * 32);
  // group g of tile t -> register set (channel group 2 ks + h of the concatenated input at the lane's position of sample b) and
  // halo register (16 bytes of channel group 2 (g GS + hk) + hh at the position beyond the segment's end hend)
  auto issue = [&](uint4 (&st)[2 * GS], uint4& hreg, int t, int g) {
    const int b = t / tiles_per_sample;
    const int64_t p0 = (int64_t)(t - b * tiles_per_sample) * BP_TILE;
#pragma unroll
    for (int k = 0; k < GS; ++k) {
      const int ks = g * GS + k;
      const uint64_t ub = bp_uniform((2 * ks < split8) ? (const char*)x1 + (((int64_t)b * (c1 >> 3) + 2 * ks) * P + p0) * 32
                                                    : (const char*)x2 + (((int64_t)b * (c2 >> 3) + (2 * ks - split8)) * P + p0) * 32);
      st[2 * k] = bp_load(ub, loff);
      st[2 * k + 1] = bp_load(ub, loff + 16);
    }
    if (hload) {
      const int cg = 2 * (g * GS + hk) + hh;
      const char* src = cg < split8 ? (const char*)x1 + ((int64_t)b * (c1 >> 3) + cg) * P * 32
                                    : (const char*)x2 + ((int64_t)b * (c2 >> 3) + (cg - split8)) * P * 32;
      hreg = *(const uint4*)(src + (p0 + wid * 32 + (hend ? 32 : -1)) * 32 + hq * 16);
    }
  };
  f32x16 acc[NIN ? 4 : 1];
  auto step = [&](int ks, const uint4& r0, const uint4& r1) {      // md_nin_f32_kernel's
    uint32_t hw[4], lw[4];
    md_split2(__uint_as_float(r0.x), __uint_as_float(r0.y), hw[0], lw[0]);
    md_split2(__uint_as_float(r0.z), __uint_as_float(r0.w), hw[1], lw[1]);
    md_split2(__uint_as_float(r1.x), __uint_as_float(r1.y), hw[2], lw[2]);
    md_split2(__uint_as_float(r1.z), __uint_as_float(r1.w), hw[3], lw[3]);
    const bf16x8 bhi = __builtin_bit_cast(bf16x8, make_uint4(hw[0], hw[1], hw[2], hw[3]));
    const bf16x8 blo = __builtin_bit_cast(bf16x8, make_uint4(lw[0], lw[1], lw[2], lw[3]));
    const unsigned char* wt = wb + (ks >> 1) * 16384 + (((2 * (ks & 1) + h) * 2) * BP_ROWS + j) * 16;
#pragma unroll
    for (int rt = 0; rt < (NIN ? 4 : 0); ++rt) {
      const bf16x8 ahi = *(const bf16x8*)(wt + rt * 32 * 16);
      const bf16x8 alo = *(const bf16x8*)(wt + (BP_ROWS + rt * 32) * 16);
      acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, bhi, acc[rt], 0, 0, 0);
      acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, blo, acc[rt], 0, 0, 0);
      acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, bhi, acc[rt], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  const float* aw = acl[wid];
  // `n` consecutive channels from `ch` on (n = 4 or 8), raw -> activated and equalised
  auto activate4 = [&](float (&y)[4], int ch) {
    if (ac != nullptr) {
      const f32x4 p0 = *(const f32x4*)(aw + 2 * ch), p1 = *(const f32x4*)(aw + 2 * ch + 4);
      y[0] = md_prep_act(y[0], p0[0], p0[1], silu);
      y[1] = md_prep_act(y[1], p0[2], p0[3], silu);
      y[2] = md_prep_act(y[2], p1[0], p1[1], silu);
      y[3] = md_prep_act(y[3], p1[2], p1[3], silu);
    }
    if (eq != nullptr) {
      const f32x4 e4 = *(const f32x4*)(eql + ch);
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = md_prep_eq(y[e], e4[e]);
    }
  };
  // the operand items of K block ks at the lane's position; hv: the lane's activated halo values of the group
  auto prep = [&](int ks, int k, const uint4& r0, const uint4& r1, const float (&hv)[4], uint64_t tb) {
    float ya[4] = {__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), __uint_as_float(r0.w)};
    float yb[4] = {__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z), __uint_as_float(r1.w)};
    activate4(ya, 16 * ks + 8 * h);
    activate4(yb, 16 * ks + 8 * h + 4);
    float fa[8], fb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float own = e < 4 ? ya[e] : yb[e - 4];
      asm("" : "+v"(own));      // the transform's operands are values, not products: nothing to contract with
      const float hl = bp_pull(a_h + (8 * k + (e >> 2)) * 4, hv[e & 3]);
      // the neighbour inside the segment, else the halo value where that end of the segment has one, else zero (the conv pads the
      // ACTIVATED tensor).  One `edge` serves both sides: a lane is the first or the last of its segment, and W is even
      const float edge = use_h ? hl : 0.f;
      // lane = 32 h + j: a lane that takes pl (j > 0) / pr (j < 31) finds its neighbour in lane - 1 / lane + 1 of its own half; what
      // the wave-wide shift brings to lanes 0, 31, 32 and 63 is never selected
      const float pl = bp_from_prev(own), pr = bp_from_next(own);
      const float l = no_l ? edge : pl, r = no_r ? edge : pr;
      // even position of its pair: own = d1, l = d0, r = d2 -> f0, f1; odd: own = d2, l = d1, r = d3 -> f2, f3 (f3 = d1 - d3 = l - r)
      const float lr = md_wino_bt(0, l, 0.f, r, 0.f);
      const float f1 = md_wino_bt(1, 0.f, own, r, 0.f);
      const float f2 = md_wino_bt(2, 0.f, l, own, 0.f);
      fa[e] = odd ? f2 : lr;
      fb[e] = odd ? lr : f1;
    }
    __builtin_amdgcn_sched_barrier(0);
    // fa's upper 32 lanes <-> fb's lower 32 lanes: lane (j, h) then holds frequency 2 (j & 1) + h, channels 0-7 in fa, 8-15 in fb
    float t[16];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, fa[e]), __builtin_bit_cast(uint32_t, fb[e]), false, false);
      t[e] = __uint_as_float(sw[0]);
      t[8 + e] = __uint_as_float(sw[1]);
    }
    uint4 h0, h1, q0, q1;
    md_split_f16f6(t, false, 0, h0, h1, q0, q1);
    // T[b][2 ks (+1)][f][plane][Ph] items: f = 2 (j & 1) + h, item = the segment's first pair + (j >> 1)
    const uint32_t voff = (uint32_t)(((int64_t)(2 * (2 * (j & 1) + h)) * Ph + (j >> 1)) * 16);
    const uint32_t plane = (uint32_t)(Ph * 16), group = (uint32_t)(8 * Ph * 16);
    bp_store(tb, voff, h0);
    bp_store(tb, voff + plane, q0);
    bp_store(tb, voff + group, h1);
    bp_store(tb, voff + group + plane, q1);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto consume = [&](uint4 (&st)[2 * GS], const uint4& hreg, int g, int b, int64_t p0) {
    float hv[4] = {__uint_as_float(hreg.x), __uint_as_float(hreg.y), __uint_as_float(hreg.z), __uint_as_float(hreg.w)};
    activate4(hv, 16 * (g * GS + hk) + 8 * hh + 4 * hq);
#pragma unroll
    for (int k = 0; k < GS; ++k) {
      const int ks = g * GS + k;
      if constexpr (NIN) step(ks, st[2 * k], st[2 * k + 1]);
      const uint64_t tb = bp_uniform((const char*)T + ((((int64_t)b * (K / 8) + 2 * ks) * 8) * Ph + ((p0 + wid * 32) >> 1)) * 16);
      prep(ks, k, st[2 * k], st[2 * k + 1], hv, tb);
    }
  };

  int t = blockIdx.x, cur_b = -1;
  if (t < n_tiles) { issue(s0, g0, t, 0); issue(s1, g1, t, 1); }
  for (; t < n_tiles; t += gridDim.x) {
    const int tn = t + gridDim.x;
    const int b = t / tiles_per_sample;
    const int64_t p0 = (int64_t)(t - b * tiles_per_sample) * BP_TILE;
    if (ac != nullptr && b != cur_b) {
      // the wave's copy of the sample's (a, c) pairs; the wave's own LDS accesses execute in order
      cur_b = b;
      const f32x4* src = (const f32x4*)(ac + (int64_t)b * 2 * K);
      for (int i = 0; i < 2 * K / 4 / 64; ++i) *(f32x4*)(acl[wid] + (i * 64 + lane) * 4) = src[i * 64 + lane];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if constexpr (NIN) {
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rt][r] = 0.f;
      }
    }
    // a pair of groups per iteration (set 0, set 1): consume a group, then refill its set with the group two ahead (this tile's
    // g + 2, or the next tile's g + 2 - NG).  Not unrolled over the pairs: eight steps of code stay inside the instruction cache
#pragma unroll 1
    for (int gc = 0; gc < NG; gc += 2) {
      int g = gc;
      asm volatile("" : "+s"(g));      // a run-time value also where NG = 2: with constant K blocks the eq reads of all steps are hoisted out of the tile loop
      const bool same = g + 2 < NG;
      const bool more = same || tn < n_tiles;
      const int ti = same ? t : tn, gi = same ? g + 2 : g + 2 - NG;
      consume(s0, g0, g, b, p0);
      if (more) issue(s0, g0, ti, gi);
      __builtin_amdgcn_sched_barrier(0);
      consume(s1, g1, g + 1, b, p0);
      if (more) issue(s1, g1, ti, gi + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (NIN) {
      // epilogue: + bias, 16-byte stores into the F32B layout (4 consecutive channels of one position per lane)
      const uint32_t soff = (uint32_t)((wid * 32 + j) * 32 + 16 * h);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = rt * 32 + 8 * q + 4 * h;
          const f32x4 bv = *(const f32x4*)(bias + row);
          f32x4 o4;
#pragma unroll
          for (int e = 0; e < 4; ++e) o4[e] = acc[rt][q * 4 + e] + bv[e];
          const uint64_t ub = bp_uniform((char*)res + (((int64_t)b * (BP_ROWS / 8) + rt * 4 + q) * P + p0) * 32);
          bp_store(ub, soff, o4);
        }
    }
  }
}

template <int KSTEPS, bool NIN>
static void bp_launch(int blocks, hipStream_t st, const float* x1, const float* x2, int c1, int c2, const float* ac, int silu, const float* eq,
                      void* T, const void* wpk, const float* bias, float* res, int64_t P, int W, int n_tiles) {
  hipLaunchKernelGGL((md_block_pass_kernel<KSTEPS, NIN>), dim3((unsigned)blocks), dim3(BP_THREADS), 0, st, (const uint4*)x1, (const uint4*)x2,
                     c1 >> 3, c1, c2, ac, silu, eq, (uint4*)T, (const uint4*)wpk, bias, res, P, W, n_tiles, (int)(P / BP_TILE));
}

extern "C" int md_wino_prep_f6_nin(const float* x1, const float* x2, int32_t c1, int32_t c2, const float* ac, int32_t silu, const float* eq,
                                   void* t_out, const void* wpk, const float* bias, float* res, int32_t batch, int32_t D, int32_t H,
                                   int32_t W, int32_t n_cu, void* stream) {
  // md_wino_prep_f6's checks, then md_nin_f32's
  if (!x1 || !t_out || batch <= 0 || c1 <= 0 || c2 < 0 || (c1 & 15) || (c2 & 15) || (c2 > 0 && !x2)) return MD_ERR_BAD_ARG;
  if (silu && !ac) return MD_ERR_BAD_ARG;
  if (D <= 0 || H <= 0 || W <= 0 || (W & 1)) return MD_ERR_BAD_ARG;
  if (wpk && (!bias || !res)) return MD_ERR_BAD_ARG;
  const int64_t P = (int64_t)D * H * W;
  if ((BP_TILE % W) || (P % BP_TILE)) return MD_ERR_UNSUPPORTED;      // whole rows per tile
  const int K = c1 + c2;
  if (K != 128 && K != 256) return MD_ERR_UNSUPPORTED;
  if (P > ((int64_t)1 << 25)) return MD_ERR_UNSUPPORTED;              // 32-bit lane offsets into a (sample, K block) of T
  const int64_t n_tiles64 = (int64_t)batch * (P / BP_TILE);
  if (n_tiles64 > 0x7fffffff) return MD_ERR_UNSUPPORTED;
  const int n_tiles = (int)n_tiles64;
  int blocks = n_cu > 0 ? n_cu : 256;
  if (blocks > n_tiles) blocks = n_tiles;
  hipStream_t st = (hipStream_t)stream;
  MD_HIP_CLEAR_ERROR();
  if (wpk) {
    if (K == 256) bp_launch<16, true>(blocks, st, x1, x2, c1, c2, ac, silu, eq, t_out, wpk, bias, res, P, W, n_tiles);
    else bp_launch<8, true>(blocks, st, x1, x2, c1, c2, ac, silu, eq, t_out, wpk, bias, res, P, W, n_tiles);
  } else {
    if (K == 256) bp_launch<16, false>(blocks, st, x1, x2, c1, c2, ac, silu, eq, t_out, wpk, bias, res, P, W, n_tiles);
    else bp_launch<8, false>(blocks, st, x1, x2, c1, c2, ac, silu, eq, t_out, wpk, bias, res, P, W, n_tiles);
  }
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
