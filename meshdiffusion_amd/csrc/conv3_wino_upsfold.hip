// The Upsample conv with its nearest-x2 taps folded into the weights (inference, f16f6 arithmetic).
//
// Reference op: nn.Conv3d 3x3x3 pad 1 on the nearest-x2 upsampled input (lib/diffusion/models/layers.py:618-623).
//
// Along an upsampled axis two of a position's three taps hit the same source value.  Output plane Z = 2z + a reads source planes
// z - 1 (kd = 0) and z (kd = 1, 2) for a = 0, z (kd = 0, 1) and z + 1 (kd = 2) for a = 1; the same along y with Y = 2y + b.  So for
// each of the four phases p = 2a + b the conv is a 2 x 2 (d, h) x 3 (w) conv on the SOURCE rows with pre-summed weights
// (layers.fold_upsample_weight: rows p * Cout + co of a [4 Cout][Cin][3][3][3] tensor whose five dead (kd', kh') taps are zero,
// packed by md_wino_pack_weights_f6 like any other weight): 4 live taps instead of 9, 8 matrix-core units per output instead of 18,
// same Winograd F(2,3) along w.  The operand is the T md_wino_prep_upsdh / md_wino_prep_f6 (ups) already writes: one row per source
// (z', y') in the compact layout, rows (2z', 2y') of the full one -- the same bits either way.
//
// Geometry of md_conv3_wino_kernel<0, true, true, false> (conv3_wino.hip, which documents it): one workgroup = 128 rows x (4 x 8
// SOURCE rows x 8 full-resolution x) of one phase, wave f owns frequency f, a halo image [h][plane][dz][hy][pair 4] on the source
// grid, the same fragment reads and the same epilogue exchange.  What differs:
//   rows     row block rtb = blockIdx-derived: phase p = rtb / (Cout / 128), channel block rtb % (Cout / 128); bias, GroupNorm sums
//            and the output channel use the channel block
//   steps    sequence chunk * 4 + i with tap (a + (i >> 1)) * 3 + (b + (i & 1)); the weight image keeps its 9-tap layout (step_of_9 =
//            chunk * 9 + tap, pair p9 = step_of_9 / 2): the two steps of a pair-step are adjacent taps but may sit in two pairs of the
//            image, so the K-concatenated f6 fragment is read per lane half (lane (row, h) takes step + h from pair (step + h) / 2, lane
//            half (step + h) & 1), the fp16 fragments are piece step & 1 of pair step / 2
//   halo     a chunk lasts 2 pair-steps = 8 groups instead of 4.5 pair-steps, so the halo must arrive 2.25 times as fast from the same
//            registers in flight.  The image holds only the 5 x 9 (dz, hy) rows the phase's 2 x 2 live taps read (origin = its first
//            live tap): 12 pieces of 1 KB instead of 15; groups 2 and 3 of a pair-step store three pieces of the next chunk each and
//            request, into the slots just stored, the same pieces of the chunk after it (UF_RING = 12 in flight, a whole chunk ahead),
//            behind the weight loads of groups 0 and 1 in the memory queue
//   output   column tile ct / halo row hy of phase (a, b) goes to output row Z = 2 (z0' + ct) + a, Y = 2 (y0' + hy) + b; x contiguous
#include <type_traits>
#include "md_common.h"

namespace {
constexpr int UF_THREADS = 256;
constexpr int UF_TZ = 4, UF_TY = 8, UF_TX = 8;          // tile: 4 x 8 source rows, 8 x (4 pairs)
// The halo image of a phase holds only the rows its 2 x 2 live taps read: 5 of the 6 planes, 9 of the 10 rows
constexpr int UF_TPOS = 5 * 9 * 4;                       // 180 transformed halo entries (dz, hy, pair) per (k-group, plane)
constexpr int UF_ENTRIES = 4 * UF_TPOS;                  // 720 entries of 16 B: [h 2][plane 2][180] = one chunk of one frequency
constexpr int UF_HBUF = UF_ENTRIES * 16;                 // 11520 B
constexpr int UF_NDMA = (UF_ENTRIES + 63) / 64;          // 12 pieces of 64 entries (one per lane) per chunk and wave; the last one holds 16
constexpr int UF_RED = 4 * 32 * 2;                       // floats: [wave][channel][sum, sumsq]
constexpr int UF_WAVE_LDS = 2 * UF_HBUF;                 // two halo buffers per wave
constexpr int UF_LDS_BYTES = 138240;                     // as md_conv3_wino_kernel: the epilogue's exchange area (133632 B) is what sizes it; the halo
                                                         // buffers (92160 B) and the offset tables (12288 B) lie inside it
static_assert(4 * UF_WAVE_LDS + 4 * UF_NDMA * 64 * 4 <= UF_LDS_BYTES, "halo buffers + offset tables");
#ifndef UF_RING
#define UF_RING 12    // halo pieces in flight per wave (4 registers each): a piece is requested where the one UF_RING pieces before it in the
#endif                // stream is stored; 12 = a whole chunk (8 groups, two pair-steps) ahead, the 48 registers the 9-tap loop spends
static_assert(UF_RING == 12 || UF_RING == 6, "the slot ring closes over one body of 24 pieces and a group's requests lie in one chunk");

typedef uint32_t uf_u32x4 __attribute__((ext_vector_type(4)));
typedef int uf_i32x8 __attribute__((ext_vector_type(8)));
typedef int uf_i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 uf_gload16(const void* p) {      // through the GLOBAL address space (see wn_gload16)
  return __builtin_bit_cast(uint4, *(__attribute__((address_space(1))) const uf_u32x4*)(uintptr_t)p);
}

__device__ __forceinline__ uint4 uf_gload16_at(const void* base, uint32_t byte_off) {      // wave-uniform base + 32-bit lane offset
  return uf_gload16((const unsigned char*)base + byte_off);
}

struct UfArgs {
  const uint4* T;          // [B][cin/8][4][2][D/2 << s][H/2 << s][W/2] items of 16 B
  const uint4* wpk;        // md_wino_pack_weights_f6 of the folded [4 cout][cin][27] tensor
  float* out;              // F32B [B][cout/8][D H W][8]
  const float* bias;       // may be null; per sample with stride bias_bstride (0 = shared)
  double* stats;           // may be null
  const float* hdr;        // the weight buffer's header {max |w|, sw, 2^-sw}
  int64_t bias_bstride;
  int batch, cin, cout, D, H, W;      // cout: the conv's (a quarter of the packed rows); D, H, W: the OUTPUT grid
  int sh;                  // 0: T is the compact operand, 1: the full upsampled one (row (z', y') of the source at (2z', 2y'))
};
}  // namespace

__global__ __launch_bounds__(UF_THREADS) void md_conv3_wino_upsfold_kernel(const UfArgs A) {
  __shared__ __attribute__((aligned(16))) unsigned char uf_smem[UF_LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);       // = frequency f of this wave
  const int j = lane & 31, h = lane >> 5;
  const int D = A.D, H = A.H, W = A.W, Wp = W >> 1;
  const int Ds = D >> 1, Hs = H >> 1;                              // the source grid
  const int64_t P = (int64_t)D * H * W;
  const int ush = A.sh, Hrows = Hs << ush;
  const int Phi = (Ds * Hs * Wp) << (2 * ush);                     // items per (frequency, plane) slice of T (16 Ph < 2^31: checked at launch)
  const int ntx = W / UF_TX, nty = Hs / UF_TY, ntz = Ds / UF_TZ;
  const int tiles = ntx * nty * ntz;
  const int ncb = A.cout >> 7;
  // XCD-aware order: one contiguous run per XCD (block b runs on XCD b % 8); inside it the four phases of one source tile are
  // adjacent (T is read four times: three of them out of L2), then the tiles, the samples and the channel blocks
  int bid = blockIdx.x;
  if ((gridDim.x & 7) == 0) bid = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  int ph = bid & 3, lin = bid >> 2;
#ifndef UF_ORDER
#define UF_ORDER 0      // A/B: 1 = phase-major inside blocks of UF_NG tiles (an XCD's 32 CUs then run ONE phase at a time: a quarter of the weights live)
#endif
#ifndef UF_NG
#define UF_NG 32
#endif
  if constexpr (UF_ORDER == 1) {
    if ((gridDim.x >> 2) % UF_NG == 0) {
      const int grp = bid / (4 * UF_NG), r = bid % (4 * UF_NG);
      ph = r / UF_NG;
      lin = grp * UF_NG + r % UF_NG;
    }
  }
  const int pa = ph >> 1, pb = ph & 1;
  const int t = lin % tiles, rest = lin / tiles;
  const int b = rest % A.batch, cb = rest / A.batch;
  const int x0 = (t % ntx) * UF_TX, y0 = ((t / ntx) % nty) * UF_TY, z0 = (t / (ntx * nty)) * UF_TZ;      // y0, z0: source rows
  const int rtb = ph * ncb + cb;                                   // 128-row block of the folded weights
  const int CG = A.cin >> 3, nchunk = A.cin >> 4;
  const int npairs9 = (nchunk * 9) >> 1;                           // pairs of the 9-tap weight image (nchunk is even)

  unsigned char* my_smem = uf_smem + wid * UF_WAVE_LDS;

  // halo piece k = entries [64 k, 64 k + 64) of the linear image [h][plane][dz][hy][pair]; source offset in items relative to the
  // (sample, chunk, freq) base, -1 = outside the source grid (zero)
  auto halo_off = [&](int k) -> int {
    const int e = k * 64 + lane;
    const int hp = e / UF_TPOS, tp = e % UF_TPOS;
    const int dz = tp / 36, hy = (tp >> 2) % 9, pr = tp & 3;
    const int z = z0 + pa + dz - 1, y = y0 + pb + hy - 1;          // the phase's first live tap is the image's origin
    const bool live = (e < UF_ENTRIES) & (z >= 0) & (z < Ds) & (y >= 0) & (y < Hs);
    const int row = (z << ush) * Hrows + (y << ush);
    const int off = (hp >> 1) * 8 * Phi + (hp & 1) * Phi + row * Wp + (x0 >> 1) + pr;
    return live ? off : -1;
  };
  const uint4* tbase = A.T + ((int64_t)b * CG * 8 + wid * 2) * Phi;                              // + chunk * 16 * Ph

  f32x16 acc[4][4];
  auto zero_acc = [&]() {
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rt][ct][r] = 0.f;
        asm volatile("" : "+a"(acc[rt][ct]));          // the 256 accumulator registers are the AccVGPR half of the file
      }
  };

  // ---- main loop ----------------------------------------------------------------------------------------------------------
  // A body = 2 chunks (c0 in halo buffer 0, c0 + 1 in buffer 1) = 4 pair-steps u = 16 groups g = 4 u + ct.  Pair-step u of chunk
  // c0 + (u >> 1) is the taps kd' = a + (u & 1), kh' = b + {0, 1}.  Group g (12 MFMAs as in the 9-tap loop):
  // The 12 halo pieces of a chunk are carried by groups of the chunk before it (UF_HSCHED below: three pieces in each of the groups
  // 2 and 3 of its two pair-steps).  Pieces form one stream q = 12 * chunk + piece over a ring of UF_RING slots.
  //   pass 0 (fp16, step 0)  stores its pieces of chunk c0 + (g >> 3) + 1 into the OTHER buffer (free: its last readers were issued one
  //                          group before the chunk began; its first reader is the fragment read of group 7 / 15, behind that group's
  //                          store), then reads the fragments of group g + 1
  //   pass 1 (fp16, step 1)  requests the pieces UF_RING further down the stream into the slots just stored; reads the offsets of
  //                          group g + 1's requests out of the table
  //   pass 2 (f6, both)      groups 0, 1: the 16 weight pieces of the next pair-step
  const uint4* wbase = A.wpk + (((int64_t)rtb * npairs9) * 4 + wid) * 1024;      // + pair * 4096 + (row tile * 4 + piece) * 64 + lane
  uint4 A8h[2][4][2], B8h[2][2], hs[UF_RING];
  uf_i32x8 A8f[2][4], B8f[2];
  uint32_t* otab = (uint32_t*)(uf_smem + 4 * UF_WAVE_LDS) + wid * (UF_NDMA * 64) + lane;
  uint32_t live_mask = 0;
  unsigned char* dump = uf_smem + 4 * UF_WAVE_LDS + 4 * UF_NDMA * 64 * 4 + tid * 16;      // 4 KB behind the offset tables
  static_assert(4 * UF_WAVE_LDS + 4 * UF_NDMA * 64 * 4 + UF_THREADS * 16 <= UF_LDS_BYTES, "dump slots");
  const unsigned char* vBh = my_smem + h * 2 * UF_TPOS * 16 + j * 16;                     // k-group h, plane 0 (fp16)
  const unsigned char* vB8 = my_smem + UF_TPOS * 16 + j * 16 + h * 64;                    // k-group 0, plane 1 (f6), step + h (kh' + h)
  auto cat8 = [](const uint4& x, const uint4& y) -> uf_i32x8 {
    const uf_i32x4 a = __builtin_bit_cast(uf_i32x4, x), c = __builtin_bit_cast(uf_i32x4, y);
    return __builtin_shufflevector(a, c, 0, 1, 2, 3, 4, 5, 6, 7);
  };
  auto halo_store8 = [&](int buf, int k, uint4 v) {
    const bool lv = (live_mask >> k) & 1u;
    v.x = lv ? v.x : 0u; v.y = lv ? v.y : 0u; v.z = lv ? v.z : 0u; v.w = lv ? v.w : 0u;
    // the last piece is 16 entries: the other lanes would write into the next buffer and go to a dump slot instead (a select on the
    // address: a branch would split the loop's one basic block)
    unsigned char* dst = my_smem + buf * UF_HBUF + k * 1024 + lane * 16;
    if (k == UF_NDMA - 1) dst = lane < UF_ENTRIES - (UF_NDMA - 1) * 64 ? dst : dump;
    *(uint4*)dst = v;
  };
  auto read_B8 = [&](auto gc, uint4 (&dh)[2], uf_i32x8& df) {       // fragments of group g (of any body)
    constexpr int g = decltype(gc)::value & 15;
    constexpr int o0 = (g >> 3) * UF_HBUF + ((g & 3) + ((g >> 2) & 1)) * 36 * 16;      // entry (ct + ul) * 36 + 4 i + j, i = step of the pair
    dh[0] = *(const uint4*)(vBh + o0);
    dh[1] = *(const uint4*)(vBh + o0 + 64);
    df = cat8(*(const uint4*)(vB8 + o0), *(const uint4*)(vB8 + o0 + 2 * UF_TPOS * 16));
  };
  const uint32_t lane_b = lane * 16, lane_odd = h ? 4096 * 16 + j * 16 : (j + 32) * 16;      // byte offsets of the lane's weight item
  auto load_A8 = [&](int chunk, int ul, int set, int rt0, int nrt) {      // row tiles rt0 .. rt0 + nrt - 1 of pair-step (chunk, ul)
    const int s0 = chunk * 9 + (pa + ul) * 3 + pb, s1 = s0 + 1;            // steps of the 9-tap image (wave-uniform)
    // every address = a wave-uniform pointer + a 32-bit lane offset (one loop-invariant register each; 64-bit lane pointers per row
    // tile and piece cost 20 registers that the loop does not have)
    const uint4* w0 = wbase + (int64_t)(s0 >> 1) * 4096 + (s0 & 1) * 64;
    const uint4* w1 = wbase + (int64_t)(s1 >> 1) * 4096 + (s1 & 1) * 64;
    // the K-concatenated fragment: lane half h takes step s0 + h.  s0 even: both halves of pair s0 / 2, the lane's own item; s0 odd:
    // h = 0 the upper lane half of pair s0 / 2, h = 1 the lower half of the next pair
    const uint4* wf = wbase + (int64_t)(s0 >> 1) * 4096;
    const uint32_t lf = (s0 & 1) ? lane_odd : lane_b;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
      if (rt >= rt0 && rt < rt0 + nrt) {
        A8h[set][rt][0] = uf_gload16_at(w0 + rt * 256, lane_b);
        A8h[set][rt][1] = uf_gload16_at(w1 + rt * 256, lane_b);
        A8f[set][rt] = cat8(uf_gload16_at(wf + (rt * 4 + 2) * 64, lf), uf_gload16_at(wf + (rt * 4 + 3) * 64, lf));
      }
  };
  // ---- prologue (order fenced as in md_conv3_wino_kernel): weights of pair-step 0, chunk 0 -> buffer 0, the first UF_RING pieces
  // of chunk 1 into the slots, the offset table; the accumulators are zeroed while the requests are in flight ----
  float descale;
  {
    uint4 h0[UF_NDMA];
    load_A8(0, 0, 0, 0, 4);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < UF_NDMA; ++k) {
      const int dk = halo_off(k);
      const uint32_t o = dk >= 0 ? (uint32_t)dk : 0u;      // outside the grid: a valid address, zeroed on its way to LDS
      live_mask |= (dk >= 0 ? 1u : 0u) << k;
      otab[k * 64] = o;
      h0[k] = uf_gload16(tbase + o);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int k = 0; k < UF_RING; ++k) hs[k] = uf_gload16(tbase + (int64_t)16 * Phi + otab[k * 64]);
    __builtin_amdgcn_sched_barrier(0);
    zero_acc();
    descale = A.hdr[2];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < UF_NDMA; ++k) halo_store8(0, k, h0[k]);
  }
  read_B8(std::integral_constant<int, 0>{}, B8h[0], B8f[0]);
  uint32_t off_next[3] = {0u, 0u, 0u};                     // source offsets of the next group's requests, read one group ahead
  // UF_HSCHED: which groups carry the halo pieces.  0: every group (2 in an even, 1 in an odd one) -- measured 0.75 of the 9-tap loop's
  // time per chunk instead of 4 / 9: groups 0 and 1 then request HBM-latency halo lines right in front of their weight loads, loads
  // return in order, and the wait for the weights one pair-step later covers them.  1: groups 2 and 3 of a pair-step, three pieces
  // each, BEHIND the weight loads of groups 0 and 1 in the memory queue (as the 9-tap loop places them).
#ifndef UF_HSCHED
#define UF_HSCHED 1
#endif
  // first piece (stream position relative to the body's first: (g >> 3) * 12 + piece) and piece count of group g (of any body)
  auto first_of = [](int g) constexpr -> int {
    return UF_HSCHED ? (((g & 15) >> 3) * 12) + ((((g & 7) >> 2) * 2 + ((g & 3) - 2)) * 3) : (((g & 15) >> 3) * 12) + (((g & 7) >> 1) * 3) + (g & 1) * 2;
  };
  auto count_of = [](int g) constexpr -> int { return UF_HSCHED ? ((g & 3) >= 2 ? 3 : 0) : 2 - (g & 1); };
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (i < count_of(0)) off_next[i] = otab[((first_of(0) + i + UF_RING) % 12) * 64];
  auto body = [&](int c0) {
    auto group = [&](auto gc) {
      constexpr int g = decltype(gc)::value, u = g >> 2, ct = g & 3, cl = g >> 3;
      constexpr int aset = u & 1, bset = ct & 1;
      // -- pass 0
      constexpr int n_st = count_of(g), q0 = n_st ? first_of(g) : 0;      // stream positions q0 ..: pieces q0 % 12 .. of chunk c0 + cl + 1
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i < n_st) halo_store8(cl ^ 1, (q0 + i) % 12, hs[(q0 + i) % UF_RING]);
      read_B8(std::integral_constant<int, g + 1>{}, B8h[bset ^ 1], B8f[bset ^ 1]);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A8h[aset][rt][0]), __builtin_bit_cast(f16x8, B8h[bset][0]),
                                                             acc[rt][ct], 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      if constexpr (n_st > 0) __builtin_amdgcn_sched_group_barrier(0x200, n_st, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      __builtin_amdgcn_sched_barrier(0);
      // -- pass 1: stream positions q0 + UF_RING, + 1 = pieces (..) % 12 of chunk c0 + 1 + (..) / 12.  A chunk that does not exist is
      //    clamped to the last one with the offsets masked to zero (every lane reads ONE resident line; the data is stored into a
      //    buffer nobody reads any more), so that the loop stays one basic block
      constexpr int r0 = q0 + UF_RING, n_ld = n_st;
      static_assert(n_ld == 0 || r0 / 12 == (r0 + n_ld - 1) / 12, "a group's requests lie in one chunk");
      constexpr int n_rd = count_of(g + 1), qn = n_rd ? first_of(g + 1) + UF_RING : 0;      // only the piece index (% 12) is used
      if constexpr (n_ld > 0) {
        const int cw = c0 + 1 + r0 / 12;
        const bool there = cw < nchunk;
        const uint4* cbp = tbase + (int64_t)(there ? cw : nchunk - 1) * 16 * Phi;
        const uint32_t om = there ? ~0u : 0u;
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (i < n_ld) hs[(q0 + i) % UF_RING] = uf_gload16(cbp + (off_next[i] & om));
      }
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i < n_rd) off_next[i] = otab[((qn + i) % 12) * 64];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A8h[aset][rt][1]), __builtin_bit_cast(f16x8, B8h[bset][1]),
                                                             acc[rt][ct], 0, 0, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      if constexpr (n_ld > 0) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      if constexpr (n_ld > 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      if constexpr (n_ld > 2) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      if constexpr (n_rd > 0) __builtin_amdgcn_sched_group_barrier(0x100, n_rd, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_barrier(0);
      // -- pass 2: in groups 0 and 1 the 16 weight pieces of the next pair-step (clamped at the end: the redundant request is never used)
      if constexpr (ct < 2) {
        const int cn = c0 + ((u + 1) >> 1);
        const bool there = cn < nchunk;
        load_A8(there ? cn : nchunk - 1, there ? ((u + 1) & 1) : 1, aset ^ 1, ct * 2, 2);
      }
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        acc[rt][ct] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A8f[aset][rt], B8f[bset], acc[rt][ct], 2, 2, 0, A8f[aset][rt][6], 0,
                                                                      B8f[bset][6]);
      if constexpr (ct < 2) {
#pragma unroll
        for (int i_ = 0; i_ < 4; ++i_) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    group(std::integral_constant<int, 0>{}); group(std::integral_constant<int, 1>{}); group(std::integral_constant<int, 2>{});
    group(std::integral_constant<int, 3>{}); group(std::integral_constant<int, 4>{}); group(std::integral_constant<int, 5>{});
    group(std::integral_constant<int, 6>{}); group(std::integral_constant<int, 7>{}); group(std::integral_constant<int, 8>{});
    group(std::integral_constant<int, 9>{}); group(std::integral_constant<int, 10>{}); group(std::integral_constant<int, 11>{});
    group(std::integral_constant<int, 12>{}); group(std::integral_constant<int, 13>{}); group(std::integral_constant<int, 14>{});
    group(std::integral_constant<int, 15>{});
  };
  for (int c0 = 0; c0 < nchunk; c0 += 2) body(c0);

  // ---- epilogue: md_conv3_wino_kernel's (exchange area, lane roles and bank layout documented there; tests/test_cpu_kernel_layouts.py)
  // with the output rows of this phase ------------------------------------------------------------------------------------------
  constexpr int XF_ITEMS = 1024, XREG_FLOATS = (4 * XF_ITEMS + 16) * 4;
  static_assert(2 * XREG_FLOATS * 4 + 2 * UF_RED * 4 <= UF_LDS_BYTES, "two exchange regions + the statistics area fit");
  float* xreg = (float*)uf_smem;
  float* red = xreg + 2 * XREG_FLOATS;
  const int rows_total = A.cout;
  float* outp = A.out + (int64_t)b * rows_total * P;
  const float* biasp = A.bias ? A.bias + (int64_t)b * A.bias_bstride : nullptr;
  const bool want_stats = A.stats != nullptr;
  const int half = lane & 1, xq = (lane >> 1) & 7, cgp = lane >> 4;      // read side
  const int cq = 2 * cgp + half, prr = xq >> 1;
  const bool odd = xq & 1;                                                // y1 lanes
  const float sgn = odd ? -1.f : 1.f;
  // positions: this wave finishes column tile wid = source plane z0 + wid -> output plane 2 (z0 + wid) + a; source row y0 + yr ->
  // output row 2 (y0 + yr) + b; x = x0 + xq
  const int64_t gp0 = ((int64_t)(2 * (z0 + wid) + pa) * H + 2 * y0 + pb) * W + x0 + xq;
  const int64_t ystride = (int64_t)2 * W * 8;
  auto flush_stats = [&](int r) {     // after the barrier that follows round r's red[] writes: 64 fp64 atomics
    if (tid < 64) {
      const int ch = tid >> 1, which = tid & 1;
      const float* rb = red + (r & 1) * UF_RED;
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) sum += rb[(k * 32 + ch) * 2 + which];
      const int row = cb * 128 + r * 32 + ch;
      atomicAdd(A.stats + ((int64_t)b * rows_total + row) * 2 + which, (double)sum);
    }
  };
  const bool has_bias = biasp != nullptr;
  f32x4 pbias[4];
  {
    const float* bsrc = has_bias ? biasp : (const float*)A.wpk;      // always a valid address: the value is dropped at its use
#pragma unroll
    for (int r = 0; r < 4; ++r) pbias[r] = *(const f32x4*)(bsrc + cb * 128 + r * 32 + 4 * cq);
  }
  auto row_sum8 = [](float v) {       // over the 8 lanes of a DPP row with the same lane & 1 (row_ror 8, 4, 2)
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xF, 0xF, true));
    return v;
  };
  const int sj = ((j & 1) << 2) | ((j >> 1) & 3);
  const int wbase_items = wid * XF_ITEMS + (wid == 2 ? 8 : (wid == 3 ? 16 : 0)) + j * 8;
  auto write_round = [&](int r) {
    float* xw = xreg + (r & 1) * XREG_FLOATS;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float* pq = xw + (wbase_items + ((2 * q + h) ^ sj)) * 4;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[r][ct][q * 4 + e];
        *(f32x4*)(pq + ct * 32 * 8 * 4) = v;
      }
    }
  };
  const int rcol_items = (wid * 32 + prr) * 8;
  const int rx0 = cq ^ (((prr & 1) << 2) | (prr >> 1)), rx1 = rx0 ^ 2;                       // rows yr even / odd
  const int offA = odd ? 2 * XF_ITEMS + 8 : 0, offC = odd ? 3 * XF_ITEMS + 16 : 2 * XF_ITEMS + 8;   // y0: m0, m1, m2; y1: m2, m1, m3
  __syncthreads();                                       // every wave is done with its private buffers (the exchange area aliases them)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float* xr = xreg + (r & 1) * XREG_FLOATS;
    if (r == 0) write_round(r);
    __syncthreads();
    f32x4 mA[8], mB[8], mC[8];
#pragma unroll
    for (int yr = 0; yr < 8; ++yr) {
      const float* pbx = xr + (rcol_items + yr * 32 + ((yr & 1) ? rx1 : rx0)) * 4;
      mA[yr] = *(const f32x4*)(pbx + offA * 4);
      mB[yr] = *(const f32x4*)(pbx + XF_ITEMS * 4);
      mC[yr] = *(const f32x4*)(pbx + offC * 4);
    }
    if (want_stats && r > 0) flush_stats(r - 1);
    if (r < 3) {      // round r + 1's accumulators follow this round's reads into the LDS queue (the other region's readers are behind the barrier)
      __builtin_amdgcn_sched_barrier(0);
      write_round(r + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    float* op = outp + ((int64_t)(cb * 16 + r * 4 + cgp) * P + gp0) * 8 + 4 * half;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const f32x4 bv = has_bias ? pbias[r] : zero4;
    f32x4 s1 = zero4, s2 = s1;
#pragma unroll
    for (int yr = 0; yr < 8; ++yr) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // y0 = (m1 + m0) + m2, y1 = (m1 - m2) - m3: one code path, the sign is the lane's (exact: fma with +-1)
        const float y = __builtin_fmaf(sgn, mC[yr][e], __builtin_fmaf(sgn, mA[yr][e], mB[yr][e]));
        o[e] = y * descale + bv[e];       // the accumulators hold 2^sw x the products (the weights' pre-scale): an exact power of two
      }
      *(f32x4*)(op + yr * ystride) = o;
      s1 += o;
      s2 += o * o;
    }
    if (want_stats) {
      f32x4 a1, a2;
#pragma unroll
      for (int e = 0; e < 4; ++e) { a1[e] = row_sum8(s1[e]); a2[e] = row_sum8(s2[e]); }
      if ((lane & 14) == 0) {         // one lane per channel quad: 8 consecutive floats of red[]
        float* rb = red + (r & 1) * UF_RED + (wid * 32 + 4 * cq) * 2;
        const f32x4 w0 = {a1[0], a2[0], a1[1], a2[1]}, w1 = {a1[2], a2[2], a1[3], a2[3]};
        *(f32x4*)rb = w0;
        *(f32x4*)(rb + 4) = w1;
      }
    }
  }
  if (want_stats) {
    __syncthreads();
    flush_stats(3);
  }
}

extern "C" int md_conv3_wino_upsfold(int32_t fmt, const void* t_in, int32_t t_full, const void* wpk, float* out, const float* bias,
                                     int64_t bias_bstride, const float* residual, int64_t res_bstride, double* stats, int32_t batch,
                                     int32_t cin, int32_t cout, int32_t D, int32_t H, int32_t W, void* stream) {
  if (!t_in || !wpk || !out || batch <= 0) return MD_ERR_BAD_ARG;
  if (fmt != MD_WINO_FMT_F16F6 || residual != nullptr) return MD_ERR_UNSUPPORTED;      // f16f6, no residual operand: what an Upsample conv is
  (void)res_bstride;
  if (cin <= 0 || cout <= 0 || (cin % 32) || (cout % 128)) return MD_ERR_UNSUPPORTED;
  if (D <= 0 || H <= 0 || W <= 0 || (D % (2 * UF_TZ)) || (H % (2 * UF_TY)) || (W % UF_TX)) return MD_ERR_UNSUPPORTED;
  if ((int64_t)D * H * W * 8 >= (int64_t)1 << 31) return MD_ERR_UNSUPPORTED;       // 32-bit halo offsets (16 Ph items of the full layout)
  const int64_t wgs = (int64_t)(D / (2 * UF_TZ)) * (H / (2 * UF_TY)) * (W / UF_TX) * batch * 4 * (cout / 128);
  if (wgs > 0x7fffffff) return MD_ERR_UNSUPPORTED;
  UfArgs a;
  a.T = (const uint4*)t_in; a.wpk = (const uint4*)wpk; a.out = out; a.bias = bias; a.stats = stats;
  a.hdr = (const float*)((const unsigned char*)wpk + (int64_t)4 * cout * cin * 36 * 4);
  a.bias_bstride = bias_bstride;
  a.batch = batch; a.cin = cin; a.cout = cout; a.D = D; a.H = H; a.W = W;
  a.sh = t_full ? 1 : 0;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_conv3_wino_upsfold_kernel, dim3((unsigned)wgs), dim3(UF_THREADS), 0, (hipStream_t)stream, a);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
