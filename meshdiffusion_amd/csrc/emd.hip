// Generation metrics under the earth mover's distance: the all-pairs matrix
//     out[i][j] = (1/p) * min over permutations pi of sum_k |x[i][k] - y[j][pi(k)]|,      x [nx][p][3], y [ny][p][3], out [nx][ny],
// the cost being the Euclidean distance (not its square).  The reference tree has no EMD and no implementation was consulted;
// the oracle of the tests is scipy's linear_sum_assignment (tests/emd_cases.py).
//
// THE EMD CONTRACT (include/meshdiffusion_hip.h states it too).  The result is a function of the inputs alone:
//   distance   d = sqrtf(dz*dz + (dy*dy + dx*dx)) in fp32, no contraction, a correctly rounded square root (hipcc's default,
//              -fhip-fp32-correctly-rounded-divide-sqrt); symmetric in its two points.
//   integer    q = rint(d / quantum), quantum a power of two handed in by the host, one per call; d / quantum >= 2^21 anywhere in a
//              pair makes the pair NaN with status 2.
//   solver     the integer assignment problem on q is solved EXACTLY: a forward auction (Bertsekas) with eps-scaling on the costs
//              C = q (p + 1), the last phase at eps = 1 -- an assignment that satisfies eps-complementary slackness is within p eps
//              of the optimum, and p < p + 1 is less than the step between two distinct totals of C.  Prices and bids are 64-bit
//              integers; there is no floating-point price.
//   output     out = (float)((double)total * quantum / p), total the optimal integer cost.  The optimal cost is unique where the
//              optimal assignment is not, so out depends neither on the bidding order nor on the eps schedule nor on the number of
//              workgroups, and md_emd_matrix(x, y)[i][j] == md_emd_matrix(y, x)[j][i] bit for bit.
//
// The auction, in the form that minimises: person k of x values object j of y at w = C[k][j] + price[j].  A round is Jacobi: every
// unassigned person finds its smallest w (ties to the lowest j) and its second smallest, and bids price[j] + (second - smallest) +
// eps for j (p = 1 has no second: price + eps); an object takes its highest bid (ties to the lowest bidder), raises its price to
// it and drops its former owner.  The highest bid is found by ONE kind of atomic, a 64-bit LDS maximum of (bid << 12 | 4095 -
// bidder), which does not depend on the order of the bidders.  A phase ends when nobody is unassigned; the next one starts from eps
// / 4 (EMD_THETA) with everybody unassigned and the prices kept; eps0 = max(1, max C / 2).  Bids stay far below 2^50: a price rises
// by at most max C + eps per bid it receives in a phase.  A bid beyond that ends the pair like the cap on the rounds does.
//
// Launch: ONE workgroup of 512 lanes (8 waves) per pair of clouds, everything in LDS after one load (50 p bytes: 100 KiB at the
// limit p = 2048): x as xyz triples (a bidder reads its own point as a broadcast), y as three planes (the lanes of a wave read
// consecutive objects), prices, bid slots, owner / assignment / bidder list.  A bid is the work of one WAVE: its 64 lanes split
// the objects and recompute every quantised cost from the points -- a p x p cost matrix never exists -- then fold (smallest, its
// index, second smallest) by an xor tree.  The rounds are latency bound (a handful of bidders per round, tests/emd_cases.py), which
// is what a wave per bidder suits.  The round loop is bounded by max_rounds: a pair that reaches it writes NaN and status 1, and
// the rest of the launch carries on.  A triangular launch (x == y) solves the pairs i < j and writes [i][j] and [j][i] (perm[j][i]
// is the inverse permutation, which is `owner`); its diagonal is the exact zero, or NaN with status 3 for a non-finite cloud.  It
// starts nx * nx workgroups, of which those below the diagonal return at once.
// Before it bids, every pair scans all p x p distances once, for eps0 (the largest cost) and for the 2^21 check: 4 M square roots
// at p = 2048, the work of 2048 single-bidder scans against the 130 - 250 k bids such a pair takes -- one or two percent.
#include "md_args.h"

static constexpr int EMD_THREADS = 512;
static constexpr int EMD_WAVES = EMD_THREADS / 64;
static constexpr int EMD_MAX_P = 2048;
static constexpr int EMD_THETA = 4;
static constexpr int EMD_IDX_BITS = 12;                     // bidder index field of a bid slot: p <= 2048 < 4095
static constexpr uint64_t EMD_IDX_MASK = (1ull << EMD_IDX_BITS) - 1;
static constexpr uint64_t EMD_BID_LIMIT = 1ull << 50;
static constexpr float EMD_Q_LIMIT = 2097152.f;             // 2^21
static constexpr int EMD_LDS_PER_POINT = 50;                // 8 price + 8 slot + 12 x + 12 y + 4 bid record + 3 * 2 owner / asg / list

enum { EMD_OK = 0, EMD_CAPPED = 1, EMD_QUANTUM = 2, EMD_NONFINITE = 3 };

__device__ __forceinline__ bool emd_finite(float v) { return fabsf(v) < __builtin_inff(); }      // false for NaN too

__device__ __forceinline__ float emd_scaled_dist(float ax, float ay, float az, float bx, float by, float bz, float inv_quantum) {
#pragma clang fp contract(off)
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrtf(dz * dz + (dy * dy + dx * dx)) * inv_quantum;                // inv_quantum is a power of two: the product is d / quantum
}

struct EmdLds {
  uint64_t* price;
  uint64_t* slot;
  float* a;                                                 // x cloud, xyz triples
  float *bx, *by, *bz;                                      // y cloud, planes
  int32_t* rec;                                             // bidder g of this round: person << 16 | object it bids for
  int16_t *owner, *asg, *list;                              // object -> person, person -> object, unassigned persons by wave slice
};

// unassigned persons of wave `wave`'s slice [wave * slice, ...) -> list[wave * slice ...], their number -> s_cnt[wave]
__device__ __forceinline__ void emd_compact(const EmdLds& L, int p, int slice, int wave, int lane, int* s_cnt) {
  const int lo = wave * slice;
  const int hi = lo + slice < p ? lo + slice : p;
  int cnt = 0;
  for (int base = lo; base < hi; base += 64) {
    const int k = base + lane;
    const bool un = k < hi && L.asg[k] < 0;
    const uint64_t mask = __ballot(un);
    if (un) L.list[lo + cnt + __popcll(mask & ((1ull << lane) - 1))] = (int16_t)k;
    cnt += __popcll(mask);
  }
  if (lane == 0) s_cnt[wave] = cnt;
}

__global__ __launch_bounds__(EMD_THREADS) void md_emd_matrix_kernel(const float* x, const float* y, int ny, int p, float inv_quantum,
                                                                    double quantum, int max_rounds, int triangular,
                                                                    float* __restrict__ out, int32_t* __restrict__ status,
                                                                    int64_t* __restrict__ total, int32_t* __restrict__ rounds,
                                                                    int32_t* __restrict__ perm) {
  extern __shared__ uint64_t emd_lds[];
  __shared__ int s_cnt[EMD_WAVES];
  __shared__ int s_qmax[EMD_WAVES];
  __shared__ uint64_t s_sum[EMD_WAVES];
  __shared__ int s_flag[3];                                 // non-finite coordinate, quantum too small, bid out of range
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t pair = blockIdx.x;
  const int64_t ci = pair / ny, cj = pair % ny;
  const int64_t mirror = cj * ny + ci;                      // triangular: nx == ny
  const float nan = __builtin_nanf("");

  if (triangular) {
    if (ci > cj) return;                                    // written by the workgroup of (cj, ci)
    if (ci == cj) {                                         // a cloud against itself: the exact zero, unless it is not finite
      if (tid == 0) s_flag[0] = 0;
      __syncthreads();
      const float* xi = x + ci * p * 3;
      bool bad = false;
      for (int k = tid; k < 3 * p; k += EMD_THREADS) bad |= !emd_finite(xi[k]);
      if (bad) s_flag[0] = 1;
      __syncthreads();
      const bool nf = s_flag[0] != 0;
      if (tid == 0) {
        out[pair] = nf ? nan : 0.f;
        status[pair] = nf ? EMD_NONFINITE : EMD_OK;
        if (total) total[pair] = nf ? -1 : 0;
        if (rounds) rounds[pair] = 0;
      }
      if (perm)
        for (int k = tid; k < p; k += EMD_THREADS) perm[pair * p + k] = nf ? -1 : k;
      return;
    }
  }

  EmdLds L;
  L.price = emd_lds;
  L.slot = L.price + p;
  L.a = (float*)(L.slot + p);
  L.bx = L.a + 3 * p;
  L.by = L.bx + p;
  L.bz = L.by + p;
  L.rec = (int32_t*)(L.bz + p);
  L.owner = (int16_t*)(L.rec + p);
  L.asg = L.owner + p;
  L.list = L.asg + p;

  // ---- load both clouds once ------------------------------------------------------------------------------------------------
  if (tid < 3) s_flag[tid] = 0;
  __syncthreads();
  {
    const float* xi = x + ci * p * 3;
    const float* yj = y + cj * p * 3;
    bool bad = false;
    for (int k = tid; k < p; k += EMD_THREADS) {
      const float ax = xi[3 * k], ay = xi[3 * k + 1], az = xi[3 * k + 2];
      const float bx = yj[3 * k], by = yj[3 * k + 1], bz = yj[3 * k + 2];
      L.a[3 * k] = ax; L.a[3 * k + 1] = ay; L.a[3 * k + 2] = az;
      L.bx[k] = bx; L.by[k] = by; L.bz[k] = bz;
      L.price[k] = 0;
      L.slot[k] = 0;
      L.owner[k] = -1;
      L.asg[k] = -1;
      bad |= !(emd_finite(ax) && emd_finite(ay) && emd_finite(az) && emd_finite(bx) && emd_finite(by) && emd_finite(bz));
    }
    if (bad) s_flag[0] = 1;
  }
  __syncthreads();

  int st = EMD_OK;
  int n_rounds = 0;
  if (s_flag[0]) {
    st = EMD_NONFINITE;
  } else {
    // ---- the largest quantised cost of the pair, and whether the quantum suits the data ----------------------------------------
    int qmax = 0;
    bool over = false;
    for (int i = wave; i < p; i += EMD_WAVES) {
      const float ax = L.a[3 * i], ay = L.a[3 * i + 1], az = L.a[3 * i + 2];
      for (int j = lane; j < p; j += 64) {
        const float t = emd_scaled_dist(ax, ay, az, L.bx[j], L.by[j], L.bz[j], inv_quantum);
        if (!(t < EMD_Q_LIMIT)) over = true;
        else {
          const int q = (int)rintf(t);
          qmax = q > qmax ? q : qmax;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int other = __shfl_xor(qmax, o, 64);
      qmax = other > qmax ? other : qmax;
    }
    if (lane == 0) s_qmax[wave] = qmax;
    if (over) s_flag[1] = 1;
    __syncthreads();
    if (s_flag[1]) st = EMD_QUANTUM;
    else {
#pragma unroll
      for (int w = 0; w < EMD_WAVES; ++w) qmax = s_qmax[w] > qmax ? s_qmax[w] : qmax;
    }

    if (st == EMD_OK) {
      // ---- the auction --------------------------------------------------------------------------------------------------------
      const uint32_t p1 = (uint32_t)p + 1u;
      const int slice = (p + EMD_WAVES - 1) / EMD_WAVES;
      uint64_t eps = ((uint64_t)qmax * p1) >> 1;
      if (eps < 1) eps = 1;
      bool done = false;
      emd_compact(L, p, slice, wave, lane, s_cnt);
      __syncthreads();
      for (int r = 0; r <= max_rounds; ++r) {
        int nbid = 0;
#pragma unroll
        for (int w = 0; w < EMD_WAVES; ++w) nbid += s_cnt[w];
        if (nbid == 0) {                                    // the phase is over
          if (eps == 1) { done = true; break; }
          eps /= EMD_THETA;
          if (eps < 1) eps = 1;
          for (int k = tid; k < p; k += EMD_THREADS) { L.owner[k] = -1; L.asg[k] = -1; }
          __syncthreads();                                  // which also says that everybody has read s_cnt
          emd_compact(L, p, slice, wave, lane, s_cnt);
          __syncthreads();
          nbid = p;
        }
        if (r == max_rounds) break;                         // the cap: this round is not run
        ++n_rounds;

        // bids: bidder g is the work of wave g % EMD_WAVES
        for (int g = wave; g < nbid; g += EMD_WAVES) {
          int seg = 0, rem = g;
#pragma unroll
          for (int w = 0; w < EMD_WAVES - 1; ++w) {
            const int c = s_cnt[w];
            const bool past = seg == w && rem >= c;
            rem -= past ? c : 0;
            seg += past ? 1 : 0;
          }
          const int i = L.list[seg * slice + rem];
          const float ax = L.a[3 * i], ay = L.a[3 * i + 1], az = L.a[3 * i + 2];
          uint64_t w1 = ~0ull, w2 = ~0ull;
          int j1 = 0x7fffffff;
#pragma unroll 4
          for (int j = lane; j < p; j += 64) {
            const float t = emd_scaled_dist(ax, ay, az, L.bx[j], L.by[j], L.bz[j], inv_quantum);
            const uint64_t w = (uint64_t)(uint32_t)(int)rintf(t) * p1 + L.price[j];
            if (w < w1) { w2 = w1; w1 = w; j1 = j; }        // ascending j: a tie keeps the lower index
            else if (w < w2) w2 = w;
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const uint64_t o1 = __shfl_xor((unsigned long long)w1, o, 64), o2 = __shfl_xor((unsigned long long)w2, o, 64);
            const int oj = __shfl_xor(j1, o, 64);
            if (o1 < w1 || (o1 == w1 && oj < j1)) { w2 = w1 < o2 ? w1 : o2; w1 = o1; j1 = oj; }
            else w2 = w2 < o1 ? w2 : o1;
          }
          if (lane == 0) {
            const uint64_t bid = L.price[j1] + (p > 1 ? w2 - w1 : 0ull) + eps;
            L.rec[g] = (i << 16) | j1;
            if (bid >= EMD_BID_LIMIT) s_flag[2] = 1;
            else
              __hip_atomic_fetch_max(&L.slot[j1], (bid << EMD_IDX_BITS) | (EMD_IDX_MASK - (uint64_t)i), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
        __syncthreads();

        // every object that got a bid goes to its highest bidder: the winner's thread does it
        for (int g = tid; g < nbid; g += EMD_THREADS) {
          const int rec = L.rec[g];
          const int i = rec >> 16, j = rec & 0xffff;
          const uint64_t s = __hip_atomic_load(&L.slot[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          if (s != 0 && (int)(EMD_IDX_MASK - (s & EMD_IDX_MASK)) == i) {
            L.price[j] = s >> EMD_IDX_BITS;
            const int old = L.owner[j];
            if (old >= 0) L.asg[old] = -1;                  // `old` was assigned, so it is nobody's bidder this round
            L.owner[j] = (int16_t)i;
            L.asg[i] = (int16_t)j;
            __hip_atomic_store(&L.slot[j], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
        __syncthreads();
        if (s_flag[2]) break;
        emd_compact(L, p, slice, wave, lane, s_cnt);
        __syncthreads();
      }
      if (!done) st = EMD_CAPPED;
    }
  }

  // ---- results ----------------------------------------------------------------------------------------------------------------
  if (st != EMD_OK) {
    if (tid == 0) {
      out[pair] = nan;
      status[pair] = st;
      if (total) total[pair] = -1;
      if (rounds) rounds[pair] = n_rounds;
      if (triangular) {
        out[mirror] = nan;
        status[mirror] = st;
        if (total) total[mirror] = -1;
        if (rounds) rounds[mirror] = n_rounds;
      }
    }
    if (perm)
      for (int k = tid; k < p; k += EMD_THREADS) {
        perm[pair * p + k] = -1;
        if (triangular) perm[mirror * p + k] = -1;
      }
    return;
  }
  uint64_t sum = 0;
  for (int k = tid; k < p; k += EMD_THREADS) {
    const int j = L.asg[k];
    sum += (uint64_t)(uint32_t)(int)rintf(emd_scaled_dist(L.a[3 * k], L.a[3 * k + 1], L.a[3 * k + 2], L.bx[j], L.by[j], L.bz[j], inv_quantum));
    if (perm) {
      perm[pair * p + k] = j;
      if (triangular) perm[mirror * p + k] = L.owner[k];   // the inverse permutation
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor((unsigned long long)sum, o, 64);
  if (lane == 0) s_sum[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    sum = 0;
#pragma unroll
    for (int w = 0; w < EMD_WAVES; ++w) sum += s_sum[w];
    const float v = (float)((double)sum * quantum / (double)p);
    out[pair] = v;
    status[pair] = EMD_OK;
    if (total) total[pair] = (int64_t)sum;
    if (rounds) rounds[pair] = n_rounds;
    if (triangular) {
      out[mirror] = v;
      status[mirror] = EMD_OK;
      if (total) total[mirror] = (int64_t)sum;
      if (rounds) rounds[mirror] = n_rounds;
    }
  }
}

extern "C" int md_emd_matrix(const float* x, const float* y, int32_t nx, int32_t ny, int32_t p, float quantum, int32_t max_rounds,
                             int32_t triangular, float* out, int32_t* status, int64_t* total, int32_t* rounds, int32_t* perm,
                             void* stream) {
  if (md_any_bad<1>(x, y, out, status) || nx < 1 || ny < 1 || p < 1 || max_rounds < 1) return MD_ERR_BAD_ARG;
  int e = 0;
  if (!(quantum > 0.f) || !(quantum < __builtin_inff()) || frexpf(quantum, &e) != 0.5f) return MD_ERR_BAD_ARG;      // NaN fails the first
  if (triangular && (x != y || nx != ny)) return MD_ERR_BAD_ARG;
  if (p > EMD_MAX_P) return MD_ERR_UNSUPPORTED;
  if (e - 1 < -126 || e - 1 > 126) return MD_ERR_UNSUPPORTED;              // 1 / quantum must be a normal fp32 number
  if (!md_fits_i32((int64_t)nx * ny)) return MD_ERR_UNSUPPORTED;           // one workgroup per pair along gridDim.x
  if (max_rounds > (1 << 30)) max_rounds = 1 << 30;                         // the round counter is an int that runs to max_rounds
  const size_t lds = ((size_t)EMD_LDS_PER_POINT * p + 15) & ~(size_t)15;
  MD_HIP_CLEAR_ERROR();
  if (lds > 48 * 1024) {                                                    // above the default limit of dynamic LDS
    hipError_t err = hipFuncSetAttribute((const void*)md_emd_matrix_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (err != hipSuccess) return (int)err;
  }
  hipLaunchKernelGGL(md_emd_matrix_kernel, dim3((unsigned)((int64_t)nx * ny)), dim3(EMD_THREADS), lds, (hipStream_t)stream, x, y,
                     (int)ny, (int)p, 1.0f / quantum, (double)quantum, (int)max_rounds, (int)triangular, out, status, total, rounds,
                     perm);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
