// Generation metrics under a light-field distance in the manner of Chen, Tian, Shen and Ouhyoung 2003: a model is L light fields
// of 10 silhouettes (one per antipodal vertex pair of a regular dodecahedron), a silhouette is 48 bytes (35 Zernike magnitudes,
// 10 Fourier magnitudes of its angular signature, 3 zero bytes), and the distance of two models is the smallest sum of the ten
// image distances over the pairs of light fields and the 60 rotations of the dodecahedron.  The original executable traces
// contours and has its own scalings: values are not comparable with its numbers.  No implementation was consulted; THE LFD
// CONTRACT below is the definition, and tests/lfd_cases.py restates it in float64.
//
// ---- md_lfd_describe ----------------------------------------------------------------------------------------------------------
// mask uint8 [n][R][R]; a pixel is set where its byte is non-zero, pixel (row y, column x) sits at (x, y).  `count` set pixels,
// centroid c = (sum x / count, sum y / count), rmax = max(0.5, max_p |p - c|); per set pixel rho = |p - c| / rmax and theta =
// atan2(dy, dx).
//   Zernike   n = 1..10, m = n mod 2, .., n in steps of 2 (35 values in that order):
//             z_nm = |sum_p R_nm(rho) e^{-i m theta}| / count,
//             R_nm(rho) = sum_{s=0}^{(n-m)/2} (-1)^s (n-s)! / (s! ((n+m)/2-s)! ((n-m)/2-s)!) rho^(n-2s)
//   Signature 64 bins, b = floor(64 theta / 2 pi + 0.5) mod 64 (axes and diagonals are bin centres); sig[b] = max rho of the bin, 0
//             when it is empty
//   Fourier   f_k = |sum_b sig[b] e^{-2 pi i k b / 64}| / sum_b sig[b], k = 1..10; 0 when the sum is 0 (a single pixel)
//   Output    coef[45] = fp32(512 z), fp32(512 f); desc = min(255, rint(coef)) as bytes, then three zero bytes.  Empty mask: all
//             zero, status 1; otherwise status 0.
//
// Evaluation scheme (the error bar DESC_BAR of tests/lfd_cases.py follows from it).  Everything that can be an integer is one:
//   Nx = x count - sum x,  Ny = y count - sum y  (|.| < 2^27 at R = 512),  q = Nx^2 + Ny^2 < 2^55,  Q = max q,
// so that (dx, dy) = (Nx, Ny) / count and rho^2 = q / Qe with Qe = max(Q, count^2 / 4) -- no rounded centroid enters.  Once per
// mask, in float64: inv = fp32(1 / sqrt(Qe)), inv2 = fp32(1 / Qe).  Per set pixel, in fp32 WITHOUT contraction:
//   w = (fp32(Nx) * inv, -(fp32(Ny) * inv))                       = rho e^{-i theta}
//   t = fp32(q) * inv2                                            = rho^2
//   W_0 = 1, W_m = W_{m-1} * w  (re = ar br - ai bi, im = ar bi + ai br)          = rho^m e^{-i m theta}
//   P_nm(t) by Horner from the highest power, p = p * t + c, the coefficients being the integers of R_nm (all below 2^24)
//   term = (P * W_m.re, P * W_m.im), each times 2^32 and rounded to an integer (round to nearest even).
// The integers are summed as int64 (|term| < 1.01 and count <= 2^18: below 2^51), so the sum is exact whatever its order: the
// result does not depend on the launch and two runs agree bit for bit.  z = sqrt(re^2 + im^2) / 2^32 / count in float64.
// The bin is the one place where fp32 decides something discrete: b = (int)floorf(atan2f(fp32(Ny), fp32(Nx)) * fp32(64 / 2 pi) +
// 0.5f) & 63; a pixel within about 1e-5 bins of a boundary may fall on either side (the test cases keep 2^-16 clear).  The
// maximum of a bin is the exact integer max q; sig[b] = sqrt(max q / Qe), the 64-point transform (twiddles cospi / sinpi of the
// exact argument (k b mod 64) / 32) and the normalisation are float64, rounded once.
//
// Launch: one workgroup of 256 lanes per mask, three sweeps over it (sums; Q and the bins; the moments): the second needs the
// sums and the third needs Q.  A mask of 256^2 is 64 KiB, so sweeps two and three come from L2.  Lane l takes the pixels l, l +
// 256, ...: a wave reads 64 consecutive bytes.  35 complex accumulators (the m = 0 ones are real: 65 int64) live in registers and
// are folded into LDS with 64-bit integer atomics at the end (exact, so their order does not matter); 1.7 KiB of LDS.
//
// ---- md_lfd_matrix ------------------------------------------------------------------------------------------------------------
// x uint8 [nx][L][10][48], y uint8 [ny][L][10][48], perm uint8 [G][10] on the HOST (checked there, passed by value):
//   out[i][j] = min over la, lb < L and g < G of sum_{v<10} SAD48(x[i][la][v], y[j][lb][perm[g][v]]).
// Integers throughout (one image pair <= 48 * 255 fits 16 bits, a sum <= 122400): exact, independent of the launch.  triangular
// (x == y): the pairs i < j only, written to both halves, and a zero diagonal.
//
// Launch: a workgroup of 256 lanes owns ONE x model and a run of MD_LFD_RUN consecutive y models; both models lie in LDS as dwords
// (L * 480 bytes each).  The L^2 pairs of light fields are dealt to the four waves in turn.  For its pair a wave first builds the
// 10 x 10 table of image distances -- lane e (and e + 64 below 100) reads the two 48-byte images as three 16-byte LDS reads each
// and folds them with 12 v_sad_u8 (__builtin_amdgcn_sad_u8: four bytes per instruction, accumulating) -- into its own 400 bytes
// of LDS; then lane g < G adds the ten entries [v][perm[g][v]] (offsets kept in registers) and keeps a running minimum.  After
// the last pair the minimum goes through an xor tree of the wave and the four waves meet in LDS.  No atomics.  ~17 KiB of LDS.
#include "md_args.h"

static constexpr int LFD_THREADS = 256;
static constexpr int LFD_NZ = 35;                           // Zernike values
static constexpr int LFD_NF = 10;                           // Fourier values
static constexpr int LFD_BINS = 64;
static constexpr int LFD_MAX_N = 10;
static constexpr int LFD_NACC = 2 * LFD_NZ;                 // (re, im) per value; the im of an m = 0 value stays 0
static_assert(LFD_NZ + LFD_NF == MD_LFD_COEFS && MD_LFD_COEFS + 3 == MD_LFD_DESC_BYTES, "descriptor layout");

// the coefficient of rho^(n - 2s) in R_nm: an integer below 2^24, exact in fp32
constexpr double lfd_fact(int k) {
  double r = 1.0;
  for (int i = 2; i <= k; ++i) r *= i;
  return r;
}
template <int N, int M, int S> struct LfdCoef {
  static constexpr float v =
      (float)(((S & 1) ? -1.0 : 1.0) * lfd_fact(N - S) / (lfd_fact(S) * lfd_fact((N + M) / 2 - S) * lfd_fact((N - M) / 2 - S)));
};
// position of (n, m) in the order n = 1..10, m = n mod 2, .., n
constexpr int lfd_index(int n, int m) {
  int idx = 0;
  for (int a = 1; a < n; ++a) idx += a / 2 + 1;
  return idx + (m - (n & 1)) / 2;
}
static_assert(lfd_index(1, 1) == 0 && lfd_index(2, 0) == 1 && lfd_index(10, 10) == LFD_NZ - 1, "order of the Zernike values");

// Horner steps S.. of P_nm in t
template <int N, int M, int S> __device__ __forceinline__ float lfd_horner(float P, float t) {
#pragma clang fp contract(off)
  if constexpr (S > (N - M) / 2) return P;
  else return lfd_horner<N, M, S + 1>(P * t + LfdCoef<N, M, S>::v, t);
}
// the terms of (N, M) and of every value after it, added to acc as integers
template <int N, int M> __device__ __forceinline__ void lfd_terms(const float (&Wr)[LFD_MAX_N + 1], const float (&Wi)[LFD_MAX_N + 1], float t,
                                                                  long long (&acc)[LFD_NACC]) {
#pragma clang fp contract(off)
  if constexpr (N <= LFD_MAX_N) {
    constexpr int idx = lfd_index(N, M);
    const float P = lfd_horner<N, M, 1>(LfdCoef<N, M, 0>::v, t);
    acc[2 * idx] += __float2ll_rn((P * Wr[M]) * 4294967296.f);
    if constexpr (M > 0) acc[2 * idx + 1] += __float2ll_rn((P * Wi[M]) * 4294967296.f);
    if constexpr (M + 2 <= N) lfd_terms<N, M + 2>(Wr, Wi, t, acc);
    else lfd_terms<N + 1, (N + 1) & 1>(Wr, Wi, t, acc);
  }
}

__device__ __forceinline__ void lfd_pixel(int p, int R, int& x, int& y) {
  y = (int)((unsigned)p / (unsigned)R);
  x = p - y * R;
}

__global__ __launch_bounds__(LFD_THREADS) void md_lfd_describe_kernel(const uint8_t* __restrict__ mask, int R, uint8_t* __restrict__ desc,
                                                                      float* __restrict__ coef, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_sum[3];                   // count, sum x, sum y
  __shared__ unsigned long long s_q[LFD_BINS + 1];          // max q per bin; [64] = Q
  __shared__ unsigned long long s_acc[LFD_NACC];            // two's complement sums of the terms
  __shared__ double s_sig[LFD_BINS];
  const int tid = threadIdx.x;
  const int npix = R * R;
  const uint8_t* m = mask + (int64_t)blockIdx.x * npix;
  uint8_t* d = desc + (int64_t)blockIdx.x * MD_LFD_DESC_BYTES;
  float* cf = coef ? coef + (int64_t)blockIdx.x * MD_LFD_COEFS : nullptr;

  if (tid < 3) s_sum[tid] = 0;
  if (tid <= LFD_BINS) s_q[tid] = 0;
  if (tid < LFD_NACC) s_acc[tid] = 0;
  __syncthreads();

  // sweep 1: count and the coordinate sums (a lane sees at most 1024 pixels: 1024 * 511 fits 32 bits)
  {
    unsigned cnt = 0, sx = 0, sy = 0;
    for (int p = tid; p < npix; p += LFD_THREADS)
      if (m[p]) {
        int x, y;
        lfd_pixel(p, R, x, y);
        ++cnt; sx += (unsigned)x; sy += (unsigned)y;
      }
    if (cnt) {
      atomicAdd(&s_sum[0], (unsigned long long)cnt);
      atomicAdd(&s_sum[1], (unsigned long long)sx);
      atomicAdd(&s_sum[2], (unsigned long long)sy);
    }
  }
  __syncthreads();
  const int count = (int)s_sum[0];
  if (count == 0) {                                         // workgroup-uniform
    if (tid < MD_LFD_DESC_BYTES) d[tid] = 0;
    if (cf && tid < MD_LFD_COEFS) cf[tid] = 0.f;
    if (tid == 0) status[blockIdx.x] = 1;
    return;
  }
  const int sumx = (int)s_sum[1], sumy = (int)s_sum[2];     // <= 2^18 * 511 < 2^27

  // sweep 2: Q and the largest q of every angular bin
  {
    unsigned long long qmax = 0;
    for (int p = tid; p < npix; p += LFD_THREADS)
      if (m[p]) {
        int x, y;
        lfd_pixel(p, R, x, y);
        const long long nx = (long long)(x * count - sumx), ny = (long long)(y * count - sumy);
        const unsigned long long q = (unsigned long long)(nx * nx + ny * ny);
        if (q) {                                            // q == 0: the centroid itself, rho = 0 in whatever bin
          const float a = atan2f((float)ny, (float)nx);
          const int b = (int)floorf(a * 10.18591636f + 0.5f) & (LFD_BINS - 1);      // 64 / (2 pi)
          atomicMax(&s_q[b], q);
          qmax = q > qmax ? q : qmax;
        }
      }
    if (qmax) atomicMax(&s_q[LFD_BINS], qmax);
  }
  __syncthreads();
  const double qfloor = 0.25 * (double)count * (double)count;
  const double Q = (double)s_q[LFD_BINS];
  const double Qe = Q > qfloor ? Q : qfloor;
  const float inv = (float)(1.0 / sqrt(Qe)), inv2 = (float)(1.0 / Qe);

  // sweep 3: the 35 complex moments as exact integer sums
  long long acc[LFD_NACC];
#pragma unroll
  for (int k = 0; k < LFD_NACC; ++k) acc[k] = 0;
  for (int p = tid; p < npix; p += LFD_THREADS)
    if (m[p]) {
      int x, y;
      lfd_pixel(p, R, x, y);
      const long long nx = (long long)(x * count - sumx), ny = (long long)(y * count - sumy);
      const unsigned long long q = (unsigned long long)(nx * nx + ny * ny);
      const float wr = (float)nx * inv, wi = -((float)ny * inv);
      const float t = (float)q * inv2;
      float Wr[LFD_MAX_N + 1], Wi[LFD_MAX_N + 1];
      Wr[0] = 1.f; Wi[0] = 0.f;
      Wr[1] = wr; Wi[1] = wi;
#pragma unroll
      for (int k = 2; k <= LFD_MAX_N; ++k) {
        Wr[k] = Wr[k - 1] * wr - Wi[k - 1] * wi;
        Wi[k] = Wr[k - 1] * wi + Wi[k - 1] * wr;
      }
      lfd_terms<1, 1>(Wr, Wi, t, acc);
    }
#pragma unroll
  for (int k = 0; k < LFD_NACC; ++k)
    if (acc[k]) atomicAdd(&s_acc[k], (unsigned long long)acc[k]);
  if (tid < LFD_BINS) s_sig[tid] = sqrt((double)s_q[tid] / Qe);
  __syncthreads();

  float c = 0.f;
  if (tid < LFD_NZ) {
    const double re = (double)(long long)s_acc[2 * tid], im = (double)(long long)s_acc[2 * tid + 1];
    c = (float)(512.0 * (sqrt(re * re + im * im) * (1.0 / 4294967296.0) / (double)count));
  } else if (tid < MD_LFD_COEFS) {
    const int k = tid - LFD_NZ + 1;
    double re = 0.0, im = 0.0, tot = 0.0;
    for (int b = 0; b < LFD_BINS; ++b) {
      const double a = (double)((k * b) & (LFD_BINS - 1)) * (1.0 / 32.0);
      re += s_sig[b] * cospi(a);
      im -= s_sig[b] * sinpi(a);
      tot += s_sig[b];
    }
    c = tot > 0.0 ? (float)(512.0 * (sqrt(re * re + im * im) / tot)) : 0.f;
  }
  if (tid < MD_LFD_DESC_BYTES) d[tid] = tid < MD_LFD_COEFS ? (uint8_t)fminf(255.f, rintf(c)) : (uint8_t)0;
  if (cf && tid < MD_LFD_COEFS) cf[tid] = c;
  if (tid == 0) status[blockIdx.x] = 0;
}

extern "C" int md_lfd_describe(const uint8_t* mask, int32_t n, int32_t R, uint8_t* desc, float* coef, int32_t* status, void* stream) {
  if (md_any_bad<1>(mask, desc) || md_any_bad<4>(status) || md_any_misaligned<4>(coef) || n < 1 || R < 1) return MD_ERR_BAD_ARG;
  if (R > MD_LFD_MAX_RES || (int64_t)n * LFD_THREADS > 0x7fffffffLL) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_lfd_describe_kernel, dim3((unsigned)n), dim3(LFD_THREADS), 0, (hipStream_t)stream, mask, (int)R, desc, coef,
                     status);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}

// ---- the matrix ------------------------------------------------------------------------------------------------------------------
static constexpr int LFD_V = MD_LFD_VIEWS;
static constexpr int LFD_IMG_DW = MD_LFD_DESC_BYTES / 4;                 // 12 dwords per image
static constexpr int LFD_FIELD_DW = LFD_V * LFD_IMG_DW;                  // 120 dwords per light field
static constexpr int LFD_MODEL_DW = MD_LFD_MAX_FIELDS * LFD_FIELD_DW;    // 1920 dwords = 7680 bytes
static constexpr int LFD_TABLE = LFD_V * LFD_V;
static constexpr int LFD_WAVES = LFD_THREADS / 64;

struct LfdPerm {
  uint8_t p[MD_LFD_MAX_ROTATIONS][LFD_V];
};

__global__ __launch_bounds__(LFD_THREADS) void md_lfd_matrix_kernel(const uint32_t* __restrict__ x, const uint32_t* __restrict__ y,
                                                                    const LfdPerm perm, int ny, int L, int G, int triangular,
                                                                    int32_t* __restrict__ out) {
  __shared__ uint4 s_x[LFD_MODEL_DW / 4];
  __shared__ uint4 s_y[LFD_MODEL_DW / 4];
  __shared__ int s_tab[LFD_WAVES][LFD_TABLE];
  __shared__ int s_min[LFD_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x;
  const int j_begin = blockIdx.y * MD_LFD_RUN;
  const int j_end = j_begin + MD_LFD_RUN < ny ? j_begin + MD_LFD_RUN : ny;
  const int model_dw = L * LFD_FIELD_DW;
  if (triangular && j_end <= i) return;                     // workgroup-uniform: neither the diagonal nor a pair i < j in this run

  int off[LFD_V];                                            // lane g: the table entries [v][perm[g][v]]
  {
    const int g = lane < G ? lane : 0;
#pragma unroll
    for (int v = 0; v < LFD_V; ++v) off[v] = v * LFD_V + perm.p[g][v];
  }
  for (int k = tid; k < model_dw; k += LFD_THREADS) ((uint32_t*)s_x)[k] = x[(int64_t)i * model_dw + k];

  const int pairs = L * L;
  for (int j = j_begin; j < j_end; ++j) {
    if (triangular && j <= i) {                             // workgroup-uniform
      if (j == i && tid == 0) out[(int64_t)i * ny + i] = 0;
      continue;
    }
    __syncthreads();                                        // the previous y model has been read to the end
    for (int k = tid; k < model_dw; k += LFD_THREADS) ((uint32_t*)s_y)[k] = y[(int64_t)j * model_dw + k];
    __syncthreads();
    int best = 0x7fffffff;
    for (int p0 = 0; p0 < pairs; p0 += LFD_WAVES) {
      const int pi = p0 + wave;
      const bool active = pi < pairs;                       // wave-uniform
      if (active) {
        const int la = pi / L, lb = pi - la * L;
        for (int e = lane; e < LFD_TABLE; e += 64) {
          const int v = e / LFD_V, u = e - v * LFD_V;
          const uint4* a = s_x + (la * LFD_V + v) * (LFD_IMG_DW / 4);
          const uint4* b = s_y + (lb * LFD_V + u) * (LFD_IMG_DW / 4);
          unsigned s = 0;
#pragma unroll
          for (int k = 0; k < LFD_IMG_DW / 4; ++k) {
            const uint4 p = a[k], r = b[k];
            s = __builtin_amdgcn_sad_u8(p.x, r.x, s);
            s = __builtin_amdgcn_sad_u8(p.y, r.y, s);
            s = __builtin_amdgcn_sad_u8(p.z, r.z, s);
            s = __builtin_amdgcn_sad_u8(p.w, r.w, s);
          }
          s_tab[wave][e] = (int)s;
        }
      }
      __syncthreads();                                      // the tables are written
      if (active && lane < G) {
        int s = 0;
#pragma unroll
        for (int v = 0; v < LFD_V; ++v) s += s_tab[wave][off[v]];
        best = s < best ? s : best;
      }
      __syncthreads();                                      // and read, before the next pair overwrites them
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int other = __shfl_xor(best, o, 64);
      best = other < best ? other : best;
    }
    if (lane == 0) s_min[wave] = best;
    __syncthreads();
    if (tid == 0) {
      int r = s_min[0];
#pragma unroll
      for (int w = 1; w < LFD_WAVES; ++w) r = s_min[w] < r ? s_min[w] : r;
      out[(int64_t)i * ny + j] = r;
      if (triangular) out[(int64_t)j * ny + i] = r;
    }
  }
}

extern "C" int md_lfd_matrix(const uint8_t* x, const uint8_t* y, const uint8_t* perm, int32_t nx, int32_t ny, int32_t L, int32_t G,
                             int32_t triangular, int32_t* out, void* stream) {
  if (md_any_bad<4>(x, y, out) || md_any_bad<1>(perm) || nx < 1 || ny < 1 || L < 1 || G < 1) return MD_ERR_BAD_ARG;
  if (L > MD_LFD_MAX_FIELDS || G > MD_LFD_MAX_ROTATIONS) return MD_ERR_UNSUPPORTED;
  LfdPerm table = {};
  for (int g = 0; g < G; ++g)
    for (int v = 0; v < LFD_V; ++v) {
      if (perm[g * LFD_V + v] >= LFD_V) return MD_ERR_BAD_ARG;
      table.p[g][v] = perm[g * LFD_V + v];
    }
  if (triangular && (x != y || nx != ny)) return MD_ERR_BAD_ARG;
  // gridDim.x = nx (a launch's threads along x stay below 2^32), gridDim.y = the runs of y models
  const int64_t runs = ((int64_t)ny + MD_LFD_RUN - 1) / MD_LFD_RUN;
  if ((int64_t)nx * LFD_THREADS > 0xffffffffLL || runs > 65535) return MD_ERR_UNSUPPORTED;
  MD_HIP_CLEAR_ERROR();
  hipLaunchKernelGGL(md_lfd_matrix_kernel, dim3((unsigned)nx, (unsigned)runs), dim3(LFD_THREADS), 0, (hipStream_t)stream,
                     (const uint32_t*)x, (const uint32_t*)y, table, (int)ny, (int)L, (int)G, (int)(triangular != 0), out);
  MD_HIP_CHECK_LAUNCH();
  return MD_OK;
}
