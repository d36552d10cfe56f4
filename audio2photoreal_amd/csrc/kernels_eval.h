// Motion evaluation in fp64 (audio2photoreal_amd/evaluate.py): the moments behind the static / kinematic Frechet distances and
// the diversity metrics of the reference's utils/eval.py, a cyclic Jacobi eigensolver for the matrix square root, a small fp64
// GEMM, and the pair distances of the diversity draw.  Inputs are [S, C, T] channels-first motion batches (fp32 as the samplers
// return them, or fp64 as the un-normalised results.npy holds them); every sum is fp64, in a fixed order, with no floating-point
// atomics: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define EVAL_NSPLIT 16          // frame ranges of the covariance partials, merged in ascending order
#define EVAL_XV_BLOCKS 256      // fixed grid of the cross-repetition variance (its partials are merged in block order)
#define EVAL_EIG_THREADS 1024
#define EVAL_EIG_LDS_MAX 128    // n <= 128: the padded matrix lives in LDS (128 x 128 fp64 = 128 KiB of 160)
#define EVAL_EIG_MAX_SWEEPS 40  // Jacobi converges quadratically: hitting this is reported as an error, never returned as a result
#define EVAL_EIG_TOL 1e-15      // stop when ||offdiag(A)||_F <= EVAL_EIG_TOL * ||A||_F

__device__ __forceinline__ bool eval_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// Sum of a and b over a 256-thread block in a fixed tree order; every thread gets the totals.
__device__ __forceinline__ void eval_block_sum2(double& a, double& b, double* red) {
  const int tid = threadIdx.x;
  red[tid] = a;
  red[256 + tid] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      red[256 + tid] += red[256 + tid + s];
    }
    __syncthreads();
  }
  a = red[0];
  b = red[256];
  __syncthreads();
}

// Wave64 butterfly sum: the same order on every run (lane 0's value is the one used).
__device__ __forceinline__ double eval_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Grid C, 256 threads: per channel c, over the S sequences in order, the row sum, the sum of the in-sequence deltas
// x[t+1] - x[t] (never across sequences) and the row's centred M2 (second pass over the row).  mu[c] = sum / (S T),
// mu_v[c] = delta sum / (S (T - 1)), varsum[c] = sum_s M2_s / T (numpy's var along T, ddof 0, summed over s).
template <typename T>
__global__ __launch_bounds__(256) void eval_channel_kernel(const T* __restrict__ x, int S, int C, int Tn, double* mu, double* mu_v,
                                                           double* varsum, int* nonfinite) {
  __shared__ double red[512];
  const int c = blockIdx.x, tid = threadIdx.x;
  double csum = 0.0, cdsum = 0.0, cvar = 0.0;
  bool bad = false;
  for (int s = 0; s < S; ++s) {
    const T* row = x + ((int64_t)s * C + c) * Tn;
    double a = 0.0, d = 0.0;
    for (int t = tid; t < Tn; t += 256) {
      const double v = (double)row[t];
      bad |= !eval_finite(v);
      a += v;
      if (t + 1 < Tn) d += (double)row[t + 1] - v;
    }
    eval_block_sum2(a, d, red);
    const double mean = a / Tn;
    double m2 = 0.0, z = 0.0;
    for (int t = tid; t < Tn; t += 256) {
      const double dv = (double)row[t] - mean;
      m2 = fma(dv, dv, m2);
    }
    eval_block_sum2(m2, z, red);
    csum += a;
    cdsum += d;
    cvar += m2 / Tn;
  }
  if (tid == 0) {
    mu[c] = csum / ((double)S * Tn);
    mu_v[c] = cdsum / ((double)S * (Tn - 1));
    varsum[c] = cvar;
  }
  if (bad) atomicOr(nonfinite, 1);
}

// Grid EVAL_XV_BLOCKS, 256 threads: for every element e of one repetition (per = B C T elements), the variance over the reps
// repetitions x[r * per + e] (two passes, ddof 0), summed per block into part[blockIdx.x].
template <typename T>
__global__ __launch_bounds__(256) void eval_crossvar_kernel(const T* __restrict__ x, int reps, int64_t per, double* part) {
  __shared__ double red[512];
  double acc = 0.0, z = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (int64_t)256 * EVAL_XV_BLOCKS) {
    double m = 0.0;
    for (int r = 0; r < reps; ++r) m += (double)x[r * per + e];
    m /= reps;
    double v = 0.0;
    for (int r = 0; r < reps; ++r) {
      const double dv = (double)x[r * per + e] - m;
      v = fma(dv, dv, v);
    }
    acc += v / reps;
  }
  eval_block_sum2(acc, z, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// One block of 256: sums[0] = sum_c varsum[c], sums[1] = sum of the n_part cross-variance partials (0 when n_part is 0).
__global__ __launch_bounds__(256) void eval_sums_kernel(const double* varsum, int C, const double* part, int n_part, double* sums) {
  __shared__ double red[512];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < C; i += 256) a += varsum[i];
  for (int i = threadIdx.x; i < n_part; i += 256) b += part[i];
  eval_block_sum2(a, b, red);
  if (threadIdx.x == 0) {
    sums[0] = a;
    sums[1] = b;
  }
}

// Grid (ceil(C / 32), ceil(C / 32), EVAL_NSPLIT), 256 threads: the centred cross products of a 32 x 32 tile of channels over
// the z-th of EVAL_NSPLIT equal ranges of the N frames (VEL: of the N = S (T - 1) in-sequence deltas).  Frame n is (s = n / Tf,
// t = n % Tf), read straight from the channels-first layout.  part[(z C + i) C + j].  Tile (I, J) and tile (J, I) multiply the
// same values in the same order, so the covariance comes out exactly symmetric.
template <typename T, bool VEL>
__global__ __launch_bounds__(256) void eval_cov_kernel(const T* __restrict__ x, int S, int C, int Tn, const double* __restrict__ mu,
                                                       double* part) {
  __shared__ double xi[32][33], xj[32][33];  // [frame][channel]
  const int tid = threadIdx.x, z = blockIdx.z;
  const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
  const int ty = tid >> 4, tx = tid & 15;
  const int Tf = VEL ? Tn - 1 : Tn;
  const int64_t N = (int64_t)S * Tf;
  const int64_t n0 = N * z / EVAL_NSPLIT, n1 = N * (z + 1) / EVAL_NSPLIT;
  double acc00 = 0.0, acc01 = 0.0, acc10 = 0.0, acc11 = 0.0;
  for (int64_t nb = n0; nb < n1; nb += 32) {
    for (int k = tid; k < 1024; k += 256) {
      const int f = k & 31, cl = k >> 5;
      const int64_t n = nb + f;
      double vi = 0.0, vj = 0.0;
      if (n < n1) {
        const int64_t s = n / Tf, t = n % Tf;
        const int64_t base = s * C * (int64_t)Tn + t;
        const int ci = i0 + cl, cj = j0 + cl;
        if (ci < C) {
          const T* p = x + base + (int64_t)ci * Tn;
          vi = (VEL ? (double)p[1] - (double)p[0] : (double)p[0]) - mu[ci];
        }
        if (cj < C) {
          const T* p = x + base + (int64_t)cj * Tn;
          vj = (VEL ? (double)p[1] - (double)p[0] : (double)p[0]) - mu[cj];
        }
      }
      xi[f][cl] = vi;
      xj[f][cl] = vj;
    }
    __syncthreads();
#pragma unroll 8
    for (int f = 0; f < 32; ++f) {
      const double a0 = xi[f][ty], a1 = xi[f][ty + 16], b0 = xj[f][tx], b1 = xj[f][tx + 16];
      acc00 = fma(a0, b0, acc00);
      acc01 = fma(a0, b1, acc01);
      acc10 = fma(a1, b0, acc10);
      acc11 = fma(a1, b1, acc11);
    }
    __syncthreads();
  }
  double* o = part + (int64_t)z * C * C;
  const int ia = i0 + ty, ib = i0 + ty + 16, ja = j0 + tx, jb = j0 + tx + 16;
  if (ia < C && ja < C) o[(int64_t)ia * C + ja] = acc00;
  if (ia < C && jb < C) o[(int64_t)ia * C + jb] = acc01;
  if (ib < C && ja < C) o[(int64_t)ib * C + ja] = acc10;
  if (ib < C && jb < C) o[(int64_t)ib * C + jb] = acc11;
}

// cov[e] = (sum over z in ascending order of part[z][e]) / (N - 1), as np.cov normalises (N = 1 gives 0 / 0 = nan like numpy).
__global__ void eval_cov_finish_kernel(const double* part, int64_t CC, int64_t N, double* cov) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= CC) return;
  double a = 0.0;
  for (int z = 0; z < EVAL_NSPLIT; ++z) a += part[z * CC + e];
  cov[e] = a / (double)(N - 1);
}

// 256 threads, one wave per pair: out[w] = || frame idx1[w] - frame idx2[w] ||_2 in fp64, frame f = (s = f / T, t = f % T) read
// from the channels-first layout (the rows of the reference's transpose(0, 1, 3, 2).reshape(-1, C)).  An index outside
// [0, S T) writes nan and sets bit 1 of the flag; a non-finite element sets bit 0.
template <typename T>
__global__ __launch_bounds__(256) void eval_pair_dist_kernel(const T* __restrict__ x, int S, int C, int Tn, const int64_t* idx1,
                                                             const int64_t* idx2, int64_t times, double* out, int* nonfinite) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= times) return;
  const int64_t N = (int64_t)S * Tn, f1 = idx1[w], f2 = idx2[w];
  if (f1 < 0 || f1 >= N || f2 < 0 || f2 >= N) {
    if (lane == 0) {
      out[w] = __builtin_nan("");
      atomicOr(nonfinite, 2);
    }
    return;
  }
  const T* a = x + (f1 / Tn) * C * (int64_t)Tn + f1 % Tn;
  const T* b = x + (f2 / Tn) * C * (int64_t)Tn + f2 % Tn;
  double acc = 0.0;
  bool bad = false;
  for (int c = lane; c < C; c += 64) {
    const double va = (double)a[(int64_t)c * Tn], vb = (double)b[(int64_t)c * Tn];
    bad |= !(eval_finite(va) && eval_finite(vb));
    const double d = va - vb;
    acc = fma(d, d, acc);
  }
  acc = eval_wave_sum(acc);
  if (lane == 0) out[w] = sqrt(acc);
  if (bad) atomicOr(nonfinite, 1);
}

// Grid (ceil(n / 16), ceil(n / 16)), 256 threads: C[i][j] = sum_k A(i, k) d[k] B(k, j) over ascending k, with A(i, k) =
// a[i * a_rs + k * a_cs] and B(k, j) = b[k * b_rs + j * b_cs] (strides express transposes), d NULL = identity.  n <= 256.
__global__ __launch_bounds__(256) void eval_gemm_kernel(int n, const double* a, int64_t a_rs, int64_t a_cs, const double* d,
                                                        const double* b, int64_t b_rs, int64_t b_cs, double* c) {
  __shared__ double as[16][17], bs[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i = blockIdx.y * 16 + ty, j = blockIdx.x * 16 + tx;
  double acc = 0.0;
  for (int k0 = 0; k0 < n; k0 += 16) {
    const int ka = k0 + tx, kb = k0 + ty;
    double av = 0.0, bv = 0.0;
    if (i < n && ka < n) av = a[i * a_rs + ka * a_cs] * (d ? d[ka] : 1.0);
    if (kb < n && j < n) bv = b[kb * b_rs + j * b_cs];
    as[ty][tx] = av;
    bs[ty][tx] = bv;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) acc = fma(as[ty][k], bs[k][tx], acc);
    __syncthreads();
  }
  if (i < n && j < n) c[(int64_t)i * n + j] = acc;
}

// Sum of v over the 1024-thread block, fixed order (wave butterflies, then the 16 wave totals in order); every thread gets it.
__device__ __forceinline__ double eval_eig_block_sum(double v, double* red16) {
  v = eval_wave_sum(v);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red16[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int k = 0; k < EVAL_EIG_THREADS / 64; ++k) t += red16[k];
  return t;
}

// Cyclic Jacobi eigensolver for a symmetric n x n fp64 matrix (n <= 256), one workgroup of 1024 threads.
// The input is symmetrised on load (0.5 (a_ij + a_ji): exact for a symmetric input) and padded to even m = n + (n & 1) with a
// zero row and column.  A sweep is m - 1 rounds of the round-robin (circle) tournament: every round pairs all m indices into
// m / 2 disjoint pairs (p, q), computes one symmetric Schur rotation per pair (Golub & Van Loan 8.4.2) from a_pp, a_qq, a_pq,
// and applies all of them at once: A <- J^T A J as independent 2 x 2 blocks (pair a rows x pair b columns, a <= b, mirrored),
// so every element is read and written by one thread; the diagonal block takes the exact a_pp - t a_pq, a_qq + t a_pq, 0.
// An a_pq below 1e-16 sqrt(|a_pp a_qq|) is set to zero without a rotation (the relative-accuracy rule of Demmel & Veselic):
// without it, clusters of equal eigenvalues keep trading rounding-level 45-degree rotations and need 2-3x the sweeps.
// Q <- Q J when eigenvectors are asked for.  Before every sweep, off = ||offdiag(A)||_F is compared with tol ||A||_F.
//
// Where the matrix lives: IN_LDS (m <= 128): in dynamic LDS (m^2 fp64 <= 128 KiB of the CU's 160).  For 128 < n <= 256 the
// padded matrix is 512 KiB, more than LDS holds; it cannot sit in registers either, because the 2 x 2 blocks a thread owns
// change with the pairing every round (the data would have to cross LDS anyway).  So it lives in a global workspace `gA`
// that stays resident in the XCD's 4 MiB L2: each round touches every element once (read + write), and the barrier of the
// one workgroup orders those accesses (all waves of a workgroup share the CU's L1).  Q is always in global memory ([n][n]).
//
// info[0] = sweeps done, info[1] = status (0 converged, 1 sweep cap hit, 2 non-finite input); off_out[0] = final off.
template <bool IN_LDS>
__global__ __launch_bounds__(EVAL_EIG_THREADS) void eval_jacobi_kernel(const double* __restrict__ a_in, int n, double* w, double* q,
                                                                      double* gA, int* info, double* off_out, int max_sweeps,
                                                                      double tol) {
  extern __shared__ double eig_lds[];
  const int tid = threadIdx.x;
  const int m = n + (n & 1), P = m / 2;
  double* A = IN_LDS ? eig_lds : gA;
  double* cs = eig_lds + (IN_LDS ? (int64_t)m * m : 0);  // [P]
  double* sn = cs + P;                                  // [P]
  double* tt = sn + P;                                  // [P] t = s / c
  double* red16 = tt + P;                               // [16]
  int* pp = reinterpret_cast<int*>(red16 + 16);         // [P]
  int* qq = pp + P;                                     // [P]

  bool bad = false;
  double f2 = 0.0;
  for (int e = tid; e < m * m; e += EVAL_EIG_THREADS) {
    const int i = e / m, j = e % m;
    double v = 0.0;
    if (i < n && j < n) v = 0.5 * (a_in[(int64_t)i * n + j] + a_in[(int64_t)j * n + i]);
    bad |= !eval_finite(v);
    A[e] = v;
    f2 = fma(v, v, f2);
  }
  if (q)
    for (int e = tid; e < n * n; e += EVAL_EIG_THREADS) q[e] = (e / n == e % n) ? 1.0 : 0.0;
  bad = __syncthreads_or(bad);
  if (bad) {
    if (tid == 0) {
      info[0] = 0;
      info[1] = 2;
      off_out[0] = __builtin_nan("");
    }
    return;
  }
  const double fro2 = eval_eig_block_sum(f2, red16);
  int sweeps = 0, status = 0;
  double off2;
  for (;;) {
    double o2 = 0.0;
    for (int e = tid; e < m * m; e += EVAL_EIG_THREADS) {
      const double v = A[e];
      if (e / m != e % m) o2 = fma(v, v, o2);
    }
    off2 = eval_eig_block_sum(o2, red16);
    if (!eval_finite(off2) || !eval_finite(fro2)) {  // overflow of the squares: no result rather than a wrong one
      status = 2;
      break;
    }
    if (off2 <= tol * tol * fro2) break;  // converged (a zero matrix at once)
    if (sweeps == max_sweeps) {
      status = 1;
      break;
    }
    for (int r = 0; r < m - 1; ++r) {
      __syncthreads();  // the previous round's block updates are complete before its diagonal is read
      if (tid < P) {
        int p, qi;
        if (tid == 0) {
          p = r;
          qi = m - 1;
        } else {
          p = (r + tid) % (m - 1);
          qi = (r - tid + m - 1) % (m - 1);
        }
        if (p > qi) {
          const int t = p;
          p = qi;
          qi = t;
        }
        const double app = A[p * m + p], aqq = A[qi * m + qi], apq = A[p * m + qi];
        double c = 1.0, s = 0.0, t = 0.0;
        if (fabs(apq) > 1e-16 * sqrt(fabs(app * aqq))) {  // else negligible next to its diagonal: zeroed without a rotation
          const double tau = (aqq - app) / (2.0 * apq);
          t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + hypot(1.0, tau));
          c = 1.0 / sqrt(fma(t, t, 1.0));
          s = t * c;
        }
        pp[tid] = p;
        qq[tid] = qi;
        cs[tid] = c;
        sn[tid] = s;
        tt[tid] = t;
      }
      __syncthreads();
      for (int e = tid; e < P * P; e += EVAL_EIG_THREADS) {
        const int a = e / P, b = e % P;
        if (a > b) continue;
        const int p1 = pp[a], q1 = qq[a];
        if (a == b) {
          const double apq = A[p1 * m + q1], t = tt[a];
          A[p1 * m + p1] -= t * apq;
          A[q1 * m + q1] += t * apq;
          A[p1 * m + q1] = 0.0;
          A[q1 * m + p1] = 0.0;
          continue;
        }
        const int r2 = pp[b], t2 = qq[b];
        const double c1 = cs[a], s1 = sn[a], c2 = cs[b], s2 = sn[b];
        const double xpr = A[p1 * m + r2], xpt = A[p1 * m + t2], xqr = A[q1 * m + r2], xqt = A[q1 * m + t2];
        const double ypr = c2 * xpr - s2 * xpt, ypt = s2 * xpr + c2 * xpt;
        const double yqr = c2 * xqr - s2 * xqt, yqt = s2 * xqr + c2 * xqt;
        const double bpr = c1 * ypr - s1 * yqr, bqr = s1 * ypr + c1 * yqr;
        const double bpt = c1 * ypt - s1 * yqt, bqt = s1 * ypt + c1 * yqt;
        A[p1 * m + r2] = bpr;
        A[r2 * m + p1] = bpr;
        A[p1 * m + t2] = bpt;
        A[t2 * m + p1] = bpt;
        A[q1 * m + r2] = bqr;
        A[r2 * m + q1] = bqr;
        A[q1 * m + t2] = bqt;
        A[t2 * m + q1] = bqt;
      }
      if (q)
        for (int e = tid; e < n * P; e += EVAL_EIG_THREADS) {
          const int i = e / P, b = e % P;
          const int r2 = pp[b], t2 = qq[b];
          if (t2 >= n) continue;  // paired with the padding index: identity
          const double c2 = cs[b], s2 = sn[b];
          const double vr = q[(int64_t)i * n + r2], vt = q[(int64_t)i * n + t2];
          q[(int64_t)i * n + r2] = c2 * vr - s2 * vt;
          q[(int64_t)i * n + t2] = s2 * vr + c2 * vt;
        }
    }
    __syncthreads();
    ++sweeps;
  }
  for (int i = tid; i < n; i += EVAL_EIG_THREADS) w[i] = A[i * m + i];
  if (tid == 0) {
    info[0] = sweeps;
    info[1] = status;
    off_out[0] = sqrt(off2);
  }
}
