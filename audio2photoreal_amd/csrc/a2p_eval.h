// C ABI of the motion evaluation (include/a2p_hip.h "motion evaluation"; kernels in kernels_eval.h).  Context-free like the
// stand-alone sampler arithmetic.  Included at the end of a2p_lib.hip (set_err / ARG / HIPCHK).
#pragma once

extern "C" int a2p_eval_moments(const void* x, int32_t x_f64, int32_t S, int32_t C, int32_t T, int32_t reps, double* mu, double* cov,
                                double* mu_v, double* cov_v, double* sums, double* workspace, int32_t* nonfinite, void* stream) {
  ARG(x && mu && cov && mu_v && cov_v && sums && workspace && nonfinite, "eval_moments: null argument");
  ARG(S >= 1 && C >= 1 && C <= A2P_EVAL_MAX_CHANNELS && T >= 2, "eval_moments: need S >= 1, 1 <= C <= %d, T >= 2 (got S=%d C=%d T=%d)",
      A2P_EVAL_MAX_CHANNELS, S, C, T);
  ARG((int64_t)S * C * T <= ((int64_t)1 << 40), "eval_moments: input too large");
  ARG(reps >= 0 && (reps == 0 || S % reps == 0), "eval_moments: reps=%d does not divide S=%d", reps, S);
  static_assert(EVAL_XV_BLOCKS == A2P_EVAL_XV_PARTIALS && EVAL_NSPLIT == A2P_EVAL_NSPLIT, "eval workspace layout");
  hipStream_t s = (hipStream_t)stream;
  double* varsum = workspace;                       // [C]
  double* xv = varsum + C;                          // [A2P_EVAL_XV_PARTIALS]
  double* part = xv + A2P_EVAL_XV_PARTIALS;         // [A2P_EVAL_NSPLIT, C, C]
  const int64_t CC = (int64_t)C * C;
  const dim3 cov_grid((C + 31) / 32, (C + 31) / 32, EVAL_NSPLIT);
  const int fin_grid = (int)((CC + 255) / 256);
  if (x_f64) {
    const double* xd = static_cast<const double*>(x);
    eval_channel_kernel<double><<<C, 256, 0, s>>>(xd, S, C, T, mu, mu_v, varsum, nonfinite);
    if (reps) eval_crossvar_kernel<double><<<EVAL_XV_BLOCKS, 256, 0, s>>>(xd, reps, (int64_t)(S / reps) * C * T, xv);
    eval_cov_kernel<double, false><<<cov_grid, 256, 0, s>>>(xd, S, C, T, mu, part);
    eval_cov_finish_kernel<<<fin_grid, 256, 0, s>>>(part, CC, (int64_t)S * T, cov);
    eval_cov_kernel<double, true><<<cov_grid, 256, 0, s>>>(xd, S, C, T, mu_v, part);
  } else {
    const float* xf = static_cast<const float*>(x);
    eval_channel_kernel<float><<<C, 256, 0, s>>>(xf, S, C, T, mu, mu_v, varsum, nonfinite);
    if (reps) eval_crossvar_kernel<float><<<EVAL_XV_BLOCKS, 256, 0, s>>>(xf, reps, (int64_t)(S / reps) * C * T, xv);
    eval_cov_kernel<float, false><<<cov_grid, 256, 0, s>>>(xf, S, C, T, mu, part);
    eval_cov_finish_kernel<<<fin_grid, 256, 0, s>>>(part, CC, (int64_t)S * T, cov);
    eval_cov_kernel<float, true><<<cov_grid, 256, 0, s>>>(xf, S, C, T, mu_v, part);
  }
  eval_cov_finish_kernel<<<fin_grid, 256, 0, s>>>(part, CC, (int64_t)S * (T - 1), cov_v);
  eval_sums_kernel<<<1, 256, 0, s>>>(varsum, C, xv, reps ? EVAL_XV_BLOCKS : 0, sums);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_eval_pair_dist(const void* x, int32_t x_f64, int32_t S, int32_t C, int32_t T, const int64_t* idx1, const int64_t* idx2,
                                  int64_t times, double* dist, int32_t* nonfinite, void* stream) {
  ARG(x && idx1 && idx2 && dist && nonfinite, "eval_pair_dist: null argument");
  ARG(S >= 1 && C >= 1 && C <= A2P_EVAL_MAX_CHANNELS && T >= 1, "eval_pair_dist: bad shape S=%d C=%d T=%d", S, C, T);
  ARG(times >= 1 && times <= ((int64_t)1 << 31), "eval_pair_dist: bad times %lld", (long long)times);
  hipStream_t s = (hipStream_t)stream;
  const int grid = (int)((times + 3) / 4);
  if (x_f64)
    eval_pair_dist_kernel<double><<<grid, 256, 0, s>>>(static_cast<const double*>(x), S, C, T, idx1, idx2, times, dist, nonfinite);
  else
    eval_pair_dist_kernel<float><<<grid, 256, 0, s>>>(static_cast<const float*>(x), S, C, T, idx1, idx2, times, dist, nonfinite);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_eval_gemm_f64(int32_t n, const double* a, int64_t a_rs, int64_t a_cs, const double* d, const double* b, int64_t b_rs,
                                 int64_t b_cs, double* c, void* stream) {
  ARG(a && b && c, "eval_gemm_f64: null argument");
  ARG(n >= 1 && n <= A2P_EVAL_MAX_CHANNELS, "eval_gemm_f64: n=%d outside [1, %d]", n, A2P_EVAL_MAX_CHANNELS);
  ARG(c != a && c != b && c != d, "eval_gemm_f64: c must not alias an input");
  const dim3 grid((n + 15) / 16, (n + 15) / 16);
  eval_gemm_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(n, a, a_rs, a_cs, d, b, b_rs, b_cs, c);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_eval_eigh(const double* a, int32_t n, double* w, double* q, double* workspace, int32_t* sweeps_host, double* off_host,
                             void* stream) {
  ARG(a && w && workspace, "eval_eigh: null argument");
  ARG(n >= 1 && n <= A2P_EVAL_MAX_CHANNELS, "eval_eigh: n=%d outside [1, %d]", n, A2P_EVAL_MAX_CHANNELS);
  ARG(q != a && w != a, "eval_eigh: outputs must not alias the input");
  hipStream_t s = (hipStream_t)stream;
  const int m = n + (n & 1), P = m / 2;
  // workspace: [m * m] the matrix (n > 128) | info (2 ints) | off (1 double)
  double* gA = workspace;
  int* info = reinterpret_cast<int*>(workspace + (int64_t)m * m);
  double* off = workspace + (int64_t)m * m + 1;
  const size_t small = (size_t)(4 * P + 16) * sizeof(double) + (size_t)2 * P * sizeof(int);
  if (m <= EVAL_EIG_LDS_MAX) {
    const size_t lds = (size_t)m * m * sizeof(double) + small;
    // opt in to the largest size this kernel asks for (m = 128).  The runtime refused 160 KiB ("invalid argument"); should it
    // refuse this too, the launch itself reports an LDS request it cannot meet (hipGetLastError below)
    static bool attr_set = false;
    if (!attr_set) {
      const size_t max_lds = (size_t)EVAL_EIG_LDS_MAX * EVAL_EIG_LDS_MAX * sizeof(double) +
                             (size_t)(2 * EVAL_EIG_LDS_MAX + 16) * sizeof(double) + (size_t)EVAL_EIG_LDS_MAX * sizeof(int);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(eval_jacobi_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)max_lds);
      (void)hipGetLastError();
      attr_set = true;
    }
    eval_jacobi_kernel<true><<<1, EVAL_EIG_THREADS, lds, s>>>(a, n, w, q, gA, info, off, EVAL_EIG_MAX_SWEEPS, EVAL_EIG_TOL);
  } else {
    eval_jacobi_kernel<false><<<1, EVAL_EIG_THREADS, small, s>>>(a, n, w, q, gA, info, off, EVAL_EIG_MAX_SWEEPS, EVAL_EIG_TOL);
  }
  HIPCHK(hipGetLastError());
  int32_t h_info[2] = {0, 0};
  double h_off = 0.0;
  HIPCHK(hipMemcpyAsync(h_info, info, sizeof(h_info), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&h_off, off, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (sweeps_host) *sweeps_host = h_info[0];
  if (off_host) *off_host = h_off;
  if (h_info[1] == 2) {
    set_err("eval_eigh: the %d x %d input holds non-finite values (or its squares overflow)", n, n);
    return A2P_ERR_NONFINITE;
  }
  if (h_info[1] != 0) {
    set_err("eval_eigh: Jacobi did not converge in %d sweeps (off-diagonal norm %g)", h_info[0], h_off);
    return A2P_ERR_NOCONVERGE;
  }
  return 0;
}
