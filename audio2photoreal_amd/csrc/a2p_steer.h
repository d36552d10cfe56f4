// C ABI of joint steering (include/a2p_hip.h "steering joints to 3D targets"; kernel in kernels_steer.h).  a2p_skin_steer is
// context-free like a2p_skin_states; a2p_sample_step_steer is a2p_sample_step_inpaint's shape with the steer between the guided
// model output and the unchanged step tail.  Included at the end of a2p_lib.hip (set_err / ARG / HIPCHK, run_forward,
// guide_combine, launch_step_tail).
#pragma once

static int steer_params(const a2p_steer* a, int64_t N, const char* who, SteerP& p) {
  static_assert(STEER_MAX_CONSTRAINTS == A2P_STEER_MAX_CONSTRAINTS && STEER_REACH == A2P_STEER_REACH && STEER_AIM == A2P_STEER_AIM,
                "steering limits");
  ARG(a, "%s: null steer description", who);
  ARG(a->row_ptr && a->cols && a->vals && a->offsets && a->joint_offset && a->pre_rotation && a->parents && a->order &&
          a->level_start && a->child_ptr && a->child_idx && a->col_ptr && a->rows && a->cvals,
      "%s: null skeleton table", who);
  ARG(a->J >= 1 && a->J <= A2P_SKIN_MAX_JOINTS, "%s: J=%d outside [1, %d]", who, a->J, A2P_SKIN_MAX_JOINTS);
  ARG(a->P_pos >= 1 && a->P_scale >= 0 && a->P_pos + (int64_t)a->P_scale <= A2P_SKIN_MAX_PARAMS,
      "%s: need P_pos >= 1, P_scale >= 0, P_pos + P_scale <= %d (got %d + %d)", who, A2P_SKIN_MAX_PARAMS, a->P_pos, a->P_scale);
  ARG(a->P_scale == 0 || a->scale, "%s: P_scale=%d but scale is null", who, a->P_scale);
  ARG(a->n_levels >= 1 && a->n_levels <= a->J, "%s: n_levels=%d outside [1, J=%d]", who, a->n_levels, a->J);
  ARG(a->K >= 1 && a->K <= A2P_STEER_MAX_CONSTRAINTS, "%s: K=%d constraints outside [1, %d]", who, a->K, A2P_STEER_MAX_CONSTRAINTS);
  ARG(a->joints_host && a->kinds_host && a->axes_host && a->targets && a->weights, "%s: null constraint array", who);
  ARG(a->iterations >= 0 && a->iterations <= 1024, "%s: iterations=%d outside [0, 1024]", who, a->iterations);
  ARG(a->alpha > 0.0f && a->alpha <= 3.4028234e38f && a->max_step > 0.0f && a->max_step <= 3.4028234e38f,
      "%s: alpha=%g and max_step=%g must be positive and finite", who, (double)a->alpha, (double)a->max_step);
  ARG(N >= 0 && N <= 0x7fffffff, "%s: N=%lld outside [0, 2^31)", who, (long long)N);
  memset(&p, 0, sizeof(p));
  for (int k = 0; k < a->K; ++k) {
    ARG(a->joints_host[k] >= 0 && a->joints_host[k] < a->J, "%s: constraint %d: joint %d outside [0, J=%d)", who, k, a->joints_host[k], a->J);
    ARG(a->kinds_host[k] == A2P_STEER_REACH || a->kinds_host[k] == A2P_STEER_AIM, "%s: constraint %d: kind %d", who, k, a->kinds_host[k]);
    p.joint[k] = a->joints_host[k];
    p.kind[k] = a->kinds_host[k];
    for (int i = 0; i < 3; ++i) {
      ARG(fabsf(a->axes_host[3 * k + i]) <= 3.4028234e38f, "%s: constraint %d: axis is not finite", who, k);
      p.axis[k][i] = a->axes_host[3 * k + i];
    }
  }
  p.mean = a->mean; p.std = a->std; p.scale = a->scale; p.scale_stride = a->scale_per_frame ? (int64_t)a->P_scale : 0;
  p.P_pos = a->P_pos; p.P_scale = a->P_scale; p.J = a->J; p.n_levels = a->n_levels;
  p.row_ptr = a->row_ptr; p.cols = a->cols; p.vals = a->vals; p.col_ptr = a->col_ptr; p.rows = a->rows; p.cvals = a->cvals;
  p.offsets = a->offsets; p.joint_offset = a->joint_offset; p.pre_rotation = a->pre_rotation;
  p.parents = a->parents; p.order = a->order; p.level_start = a->level_start; p.child_ptr = a->child_ptr; p.child_idx = a->child_idx;
  p.gx = a->global_scaling[0]; p.gy = a->global_scaling[1]; p.gz = a->global_scaling[2];
  p.K = a->K; p.targets = a->targets; p.weights = a->weights;
  p.alpha = a->alpha; p.max_step = a->max_step; p.iterations = a->iterations;
  return 0;
}

static int launch_steer(const SteerP& p, int64_t N, hipStream_t s) {
  const size_t lds = ((size_t)16 * p.J + p.P_pos + p.P_scale + 2 * p.P_pos + 2 * SKIN_THREADS + 8 * STEER_MAX_CONSTRAINTS) * sizeof(float);
  if (lds > 64 * 1024)   // <= 78.5 KiB: beyond the 64 KiB a kernel gets without asking
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(skin_steer_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
  skin_steer_kernel<<<(unsigned)N, SKIN_THREADS, lds, s>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_skin_steer(const a2p_steer* steer, const float* z_in, int64_t z_in_stride, int64_t N, float* z_out,
                              int64_t z_out_stride, float* loss, float* grad, void* stream) {
  SteerP p;
  CHK(steer_params(steer, N, "skin_steer", p));
  ARG(z_in && z_out, "skin_steer: null argument");
  ARG(z_in_stride >= p.P_pos && z_out_stride >= p.P_pos, "skin_steer: row strides %lld / %lld are shorter than P_pos=%d",
      (long long)z_in_stride, (long long)z_out_stride, p.P_pos);
  ARG(z_out != z_in || z_out_stride == z_in_stride, "skin_steer: z_out aliases z_in with another row stride");
  if (N == 0) return 0;
  p.za = z_in; p.oa = z_out; p.in_row = z_in_stride; p.out_row = z_out_stride; p.T = (int)N;
  p.loss = loss; p.grad = grad;
  return launch_steer(p, N, (hipStream_t)stream);
}

extern "C" int a2p_sample_step_steer(a2p_ctx* c, int32_t sampler, const float* x, const int64_t* t_idx, const int64_t* timestep_map,
                                     const float* tables, int32_t n_steps, const float* scale, const float* noise, float eta,
                                     int32_t clip_denoised, const a2p_steer* steer, float* x_next, float* pred_xstart,
                                     void* stream) {
  ARG(c && x && t_idx && timestep_map && tables && x_next, "null argument");
  ARG(sampler == A2P_SAMPLER_DDIM || sampler == A2P_SAMPLER_DDPM, "bad sampler");
  ARG(sampler == A2P_SAMPLER_DDIM || noise, "DDPM step needs noise");
  ARG(scale, "classifier-free guidance scale required");
  if (!c->prepared) {
    set_err("denoise before a2p_prepare_cond");
    return A2P_ERR_STATE;
  }
  const int64_t N = (int64_t)c->pB * c->pT;
  SteerP p;
  CHK(steer_params(steer, N, "sample_step_steer", p));
  ARG(c->pose && c->C == p.P_pos, "sample_step_steer: a pose context whose nfeats (%d) is the skeleton's P_pos (%d) is required", c->C,
      p.P_pos);
  ARG(!steer->scale_per_frame, "sample_step_steer: the scale parameters are shared by all frames (scale_per_frame = 0)");
  hipStream_t s = (hipStream_t)stream;
  int64_t* t_orig = reinterpret_cast<int64_t*>(c->tmpa.p);
  map_timesteps_kernel<<<1, 256, 0, s>>>(t_idx, timestep_map, t_orig, c->pB);
  int rows = 0;
  CHK(run_forward(c, x, t_orig, guided_pass(c), &rows, s));
  CHK(guide_combine(c, guided_pass(c), scale, rows, s));
  // the guided output of a frame from the two sequence blocks, steered, back into both (guide_combine_kernel's hand-over)
  float* mo = c->mo.f();
  p.za = p.oa = mo;
  p.zu = p.ou = mo + (int64_t)c->pB * rows * c->C;
  p.cfg = scale;
  p.in_seq = p.out_seq = (int64_t)rows * c->C;
  p.in_row = p.out_row = c->C;
  p.T = c->pT;
  CHK(launch_steer(p, N, s));
  StepP sp;
  memset(&sp, 0, sizeof(sp));
  sp.mo = mo; sp.mo_seq_rows = rows; sp.mo_ld = c->C; sp.B = c->pB; sp.C = c->C; sp.Tn = c->pT;
  sp.pass = A2P_PASS_CFG; sp.scale = scale; sp.sampler = sampler; sp.x = x; sp.t_idx = t_idx; sp.tables = tables;
  sp.n_steps = n_steps; sp.noise = noise; sp.eta = eta; sp.clip = clip_denoised; sp.x_next = x_next; sp.x0 = pred_xstart;
  sp.nonfinite = reinterpret_cast<int*>(c->nonfinite.p);
  return launch_step_tail(c, sp, s);
}
