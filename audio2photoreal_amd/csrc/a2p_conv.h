// C ABI of the decoder layers (include/a2p_hip.h "decoder layers"; kernels in kernels_conv.h).  Context-free like the surface
// maps: weights, biases, masks and seam tables are device arrays the caller prepared once (audio2photoreal_amd/decoder.py folds
// and validates them on the host).  Included at the end of a2p_lib.hip (set_err / ARG / HIPCHK).
#pragma once

// [a, a + na) and [b, b + nb) in floats share an element
static inline bool conv_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  if (!a || !b || na <= 0 || nb <= 0) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

// Checks a source against the output plane and fills the kernel's view of it; `extent` gets the floats it spans.
static int conv_source(const char* name, const a2p_conv_source* s, int64_t N, int32_t groups, int32_t H, int32_t W, ConvSrc* out,
                       int32_t* per_group, int64_t* extent) {
  ARG(s->data, "conv2d_ub: %s.data is null", name);
  ARG(s->C >= 1 && s->C % groups == 0 && s->C / groups <= A2P_CONV_MAX_CHANNELS,
      "conv2d_ub: %s.C=%d with groups=%d: need a multiple of groups with at most %d channels per group", name, s->C, groups,
      A2P_CONV_MAX_CHANNELS);
  ARG(s->H >= 1 && s->H <= A2P_CONV_MAX_SIZE && s->W >= 1 && s->W <= A2P_CONV_MAX_SIZE, "conv2d_ub: %s is %d x %d, outside [1, %d]", name,
      s->H, s->W, A2P_CONV_MAX_SIZE);
  const int64_t frame = (int64_t)s->C * s->H * s->W;
  ARG(s->frame_stride >= frame, "conv2d_ub: %s.frame_stride=%lld is below C H W = %lld", name, (long long)s->frame_stride,
      (long long)frame);
  out->p = s->data;
  out->n_stride = s->frame_stride;
  out->Hs = s->H;
  out->Ws = s->W;
  out->up = s->H != H || s->W != W;
  out->sy = H > 1 ? (float)(s->H - 1) / (float)(H - 1) : 0.0f;
  out->sx = W > 1 ? (float)(s->W - 1) / (float)(W - 1) : 0.0f;
  *per_group = s->C / groups;
  *extent = N > 0 ? (N - 1) * s->frame_stride + frame : 0;
  return 0;
}

extern "C" int a2p_conv2d_ub(const a2p_conv2d_desc* d, void* stream) {
  static_assert(CONV_MAX_CHANNELS == A2P_CONV_MAX_CHANNELS && CONV_MAX_SIZE == A2P_CONV_MAX_SIZE, "decoder layer limits");
  static_assert((int64_t)CONV_MAX_SIZE * CONV_MAX_SIZE <= 0x7fffffffll, "a plane must fit in int32");
  ARG(d, "conv2d_ub: null descriptor");
  ARG(d->weight && d->out, "conv2d_ub: null weight or out");
  ARG(d->k == 1 || d->k == 3, "conv2d_ub: k=%d, need 1 or 3", d->k);
  ARG(d->groups >= 1, "conv2d_ub: groups=%d, need >= 1", d->groups);
  ARG(d->H >= 1 && d->H <= A2P_CONV_MAX_SIZE && d->W >= 1 && d->W <= A2P_CONV_MAX_SIZE, "conv2d_ub: the output is %d x %d, outside [1, %d]",
      d->H, d->W, A2P_CONV_MAX_SIZE);
  ARG(d->C_out >= 1 && d->C_out % d->groups == 0 && d->C_out / d->groups <= A2P_CONV_MAX_CHANNELS,
      "conv2d_ub: C_out=%d with groups=%d: need a multiple of groups with at most %d channels per group", d->C_out, d->groups,
      A2P_CONV_MAX_CHANNELS);
  ARG(d->bias_mode >= A2P_CONV_BIAS_NONE && d->bias_mode <= A2P_CONV_BIAS_UNTIED, "conv2d_ub: bias_mode=%d outside [0, 2]", d->bias_mode);
  ARG(d->bias_mode == A2P_CONV_BIAS_NONE || d->bias, "conv2d_ub: bias_mode=%d needs a bias", d->bias_mode);
  ARG(d->skip_mode >= A2P_CONV_SKIP_NONE && d->skip_mode <= A2P_CONV_SKIP_CONV, "conv2d_ub: skip_mode=%d outside [0, 2]", d->skip_mode);
  ARG(d->skip_mode != A2P_CONV_SKIP_TENSOR || d->skip, "conv2d_ub: skip_mode=1 needs the skip tensor");
  ARG(d->skip_mode != A2P_CONV_SKIP_CONV || d->skip_weight, "conv2d_ub: skip_mode=2 needs skip_weight");
  ARG(d->N >= 0, "conv2d_ub: N=%lld is negative", (long long)d->N);

  ConvParams p = {};
  int64_t x_extent = 0, s_extent = 0;
  if (int rc = conv_source("x", &d->x, d->N, d->groups, d->H, d->W, &p.x, &p.cin_pg, &x_extent)) return rc;
  if (d->skip_mode == A2P_CONV_SKIP_CONV)
    if (int rc = conv_source("skip_src", &d->skip_src, d->N, d->groups, d->H, d->W, &p.s, &p.cs_pg, &s_extent)) return rc;
  p.cout_pg = d->C_out / d->groups;
  const int co_t = p.cout_pg <= 4 ? 4 : 8;
  p.chunks = (p.cout_pg + co_t - 1) / co_t;
  p.tiles_x = (d->W + CONV_TW - 1) / CONV_TW;
  p.tiles = p.tiles_x * ((d->H + CONV_TH - 1) / CONV_TH);
  ARG(d->N * p.tiles <= 0x7fffffff, "conv2d_ub: N=%lld frames x %d tiles exceed the grid", (long long)d->N, p.tiles);
  ARG((int64_t)d->groups * p.chunks <= 65535, "conv2d_ub: groups=%d x %d channel chunks exceed the grid", d->groups, p.chunks);

  const int64_t HW = (int64_t)d->H * d->W, out_n = d->N * d->C_out * HW, KK = d->k * d->k;
  const struct { const char* name; const void* ptr; int64_t n; } inputs[] = {
      {"x", d->x.data, x_extent},
      {"weight", d->weight, (int64_t)d->C_out * p.cin_pg * KK},
      {"bias", d->bias_mode ? d->bias : nullptr, d->bias_mode == A2P_CONV_BIAS_UNTIED ? d->C_out * HW : d->C_out},
      {"skip", d->skip_mode == A2P_CONV_SKIP_TENSOR ? d->skip : nullptr, out_n},
      {"skip_src", d->skip_mode == A2P_CONV_SKIP_CONV ? d->skip_src.data : nullptr, s_extent},
      {"skip_weight", d->skip_mode == A2P_CONV_SKIP_CONV ? d->skip_weight : nullptr, (int64_t)d->C_out * p.cs_pg},
      {"skip_bias", d->skip_mode == A2P_CONV_SKIP_CONV ? d->skip_bias : nullptr, d->C_out},
      {"mask", d->mask, HW}};
  for (const auto& in : inputs)
    ARG(!conv_overlap(d->out, out_n, in.ptr, in.n), "conv2d_ub: out must not alias an input (it overlaps %s)", in.name);
  if (d->N == 0) return 0;

  p.w = d->weight;
  p.bias = d->bias;
  p.skip = d->skip;
  p.sw = d->skip_weight;
  p.sb = d->skip_bias;
  p.mask = d->mask;
  p.out = d->out;
  p.C_out = d->C_out;
  p.H = d->H;
  p.W = d->W;
  p.bias_mode = d->bias_mode;
  p.act = d->act != 0;
  p.skip_mode = d->skip_mode;
  p.slope = d->slope;
  const dim3 grid((unsigned)(d->N * p.tiles), (unsigned)(d->groups * p.chunks));
  hipStream_t s = (hipStream_t)stream;
  if (d->k == 3 && co_t == 8) conv2d_ub_kernel<3, 8><<<grid, CONV_THREADS, 0, s>>>(p);
  else if (d->k == 3) conv2d_ub_kernel<3, 4><<<grid, CONV_THREADS, 0, s>>>(p);
  else if (co_t == 8) conv2d_ub_kernel<1, 8><<<grid, CONV_THREADS, 0, s>>>(p);
  else conv2d_ub_kernel<1, 4><<<grid, CONV_THREADS, 0, s>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_seam_impaint(float* value, int64_t planes, int32_t H, int32_t W, const int32_t* dst, const int32_t* src, int32_t P,
                                float* scratch, void* stream) {
  ARG(value && dst && src && scratch, "seam_impaint: null argument");
  ARG(H >= 1 && H <= A2P_CONV_MAX_SIZE && W >= 1 && W <= A2P_CONV_MAX_SIZE, "seam_impaint: a %d x %d plane, outside [1, %d]", H, W,
      A2P_CONV_MAX_SIZE);
  ARG(planes >= 0 && P >= 0, "seam_impaint: planes=%lld, pairs=%d: both must be >= 0", (long long)planes, P);
  const int64_t work = planes * P, blocks = (work + SEAM_THREADS - 1) / SEAM_THREADS;
  ARG(blocks <= 0x7fffffff, "seam_impaint: %lld planes x %d pairs exceed the grid", (long long)planes, P);
  ARG(!conv_overlap(scratch, work, value, planes * H * W) && !conv_overlap(scratch, work, dst, P) && !conv_overlap(scratch, work, src, P),
      "seam_impaint: scratch must not alias value or the tables");
  if (work == 0) return 0;
  const int64_t HW = (int64_t)H * W;
  seam_gather_kernel<<<(unsigned)blocks, SEAM_THREADS, 0, (hipStream_t)stream>>>(value, planes, HW, src, P, scratch);
  seam_scatter_kernel<<<(unsigned)blocks, SEAM_THREADS, 0, (hipStream_t)stream>>>(value, planes, HW, dst, P, scratch);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int a2p_seam_resample(const float* tex, int64_t planes, int32_t H, int32_t W, const float* uvs, const float* weights,
                                 float* out, void* stream) {
  ARG(tex && uvs && weights && out, "seam_resample: null argument");
  ARG(H >= 1 && H <= A2P_CONV_MAX_SIZE && W >= 1 && W <= A2P_CONV_MAX_SIZE, "seam_resample: a %d x %d plane, outside [1, %d]", H, W,
      A2P_CONV_MAX_SIZE);
  ARG(planes >= 0, "seam_resample: planes=%lld is negative", (long long)planes);
  const int64_t HW = (int64_t)H * W, tblocks = (HW + SEAM_THREADS - 1) / SEAM_THREADS;
  const int64_t groups = (planes + SEAM_PLANE_GROUP - 1) / SEAM_PLANE_GROUP;
  ARG(groups * tblocks <= 0x7fffffff, "seam_resample: %lld plane groups x %lld texel blocks exceed the grid", (long long)groups,
      (long long)tblocks);
  ARG(!conv_overlap(out, planes * HW, tex, planes * HW) && !conv_overlap(out, planes * HW, uvs, 2 * HW) &&
          !conv_overlap(out, planes * HW, weights, HW),
      "seam_resample: out must not alias an input");
  if (planes == 0) return 0;
  seam_resample_kernel<<<(unsigned)(groups * tblocks), SEAM_THREADS, 0, (hipStream_t)stream>>>(tex, planes, H, W, uvs, weights, tblocks,
                                                                                              out);
  HIPCHK(hipGetLastError());
  return 0;
}
