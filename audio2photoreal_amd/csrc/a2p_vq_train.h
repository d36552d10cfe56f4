// Host side of the fused tokenizer training step (kernels_vq_train.h); included from a2p_lib.hip.
#pragma once

struct VqTrainPlan {
  int64_t n_params, ew[5], eb[5], dw[5], db[5], pms_off, pms_n;
  int64_t off_act, off_pred, off_dpred, off_res, off_rowcommit, off_seqloss, off_norms, off_rawcount, off_grads, floats;
  size_t lds;
};

static int vq_train_plan(int32_t batch, int32_t T, int32_t depth, int32_t categories, int32_t latent, int32_t vertices, VqTrainPlan* pl) {
  ARG(depth >= 1 && depth <= 8 && batch >= 1 && T >= 1 && latent >= 4 && latent % 4 == 0 && vertices >= 1 && categories >= 1,
      "bad VQ shape (the latent width must be a multiple of 4, depth at most 8)");
  const int64_t e = latent, nv = vertices, R = (int64_t)T + 7;
  // two ping-pong buffers of (T + 7) rows in LDS plus the reduction scratch
  pl->lds = (size_t)2 * R * e * 4;
  ARG(pl->lds + 64 <= 64 * 1024, "VQ training step of %d frames x %d latent needs %zu bytes of LDS (T <= %d at this width)", T, latent,
      pl->lds + 64, (int)((64 * 1024 - 64) / (8 * e) - 7));
  int64_t o = 0;
  pl->ew[0] = o; o += e * nv; pl->eb[0] = o; o += e;
  for (int i = 1; i < 5; ++i) { pl->ew[i] = o; o += e * e * 2; pl->eb[i] = o; o += e; }
  pl->pms_off = o; pl->pms_n = e * nv + e; o += pl->pms_n;
  for (int i = 0; i < 4; ++i) { pl->dw[i] = o; o += e * e * 2; pl->db[i] = o; o += e; }
  pl->dw[4] = o; o += nv * e; pl->db[4] = o; o += nv;
  pl->n_params = o;
  const int64_t N = (int64_t)batch * T;
  int64_t w = 0;
  auto take = [&](int64_t n) { const int64_t at = w; w += (n + 3) / 4 * 4; return at; };
  pl->off_act = take((int64_t)batch * VQT_SLOTS * R * e);
  pl->off_pred = take(N * nv);
  pl->off_dpred = take(N * nv);
  pl->off_res = take(N * depth * e);
  pl->off_rowcommit = take(N * depth);
  pl->off_seqloss = take((int64_t)batch * 2);
  pl->off_norms = take((int64_t)depth * categories);
  pl->off_rawcount = take((int64_t)depth * categories);
  pl->off_grads = take(pl->n_params);
  pl->floats = w;
  return 0;
}

extern "C" int a2p_vq_train_workspace_bytes(int32_t batch, int32_t T, int32_t depth, int32_t categories, int32_t latent, int32_t vertices,
                                            int64_t* bytes_out) {
  ARG(bytes_out, "null argument");
  VqTrainPlan pl;
  CHK(vq_train_plan(batch, T, depth, categories, latent, vertices, &pl));
  *bytes_out = pl.floats * 4;
  return 0;
}

extern "C" int a2p_vq_train_step(const float* x, int32_t batch, int32_t T, int32_t depth, int32_t categories, int32_t latent,
                                 int32_t vertices, float* params, float* exp_avg, float* exp_avg_sq, float* const* embed,
                                 float* const* embed_avg, float* const* cluster_size, const a2p_vq_train_hyper* hp, int64_t* tokens_out,
                                 float* loss_record, float* grads_out, void* workspace, int64_t workspace_bytes, void* stream) {
  ARG(x && params && exp_avg && exp_avg_sq && embed && embed_avg && cluster_size && hp && tokens_out && loss_record && workspace,
      "null argument");
  VqTrainPlan pl;
  CHK(vq_train_plan(batch, T, depth, categories, latent, vertices, &pl));
  ARG(workspace_bytes >= pl.floats * 4, "the workspace holds %lld bytes, the step needs %lld (a2p_vq_train_workspace_bytes)",
      (long long)workspace_bytes, (long long)pl.floats * 4);
  ARG(((uintptr_t)workspace & 15) == 0, "the workspace must be 16-byte aligned");
  ARG(hp->bias_correction1 > 0.0 && hp->bias_correction2 > 0.0 && hp->ema_decay >= 0.0 && hp->ema_decay <= 1.0 && hp->lr >= 0.0 &&
          hp->weight_decay >= 0.0 && hp->commit >= 0.0 && hp->loss_vel >= 0.0 && hp->ema_epsilon >= 0.0,
      "bad hyper-parameter (lr %g, bias corrections %g %g, weight_decay %g, commit %g, loss_vel %g, EMA decay %g, epsilon %g)", hp->lr,
      hp->bias_correction1, hp->bias_correction2, hp->weight_decay, hp->commit, hp->loss_vel, hp->ema_decay, hp->ema_epsilon);
  VqTrainP p;
  memset(&p, 0, sizeof(p));
  float* ws = reinterpret_cast<float*>(workspace);
  p.x = x; p.params = params; p.m1 = exp_avg; p.m2 = exp_avg_sq;
  p.grads = grads_out ? grads_out : ws + pl.off_grads;
  for (int i = 0; i < depth; ++i) {
    p.embed[i] = embed[i]; p.embed_avg[i] = embed_avg[i]; p.cluster[i] = cluster_size[i];
    ARG(p.embed[i] && p.embed_avg[i] && p.cluster[i], "null codebook %d", i);
  }
  for (int i = 0; i < 5; ++i) { p.ew[i] = pl.ew[i]; p.eb[i] = pl.eb[i]; p.dw[i] = pl.dw[i]; p.db[i] = pl.db[i]; }
  p.pms_off = pl.pms_off; p.pms_n = pl.pms_n; p.n_params = pl.n_params;
  p.B = batch; p.T = T; p.depth = depth; p.categories = categories; p.e = latent; p.nv = vertices;
  p.commit = (float)hp->commit; p.loss_vel = (float)hp->loss_vel;
  p.decay = (float)hp->ema_decay; p.one_minus_decay = (float)(1.0 - hp->ema_decay); p.eps_ema = (float)hp->ema_epsilon;
  p.lr_wd = (float)(hp->lr * hp->weight_decay); p.step_size = (float)(hp->lr / hp->bias_correction1);
  p.bc2_sqrt = (float)sqrt(hp->bias_correction2);
  p.act = ws + pl.off_act; p.pred = ws + pl.off_pred; p.dpred = ws + pl.off_dpred; p.res = ws + pl.off_res;
  p.rowcommit = ws + pl.off_rowcommit; p.seqloss = ws + pl.off_seqloss; p.norms = ws + pl.off_norms; p.rawcount = ws + pl.off_rawcount;
  p.tokens = tokens_out; p.record = loss_record;

  VqWgradP g;
  memset(&g, 0, sizeof(g));
  const int e = latent, nv = vertices;
  const int dil[4] = {1, 2, 3, 1}, fo[4] = {1, 3, 6, 7};
  int64_t base = 0;
  auto layer = [&](int i, int64_t w_off, int64_t b_off, int in_slot, int g_slot, int cin, int cout, int ks, int d, int first) {
    g.L[i] = VqtLayer{w_off, b_off, base, in_slot, g_slot, cin, cout, ks, d, first};
    base += (int64_t)cout * cin * ks + cout;
  };
  layer(0, pl.ew[0], pl.eb[0], VQT_SLOT_X, VQT_GE0, nv, e, 1, 1, 0);
  for (int l = 0; l < 4; ++l) layer(1 + l, pl.ew[l + 1], pl.eb[l + 1], VQT_A0 + l, VQT_GE1 + l, e, e, 2, dil[l], fo[l]);
  for (int l = 0; l < 4; ++l) layer(5 + l, pl.dw[l], pl.db[l], VQT_DIN + l, VQT_GD0 + l, e, e, 2, dil[l], fo[l]);
  layer(9, pl.dw[4], pl.db[4], VQT_D3, VQT_SLOT_DPRED, e, nv, 1, 1, 7);
  g.total = base;
  g.x = x; g.act = p.act; g.dpred = p.dpred; g.grads = p.grads; g.B = batch; g.T = T; g.e = e; g.nv = nv;

  hipStream_t s = (hipStream_t)stream;
  const int code_blocks = (depth * categories + 3) / 4;
  vqt_norms_kernel<<<code_blocks, 256, 0, s>>>(p);
  vqt_fwd_bwd_kernel<<<batch, 256, pl.lds, s>>>(p);
  vqt_wgrad_kernel<<<(unsigned)((g.total + 63) / 64), 256, 0, s>>>(g);
  vqt_stats_kernel<<<code_blocks, 256, 0, s>>>(p);
  vqt_update_kernel<<<(unsigned)(depth + 1 + (pl.n_params + 255) / 256), 256, 0, s>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}
