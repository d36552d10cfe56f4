// C ABI of the capture dataset (include/a2p_hip.h "capture dataset"; kernel in kernels_dataset.h).  Context-free: one launch on
// the caller's stream, the chunk table travels in the kernel arguments (no allocation, no copy, no synchronisation).
// Included at the end of a2p_lib.hip (set_err / ARG / HIPCHK).
#pragma once

extern "C" int a2p_dataset_batch(const a2p_dataset_take* takes, int32_t n_takes, int32_t channels, int32_t face,
                                 const int32_t* take_of, const int64_t* start_of, int32_t batch, int32_t frames, int32_t key_step,
                                 int32_t samples_per_frame, const double* mean, const double* std_dev, float audio_mean0,
                                 float audio_mean1, float audio_std, int32_t swap_channels, float* inp, float* keyframes,
                                 float* missing, float* audio, void* stream) {
  static_assert(DS_MAX_BATCH == A2P_DATASET_MAX_BATCH, "dataset batch limit");
  ARG(takes && take_of && start_of && mean && std_dev && inp && keyframes && missing && audio, "dataset_batch: null argument");
  ARG(n_takes >= 1, "dataset_batch: no takes");
  ARG(batch >= 1 && batch <= A2P_DATASET_MAX_BATCH, "dataset_batch: batch %d outside [1, %d]", batch, A2P_DATASET_MAX_BATCH);
  ARG(channels >= 1 && channels <= 4096 && frames >= 1 && frames <= (1 << 20) && key_step >= 1,
      "dataset_batch: bad shape C=%d T=%d step=%d", channels, frames, key_step);
  ARG(samples_per_frame >= 2 && samples_per_frame % 2 == 0 && samples_per_frame <= (1 << 16),
      "dataset_batch: samples_per_frame must be even (16-byte vectors of two stereo samples), got %d", samples_per_frame);
  ARG((reinterpret_cast<uintptr_t>(audio) & 15) == 0, "dataset_batch: the audio output must be 16-byte aligned");
  DatasetP p;
  memset(&p, 0, sizeof(p));
  for (int b = 0; b < batch; ++b) {
    const int32_t k = take_of[b];
    ARG(k >= 0 && k < n_takes, "dataset_batch: chunk %d names take %d of %d", b, k, n_takes);
    const a2p_dataset_take& t = takes[k];
    ARG(t.motion && t.audio, "dataset_batch: take %d has a null pointer", k);
    ARG((reinterpret_cast<uintptr_t>(t.audio) & 15) == 0, "dataset_batch: the audio of take %d must be 16-byte aligned", k);
    ARG(start_of[b] >= 0 && start_of[b] + frames <= t.frames, "dataset_batch: chunk %d = frames [%lld, %lld) of take %d, which has %lld",
        b, (long long)start_of[b], (long long)(start_of[b] + frames), k, (long long)t.frames);
    p.ch[b].motion = static_cast<const char*>(t.motion) + (size_t)start_of[b] * channels * (t.motion_f64 ? 8 : 4);
    p.ch[b].f64 = t.motion_f64 ? 1 : 0;
    p.ch[b].present = t.present ? t.present + start_of[b] : nullptr;
    p.ch[b].audio = t.audio + (size_t)start_of[b] * samples_per_frame * 2;
  }
  p.mean = mean; p.stdv = std_dev; p.inp = inp; p.kf = keyframes; p.miss = missing; p.audio = audio;
  p.B = batch; p.C = channels; p.T = frames; p.step = key_step; p.K = (frames + key_step - 1) / key_step;
  p.face = face ? 1 : 0; p.swap = swap_channels ? 1 : 0;
  p.am0 = audio_mean0; p.am1 = audio_mean1; p.astd = audio_std;
  p.n4 = (int64_t)frames * samples_per_frame / 2;
  p.tiles_c = (channels + DS_TILE - 1) / DS_TILE; p.tiles_t = (frames + DS_TILE - 1) / DS_TILE;
  // the grid follows the bytes: one workgroup per motion tile, one per 16 KiB of audio
  const int64_t per_wg = 256 * DS_AUDIO_VEC;
  const int64_t bpc = (p.n4 + per_wg - 1) / per_wg;
  const int64_t motion_blocks = (int64_t)p.tiles_c * p.tiles_t * batch;
  ARG(motion_blocks + bpc * batch < ((int64_t)1 << 31), "dataset_batch: batch too large for one launch");
  p.motion_blocks = (int)motion_blocks; p.audio_bpc = (int)bpc;
  dataset_batch_kernel<<<(unsigned)(motion_blocks + bpc * batch), 256, 0, (hipStream_t)stream>>>(p);
  HIPCHK(hipGetLastError());
  return 0;
}
