"""float64 numpy restatement of a conversation's y["audio"] (sample/conversation.py, csrc/kernels_audio.h conversation_audio_kernel).

Channel routing: the dataset loads the stereo `_audio.wav` of a capture as [L, 2], channel 0 the person's own microphone, and
for the partner swaps the two channels (data_loaders/get_data.py:83-88, flip_person).  Normalisation: z-normalisation with the
person's audio statistics (data_loaders/data.py:237); under "peak" each voice is first divided by its own maximum, the demo's
`y / max(y)` (demo/demo.py:179-186) applied to each channel, as a float32 division; under "none" the samples are taken as given.
"""
import numpy as np


def person_audio(chans, p, stats, normalize="peak"):
    """(own, partner) of person p from the resampled channels float32 [2, Lc] -> (normalised float64 [Lc, 2], the un-normalised
    float64 [2, Lc] after the z-normalisation round trip)."""
    u = np.asarray(chans, np.float32)
    if normalize == "peak":
        u = u / u.max(axis=1, keepdims=True)             # float32 division, each channel by its own maximum
    dual = np.stack([u[p], u[1 - p]], axis=-1).astype(np.float64)
    mean = np.asarray(stats["audio_mean"], np.float64).reshape(-1)
    std = float(np.asarray(stats["audio_std_flat"], np.float64).reshape(-1)[0])
    z = np.empty_like(dual)
    z[:, 0] = (dual[:, 0] - mean[0]) / std
    z[:, 1] = (dual[:, 1] - mean[-1]) / std
    return z, (z * std + np.array([mean[0], mean[-1]])).T


def conversation_audio(chans, stats, R, normalize="peak", people=(True, True)):
    """y["audio"] of every animated person: float32 [R, Lc, 2] (None for a person not animated)."""
    out = []
    for p in range(2):
        if not people[p]:
            out.append(None)
            continue
        z, _ = person_audio(chans, p, stats[p], normalize)
        out.append(np.broadcast_to(z.astype(np.float32), (R,) + z.shape).copy())
    return out
