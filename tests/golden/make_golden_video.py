"""Writes tests/golden/golden_video_v1.npz: what Pillow (libjpeg) itself writes for the test images of tests/jpeg_restatement.py.
Run where Pillow is installed (12.2 when this file was made):  python tests/golden/make_golden_video.py

  dqt/<quality>           int [2, 64], scan order: the DQT contents of PIL's files at quality 50 / 90 / 100
  dht/<name>/bits, vals   the DHT contents (not optimised), the same in every file
  pil/<quality>_<sub>/psnr, bytes    per image: PSNR of PIL's decode of PIL's own file against the source, and the file's size
  rest/<quality>_<sub>/psnr          per image: PSNR of PIL's decode of the restatement's file
  gap                     the largest shortfall pil psnr - rest psnr over all cases, in dB: what tests/test_video_cpu.py gates on
  excess                  the largest rest psnr - pil psnr.  It is reached at quality 100, where every divisor is 1 and libjpeg's
                          rounding of Y, Cb, Cr to 8-bit integers in front of its integer DCT is the larger part of its error; the
                          restatement does not round there (include/a2p_hip.h "video frames"), so it comes out about 1 dB better
  idct_diff               the largest pixel difference between PIL's and the restatement's decode of the restatement's 4:4:4 files
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_restatement as J  # noqa: E402

QUALITIES, SUBS = (50, 90, 100), {"420": 2, "444": 0}
NAMES = {0x00: "dc_luma", 0x10: "ac_luma", 0x01: "dc_chroma", 0x11: "ac_chroma"}


def pil_file(img, quality, sub):
    buf = io.BytesIO()
    Image.fromarray(img, "RGB").save(buf, format="JPEG", quality=quality, subsampling=SUBS[sub], optimize=False)
    return buf.getvalue()


def pil_decode(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    images = J.source_images()
    out, gaps, idct = {}, [], 0
    for q in QUALITIES:
        for sub in SUBS:
            files = [pil_file(img, q, sub) for img in images]
            heads = [J.parse(f) for f in files]
            for h in heads:
                assert sorted(h["dqt"]) == [0, 1] and sorted(h["dht"]) == sorted(NAMES)
                dqt = np.stack([h["dqt"][0], h["dqt"][1]])
                assert np.array_equal(out.setdefault(f"dqt/{q}", dqt), dqt)
                for key, name in NAMES.items():
                    for part, val in zip(("bits", "vals"), h["dht"][key]):
                        assert np.array_equal(out.setdefault(f"dht/{name}/{part}", np.array(val)), val)
            ours = [J.encode(img, q, sub) for img in images]
            pil = np.array([J.psnr(pil_decode(f), img) for f, img in zip(files, images)])
            rest = np.array([J.psnr(pil_decode(f), img) for f, img in zip(ours, images)])
            out[f"pil/{q}_{sub}/psnr"], out[f"pil/{q}_{sub}/bytes"] = pil, np.array([len(f) for f in files])
            out[f"rest/{q}_{sub}/psnr"], out[f"rest/{q}_{sub}/bytes"] = rest, np.array([len(f) for f in ours])
            gaps += [a - b for a, b in zip(pil, rest)]
            if sub == "444":
                idct = max([idct] + [int(np.abs(pil_decode(f).astype(int) - J.decode(f).astype(int)).max()) for f in ours])
            print(q, sub, "pil", np.round(pil, 3), "rest", np.round(rest, 3), "bytes", out[f"pil/{q}_{sub}/bytes"], out[f"rest/{q}_{sub}/bytes"])
    out["gap"], out["excess"], out["idct_diff"] = np.array(max(gaps)), np.array(-min(gaps)), np.array(idct)
    print("gap", out["gap"], "excess", out["excess"], "idct_diff", idct)
    np.savez_compressed(os.path.join(HERE, "golden_video_v1.npz"), **out)


if __name__ == "__main__":
    main()
