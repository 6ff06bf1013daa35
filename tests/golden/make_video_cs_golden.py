#!/usr/bin/env python3
"""Generate tests/golden/video_cs.npz by IMPORTING THE REFERENCE's modules/lin_inverse.py and calling its own
get_video_coding_frames and video2codedvideo (lines 42-95).  Only data travels: the masks, a random video and the coded
video the reference makes of them.  The reference imports kornia, cv2 and tqdm at module scope for other helpers;
empty stubs stand in for whichever of them is absent, as make_golden.py does.

    python3 tests/golden/make_video_cs_golden.py /path/to/reference
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
VIDEO_SIZE, NFRAMES = (6, 5, 10), 4


def main():
    ref = sys.argv[1]
    for name in ("kornia", "cv2", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, ref)
    from modules import lin_inverse

    np.random.seed(0)
    masks = lin_inverse.get_video_coding_frames(VIDEO_SIZE, NFRAMES)              # (H, W, T) float64
    H, W, T = VIDEO_SIZE
    video = np.random.default_rng(1).standard_normal((1, T, H, W)).astype(np.float32)
    masks_ten = torch.tensor(masks.astype(np.float32)).permute(2, 0, 1)[None]     # (1, T, H, W)
    coded = lin_inverse.video2codedvideo(torch.tensor(video), masks_ten, NFRAMES).numpy()
    out = os.path.join(HERE, "video_cs.npz")
    np.savez(out, masks=masks, video=video, coded=coded, video_size=np.array(VIDEO_SIZE), nframes=np.array(NFRAMES))
    print(out, "masks", masks.shape, masks.dtype, "video", video.shape, "coded", coded.shape, coded.dtype)


if __name__ == "__main__":
    main()
