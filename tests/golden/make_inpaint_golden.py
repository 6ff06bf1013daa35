#!/usr/bin/env python3
"""Generate tests/golden/inpaint_masks.npz by IMPORTING THE REFERENCE's modules/utils.py and calling its own
get_inpainting_mask (lines 203-226) and add_salt_and_pepper_noise (lines 114-129) under fixed np.random seeds.  Only data
travels: the three masks at 16 x 12 with mask_frac = 0.5, a 16 x 12 x 3 uint8 image, its noisy copy, and the seeds and
probabilities of the draws.  The reference's module is imported as make_tv_golden.py imports it (stubs stand in for the
plotting and image libraries that are absent).

    python3 tests/golden/make_inpaint_golden.py /path/to/reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_tv_golden import import_reference_utils  # noqa: E402

H, W = 16, 12
MASK_FRAC = 0.5
MASK_SEEDS = {"random2d": 11, "random1d": 12, "bayer": 13}
SP_SEED, SALT, PEPPER = 21, 0.1, 0.15


def main():
    utils = import_reference_utils(sys.argv[1])
    out = {"imsize": np.array([H, W], np.int64), "mask_frac": np.float64(MASK_FRAC),
           "sp_seed": np.int64(SP_SEED), "salt_prob": np.float64(SALT), "pepper_prob": np.float64(PEPPER)}
    for kind, seed in MASK_SEEDS.items():
        np.random.seed(seed)
        m = utils.get_inpainting_mask((H, W), kind, MASK_FRAC)
        assert m.dtype == np.float32 and m.shape == (H, W)
        out["mask_" + kind], out["seed_" + kind] = m, np.int64(seed)
        # what the generator holds after the call: the port must have drawn as many numbers
        out["next_" + kind] = np.float64(np.random.rand())
    image = np.random.default_rng(5).integers(1, 255, (H, W, 3)).astype(np.uint8)
    np.random.seed(SP_SEED)
    noisy = utils.add_salt_and_pepper_noise(image, SALT, PEPPER)
    out["sp_image"], out["sp_noisy"], out["sp_next"] = image, noisy, np.float64(np.random.rand())
    path = os.path.join(HERE, "inpaint_masks.npz")
    np.savez_compressed(path, **out)
    print(path, {k: (v.shape, float(v.mean())) for k, v in out.items() if k.startswith("mask_")},
          "salt", int((noisy == 255).all(-1).sum()), "pepper", int((noisy == 0).all(-1).sum()))


if __name__ == "__main__":
    main()
