#!/usr/bin/env python3
"""The reference's only real images (libstereo-odometry/tests/0L.png / 0R.png, 800x600) as grey arrays: the one photograph
the GPU tests run through the HIP path (tests/test_gpu_frame_layouts.py).  Image data only, nothing else of the reference.

    python tests/golden/make_ref_pair.py <reference tree>

Run where the reference tree is; the .npz is committed."""
import os
import sys

import numpy as np
from PIL import Image

ref = os.path.join(sys.argv[1], "libstereo-odometry", "tests")
L = np.array(Image.open(os.path.join(ref, "0L.png")).convert("L")); R = np.array(Image.open(os.path.join(ref, "0R.png")).convert("L"))
assert L.shape == R.shape == (600, 800) and L.dtype == np.uint8
out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_pair_800x600.npz")
np.savez_compressed(out, left=L, right=R)
print("%s: %d bytes; %.1f %% of the pixels at 255, %.1f %% at 0" % (out, os.path.getsize(out), 100.0 * ((L == 255).mean() + (R == 255).mean()) / 2, 100.0 * ((L == 0).mean() + (R == 0).mean()) / 2))
