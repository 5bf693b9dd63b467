"""Writes tests/golden/faster_kat.npz: the lists tests/faster_ref.py produces on two committed inputs, so that a change of the
reference definitions (FAST-12 segment test, KLT response, the composition with the oracle's NMS and row sort) shows up as a diff
of a committed file.  Lists only: per case, octave and side the final keypoints (x, y as uint16, response as float32), the raw
corner count and a CRC of the raw corner records.

    python tests/golden/make_faster_kat.py        (from the repository root; needs oracle/libsvo_oracle.so)"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import faster_ref as F                                          # noqa: E402
from oracle import oracle as O                                  # noqa: E402

CASES = (("photo_t20", "ref_pair_800x600.npz", "left", "right", 20), ("photo_t10", "ref_pair_800x600.npz", "left", "right", 10),
         ("small_t20", "oracle_small_seq.npz", "L0", "R0", 20))
N_OCT, NFEATS, WIN = 3, 500, 4


def lists(golden_dir):
    out = {}
    for name, fn, kl, kr, t in CASES:
        g = np.load(os.path.join(golden_dir, fn))
        p = F.faster_params(O.default_params(), t=t, orb_nfeats=NFEATS, n_oct=N_OCT)
        imgs = (F.pyramid(g[kl], N_OCT), F.pyramid(g[kr], N_OCT))
        for o, f in enumerate(F.faster_features(g[kl], g[kr], p, WIN)):
            for side in (0, 1):
                k = f[side]
                raw = F.corners(imgs[side][o], t, WIN)
                tag = "%s_o%d_s%d_" % (name, o, side)
                out[tag + "xy"] = np.stack([k["x"], k["y"]], 1).astype(np.uint16)
                out[tag + "resp"] = k["response"].copy()
                out[tag + "raw"] = np.array([len(raw), zlib.crc32(raw.tobytes())], np.int64)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "faster_kat.npz"), **lists(HERE))
    print("wrote faster_kat.npz, %d bytes" % os.path.getsize(os.path.join(HERE, "faster_kat.npz")))
