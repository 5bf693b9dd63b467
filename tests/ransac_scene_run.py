"""Child process of tests/test_gpu_ransac_forms.py: every case of ransac_scenes.all_cases through stage 4 of a one-lane context, under
whatever launch knobs the environment of THIS process sets (a context reads them when it is created); tracked pairs, counters and
status words go to an .npz for the parent to compare with the oracle.

usage: python ransac_scene_run.py <golden directory> <output .npz>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import ransac_scenes as RS                                                          # noqa: E402


def main(golden_dir, out_path):
    from stereo_vo_amd import hip
    from stereo_vo_amd.abi import StereoCamera, north_star_params
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    cam = StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), int(g["W"]), int(g["H"]))
    p = north_star_params(hip.default_params(), orb_nfeats=int(g["orb_nfeats"]))
    ctx = hip.Context(n_lanes=1, max_w=640, max_h=480, max_kps=1024, max_cand=1 << 15)
    ctx.set_params(p); ctx.set_camera(cam)
    out = {}
    for name, s in RS.all_cases(golden_dir):
        trk, ts, status = RS.run_case(ctx, s)
        out["trk/" + name], out["ts/" + name], out["st/" + name] = trk, np.array(ts, np.int32), np.array(status, np.uint32)
    ctx.close()
    np.savez(out_path, **out)
    print("done %d" % (len(out) // 3))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
