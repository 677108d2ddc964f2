"""Per-frame latency of a stereo frame from a DISTORTED rig, three ways (p50 / p99 over interleaved blocks, one process):
  (a) today's pattern without device undistortion: gfo_extract_stereo (its association thrown away), the keypoints undistorted on the host,
      then gfo_stereo_match on the host arrays -- two device round trips;
  (b) gfo_extract_stereo_un with the rig set on the context (gfo_ctx_set_camera): one submission, association on the device's mvKeysUn;
  (c) gfo_extract_stereo on a context without a camera: the floor (the same work minus the undistortion);
  (d) gfo_extract_stereo on the context WITH the rig: (b)'s device work without returning the undistorted arrays -- (b) - (d) is what
      handing them back costs (two more pack segments, their host copies, two more arrays in the wrapper), (d) - (c) the device side.
The device time of every stage of (b) and (c) is read with the library's per-kernel events (gfo_profile_read, per frame).
Input: the committed EuRoC pair (tests/golden), the EuRoC-magnitude rig of tests/undistort_ref.py.  The host undistortion of (a) is that
file's numpy statement of cv::undistortPoints (vectorised float64), standing in for OpenCV's loop, which is not on this machine; its own
time is reported separately.  (a) and (b) are checked to give the same association before anything is timed.

python tools/undistort_latency.py [--frames 300] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gf_orb_slam2_amd as G  # noqa: E402
import undistort_ref as U  # noqa: E402

LEFT = (U.K_L, U.D_L, U.R_L, U.P_L)
RIGHT = (U.K_R, U.D_R, U.R_R, U.P_R)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gold = os.path.join(ROOT, "tests", "golden")
    iml = np.fromfile(os.path.join(gold, "EuRoC_l_752x480.u8"), np.uint8).reshape(480, 752)
    imr = np.fromfile(os.path.join(gold, "EuRoC_r_752x480.u8"), np.uint8).reshape(480, 752)
    p = G.StereoParams(480, U.BF, U.BF / U.FX_P, 0.0)
    plain = G.ORBextractor(2000, 1.2, 8, 20, 7, max_batch=2)
    cam = G.ORBextractor(2000, 1.2, 8, 20, 7, max_batch=2)
    cam.set_camera(*LEFT, right=RIGHT)
    m = G.ORBmatcher(0.8, True, extractor=plain)
    sf = plain.GetScaleFactors()
    host_us = []

    def frame_a():
        kl, dl, kr, dr = plain.extract_stereo(iml, imr, p)[:4]
        t0 = time.perf_counter()
        ul = U.undistort_keypoints(kl, *LEFT)
        ur = U.undistort_keypoints(kr, *RIGHT)
        host_us.append((time.perf_counter() - t0) * 1e6)
        return m.ComputeStereoMatches(ul, dl, ur, dr, sf, p)

    def frame_b():
        return cam.extract_stereo_un(iml, imr, p)[6:]

    def frame_c():
        return plain.extract_stereo(iml, imr, p)[4:]

    def frame_d():
        return cam.extract_stereo(iml, imr, p)[4:]

    ga, gb = frame_a(), frame_b()
    assert ga[0] == gb[0] and all(x.tobytes() == y.tobytes() for x, y in zip(ga[1:], gb[1:])), "(a) and (b) disagree"
    assert all(x.tobytes() == y.tobytes() for x, y in zip(frame_d()[1:], gb[1:])), "(b) and (d) disagree"
    for f in (frame_a, frame_b, frame_c, frame_d):
        for _ in range(20):
            f()
    host_us.clear()
    per = max(1, a.frames // a.blocks)
    times = {"a": [], "b": [], "c": [], "d": []}
    for _ in range(a.blocks):
        for k, f in (("a", frame_a), ("b", frame_b), ("c", frame_c), ("d", frame_d)):
            for _ in range(per):
                t0 = time.perf_counter()
                f()
                times[k].append((time.perf_counter() - t0) * 1e6)
    res = {"what": "per-frame latency, EuRoC 752x480 stereo pair, distorted rig (tests/undistort_ref.py), 2000 features",
           "frames_each": per * a.blocks, "blocks": a.blocks, "nmatched": int(gb[0])}
    names = {"a": "extract_stereo + host undistortion (numpy) + gfo_stereo_match", "b": "gfo_extract_stereo_un",
             "c": "gfo_extract_stereo, no camera (floor)", "d": "gfo_extract_stereo on the context with the rig (no undistorted arrays back)"}
    for k, v in times.items():
        v = np.array(v)
        res[k] = {"path": names[k], "p50_us": round(float(np.percentile(v, 50)), 1), "p99_us": round(float(np.percentile(v, 99)), 1),
                  "min_us": round(float(v.min()), 1)}
    res["a"]["host_undistortion_p50_us"] = round(float(np.percentile(host_us, 50)), 1)
    res["b_minus_c_p50_us"] = round(res["b"]["p50_us"] - res["c"]["p50_us"], 1)
    res["a_minus_b_p50_us"] = round(res["a"]["p50_us"] - res["b"]["p50_us"], 1)
    res["b_minus_d_p50_us"] = round(res["b"]["p50_us"] - res["d"]["p50_us"], 1)
    res["d_minus_c_p50_us"] = round(res["d"]["p50_us"] - res["c"]["p50_us"], 1)
    # device time per stage and frame (per-kernel events; the profiled run keeps every kernel in one stream)
    for k, e, f in (("b", cam, frame_b), ("c", plain, frame_c)):
        e.profile_enable(True)
        for _ in range(50):
            f()
        prof = e.profile_read()
        e.profile_enable(False)
        res[k]["device_us_per_stage"] = {n: round(ms / 50 * 1e3, 2) for n, (ms, cnt) in prof.items() if cnt}
    res["b"]["undistort_kernel_us"] = res["b"]["device_us_per_stage"].get("undistort")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    plain.close()
    cam.close()


if __name__ == "__main__":
    main()
