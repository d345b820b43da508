"""Generates tests/golden/place.npz: the reference's own ``project_to_2d``, ``project_to_2d_linear`` (hpe/mh_so3_hpe/data/camera.py:35-95) and
``camera_to_world`` (:31-32, qrot of data/quaternion.py) on float64 tensors, for the tests of mp_lift_place / mp_lift_world.  Data only.

    python tools/gen_golden_place.py          (where oracle/gen_golden.py finds the reference)

Inputs: a seeded (6, 5, 17, 3) batch of camera-space points with depth in 3..7 m (the five points sets of a frame are the first one moved by
0.05 N(0, 1): hypotheses of one frame), two frames of it moved sideways until X / Z exceeds 1 (the clamp of the camera model), subject S11's four
cameras (frame i has camera i % 4) and keypoints = pinhole projection of the first set + 0.01 N(0, 1).  Every input is a float32 value held in
float64, so the device, which reads float32, sees the numbers the reference saw.  The reference's functions are evaluated at the points themselves
(``proj``, ``proj_linear``, ``world``) and at the points moved by the fitted translation (``proj_fit``, ``proj_linear_fit``: what mp_lift_place's
reprojection error is made of); that translation, ``t_fit``, is our own float64 statement of the fit (tests/lift_place_ref.py), not the
reference's - it has none.  Only data/camera.py and data/quaternion.py are imported: the reference's prepare_prediction_for_viz lives in
visualization/utils.py, which pulls in matplotlib, so its floor line (``prediction[..., 2] -= np.min(prediction[..., 2])``) is restated here
in numpy (``world_floor``, each frame's array on its own)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden  # noqa: E402
import lift_place_ref as own  # noqa: E402


def main():
    gen_golden.import_reference()                 # puts the reference's hpe/ folder on sys.path
    from mh_so3_hpe.data import camera as cam
    from manipose_amd.data.ingest import h36m_cameras
    s11 = h36m_cameras()["S11"]
    cams = [s11[i % 4] for i in range(6)]
    intr = np.stack([c["intrinsic"] for c in cams]).astype(np.float32)
    quat = np.stack([c["orientation"] for c in cams]).astype(np.float32)
    g = np.random.default_rng(2024)
    rel = 0.3 * g.standard_normal((6, 1, 17, 3))
    rel = np.concatenate([rel, rel + 0.05 * g.standard_normal((6, 4, 17, 3))], axis=1)
    rel[:, :, 0] = 0
    centre = np.concatenate([g.uniform(-1, 1, (6, 2)), g.uniform(3, 7, (6, 1))], axis=1)
    centre[4, 0], centre[5, 1] = 1.5 * centre[4, 2], -1.3 * centre[5, 2]          # X / Z > 1 in frame 4, Y / Z < -1 in frame 5
    X = (rel + centre[:, None, None, :]).astype(np.float32).astype(np.float64)
    pin = intr[:, None, 0:2].astype(np.float64) * (X[:, 0, :, :2] / X[:, 0, :, 2:3]) + intr[:, None, 2:4].astype(np.float64)
    kp = (pin + 0.01 * g.standard_normal((6, 17, 2))).astype(np.float32).astype(np.float64)
    t_fit = np.stack([np.stack([own.place_one(X[n, i], kp[n], intr[n])[0] for i in range(5)]) for n in range(6)])       # (6, 5, 3)
    P = torch.from_numpy(intr.astype(np.float64))
    out = {"X": X, "kp": kp, "intr": intr, "quat": quat, "t_fit": t_fit}
    for tag, pts in (("", X), ("_fit", X + t_fit[:, :, None, :])):
        out["proj" + tag] = cam.project_to_2d(torch.from_numpy(pts), P).numpy()
        out["proj_linear" + tag] = cam.project_to_2d_linear(torch.from_numpy(pts), P).numpy()
    world = np.stack([cam.camera_to_world(X[n], quat[n].astype(np.float64), 0) for n in range(6)])
    out["world"] = world
    floored = world.copy()
    for n in range(6):
        floored[n, ..., 2] -= np.min(floored[n, ..., 2])
    out["world_floor"] = floored
    assert all(v.dtype == (np.float32 if k in ("intr", "quat") else np.float64) for k, v in out.items())
    clamped = np.abs(X[..., :2] / X[..., 2:3]).max(axis=(1, 2, 3)) > 1
    assert clamped.tolist() == [False, False, False, False, True, True]
    path = os.path.join(ROOT, "tests", "golden", "place.npz")
    np.savez_compressed(path, **out)
    print("place: ok", {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
